"""Shared cases of the loss-term kernels of csrc/losses.hip (the triple-loss kernels have their own files) -- the multi-tensor L1
and MSE-to-constant sums (msmc_l1_multi_fwd_ws / msmc_mse_const_multi_fwd_ws, the atomic msmc_l1_multi_fwd /
msmc_mse_const_multi_fwd, msmc_l1_multi_bwd / msmc_mse_const_multi_bwd), the masked means (msmc_masked_mean_fwd / _bwd) and the
weighted sum of scalars (msmc_scalar_wsum_fwd / _bwd) -- through the C entries, and of hip/losses.py mse_const_halves and
weighted_sum: tests/test_losses_emu.py runs them on the kernel interpreter, tests/test_gpu_losses.py on the GPU.

Reference of every comparison: plain float64 torch on the CPU from the same fp32 / bf16 input bits (abs, square, sum, /, and
float64 autograd for the Python functions); ``target``, the weights and gout are rounded to fp32 first.  No reference restates
blocks, lanes or alignment.  Every output is pre-filled with NaN with GUARD NaN elements before and behind it (gradients of one
table are views into ONE buffer with GUARD NaN elements between neighbours); the guards keep their bits; every non-atomic case
runs twice and the two results agree bit for bit.

Bars (u = 2^-24, ONE = 1 + 2^-20, h(r) = half a bf16 ulp of the float64 reference r where the output is bf16; VE = 4 elements of a
16-byte vector in fp32, 8 in bf16):
  exact-sum cases   L1 operands are multiples of 1/8 in [-4, 4] (|a - b| is a multiple of 1/8, at most 8: 64 n < 2^24), MSE and
                    masked-mean operands multiples of 1/2 in [-2, 2] with targets 0 and 1 ((a - t)^2 is a multiple of 1/4, at most
                    9, (a - b)^2 at most 16: 64 n < 2^24), each condition checked in float64 in the test: every partial sum is
                    exact in fp32 in any order.  What is left: the division S_i / n_i of each tensor (u each) and the tree over
                    the count <= 64 tensors, one per work-item, ceil(log2 count) additions deep:
                        multi-tensor forward   (1 + ceil(log2 count)) u sum_i S_i / n_i
                        masked mean            out[0] = S / tot / C: 2 u |ref|;  out[1] = 1 / tot / C: 2 u ref
                    An omitted, doubled or misplaced element moves a sum by at least 1/8 (1/4): at the largest tensor (137 219
                    elements, mean about 2.7) that is 3.4e-7 relative against 6e-8.
  random cases      D u sum |terms| / n, D counted from the kernel: a work-item of the ws forward folds
                    ceil(nv / (64 * 256)) vectors of VE elements and one tail element, c = ceil(n / VE / 16384) VE + 1; each
                    term carries the rounding of a - b (L1: 1) or of a - target twice in the square (MSE: 2; the fmaf rounds once
                    more, counted in c); the workgroup tree 8; loss_multi_final_kernel adds the 64 partials in order (64), divides
                    (1) and its tree adds 8:  D = c + (1 | 2) + 8 + 64 + 1 + 8.  Atomic forwards: bx = min(256,
                    ceil(nmax / 4096)) blocks per tensor, c = ceil(n / VE / (256 bx)) VE + 1, the quotient per block (1) and
                    bx count atomic additions in any order: D = c + (1 | 2) + 8 + 1 + bx count; same bar, no run-twice equality.
                    Masked mean: c = ceil(T C / 8192) (+ 2 in mode 1), 8, ceil(32 B / 256) in the final kernel, 8, two quotients.
  L1 gradient       bit equality: +-fp32(gout / fp32(n)) by the sign of a - b, +0 where a == b (among them +0 against -0), rounded
                    once to bf16.
  MSE gradient      2 (a - target) fp32(gout / n): the difference, the quotient, the product: 3 u |ref| ONE + h(ref).
  masked-mean grad  fed with the kernel's own out; k = fp32(gout out[1]).  Mode 0: ga == k, gb == -k bit for bit (rounded once
                    to the storage type).  Mode 1: 2 (a - b) k: the difference and the product, 2 u |ref| ONE + h(ref).  Every
                    padding row (t >= the clamped length) of ga AND gb is +0 bit for bit.
  lengths           the numerator clamps a length to 0 .. T, the denominator is the plain sum of the lengths as given (as in the
                    reference trainer): T + 5 and -2 in one batch, sum kept positive.
  weighted sum      forward: n fmaf in term order, n u sum |w x|; backward gout * w[i] bit for bit.
  mse_const_halves  values: exact-sum inputs, the multi-tensor forward bar; gradients: the MSE gradient bar with the weight of the
                    half folded into gout (weights 1 and 0.5, exact).  A half whose output is not used: its rows of every
                    gradient are +0 bit for bit.

Which case reaches which path (fp32 / bf16 each):
  loss_multi_fwd_kernel   n = 1, VE - 1 (tail only), VE (one vector), VE + 1, 256 VE - 1, 256 VE + 1 (a second block), BIG =
                          64 * 256 * VE + 3 * 256 * VE + 3 (second and third grid-stride trip of some blocks, and a tail), the table
                          (1, BIG) (63 blocks past the small tensor's end), 64 tensors; a and b alone one element into their
                          buffer (vec false: the element loop takes everything)
  loss_multi_final_kernel count = 1, 2, 64
  atomic forwards         the same sizes without BIG's table twice
  loss_multi_bwd_kernel   the same sizes; a, b, ga alone one element in (L1 with only ga misaligned among them); past the block cap
                          (nmax > 4096 * 256): CAP_GPU = 1 052 675 fp32 elements on the GPU; the interpreter runs CAP_EMU =
                          262 147, the largest size it finishes in seconds (below the cap: the cap itself is a GPU case)
  masked means            all four dtype pairs in mode 1, fp32 and bf16 in mode 0, int32 and int64 lengths, (B, T, C) = (1, 1, 1),
                          (2, 7, 5), (9, 3, 4) (B 32 > 256: second trip of the final kernel), (3, 50, 80) and (2, 103, 80): T C =
                          8240 > 32 * 256, a second trip of the partial loop, which (3, 50, 80), 4000 elements, does not reach;
                          backward with ga only, gb only and both
  scalar_wsum             n = 1, 2, 64
  refusals                as coded: count 0 / 65, n[i] <= 0, NULL table -> SHAPE, NULL partial -> WORKSPACE; masked mean: B, T,
                          C <= 0, NULL a / lengths / out, mode 2, mode 1 without b, a dtype code of 2 -> SHAPE, forward without
                          partial -> WORKSPACE, backward without gout -> SHAPE; wsum: n 0 / 65, NULL term / weights / out.
Every comparison is appended to MEASURED and printed; the figures are recorded in profiles/loss_optim_direct.md.
"""
import ctypes
import math

import numpy as np
import torch

from _spectralcases import _nan, same_bits, twice
from _normcases import U, E_SHAPE, E_WORKSPACE, GUARD, DTYPES, half_ulp, Out, at, L, gen_for
from _wnormcases import all_nan
from _optimcases import arena, views_of, f32
import _normcases

ONE = 1.0 + 2.0 ** -20
MEASURED = []
FLOOR_HELD = set()
BOOK = (MEASURED, FLOOR_HELD, 'losses')
WS_BX = 64
CAP_GPU = 4096 * 256 + 4096 + 3
CAP_EMU = 262144 + 3


def held(what, case, got, ref, bound):
    _normcases.held(what, case, got, ref, bound, book=BOOK)


def ve_of(which):
    return 4 if which == 0 else 8


def big(which):
    return 64 * 256 * ve_of(which) + 3 * 256 * ve_of(which) + 3


def sizes(which):
    ve = ve_of(which)
    return (1, ve - 1, ve, ve + 1, 256 * ve - 1, 256 * ve + 1, big(which))


SIZE_KEYS = ('1', 've-1', 've', 've+1', '256ve-1', '256ve+1', 'big')
TABLE_KEYS = SIZE_KEYS + ('mixed', 'sixty-four')


def tables(which):
    """name -> the sizes of the tensors of one table"""
    ve = ve_of(which)
    t = {k: (n,) for k, n in zip(SIZE_KEYS, sizes(which))}
    t['mixed'] = (1, big(which))
    t['sixty-four'] = tuple((1, ve - 1, ve, ve + 1, 256 * ve - 1, 256 * ve + 1, 3, 2 * ve + 1)[i % 8] for i in range(64))
    return t


def loss_inputs(ns, which, mode, exact, key):
    """-> lists a, b (b: L1 only) of CPU tensors in the storage type"""
    dtype = DTYPES[which][1]
    a, b = [], []
    for i, n in enumerate(ns):
        gen = gen_for(600, key, i, n, which, mode)
        if exact and mode == 0:
            x, y = (torch.randint(-32, 33, (n,), generator=gen).float() / 8 for _ in range(2))
        elif exact:
            x, y = torch.randint(-4, 5, (n,), generator=gen).float() / 2, None
        else:
            x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        if mode == 0:
            k = torch.arange(n)
            y = torch.where(k % 5 == 2, x, y)                               # a == b
            x = torch.where(k % 11 == 3, torch.zeros(n), x)                 # +0 against -0
            y = torch.where(k % 11 == 3, -torch.zeros(n), y)
            b.append(y.to(dtype))
        a.append(x.to(dtype))
    return a, b


def table_of(a_views, b_views, ga_views, ns, which):
    tab = L().TensorTable()
    tab.count, tab.dtype = len(ns), which
    for i, n in enumerate(ns):
        tab.a[i], tab.n[i] = a_views[i], n
        tab.b[i] = b_views[i] if b_views else None
        tab.ga[i] = ga_views[i] if ga_views else None
    return tab


def placed(ts, dev, off):
    """the tensors one behind the other in one zero-padded buffer, tensor k ``off[k]`` elements behind a 16-byte boundary -> the
    buffer (kept alive by the caller) and the pointers"""
    esz = ts[0].element_size()
    per = 16 // esz
    pos, o = [], 0
    for t, f in zip(ts, off):
        o = (o + per - 1) // per * per + f
        pos.append(o)
        o += t.numel() + GUARD
    buf = torch.zeros(o, dtype=ts[0].dtype)
    for t, s in zip(ts, pos):
        buf[s:s + t.numel()] = t
    buf = buf.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf.data_ptr() + esz * s for s in pos]


def terms64(a, b, mode, target):
    return [(x.double() - y.double()).abs() if mode == 0 else (x.double() - target) ** 2 for x, y in zip(a, b or a)]


def d_fwd(n, which, mode, atomic, nmax, count):
    ve = ve_of(which)
    if atomic:
        bx = min(256, (nmax + 4095) // 4096)
        c = ((n + ve - 1) // ve + 256 * bx - 1) // (256 * bx) * ve + 1
        return c + (1 if mode == 0 else 2) + 8 + 1 + bx * count
    c = ((n + ve - 1) // ve + 16383) // 16384 * ve + 1
    return c + (1 if mode == 0 else 2) + 8 + 64 + 1 + 8


def check_forward(dev, which, mode, name, exact, atomic=False, off=(0, 0)):
    """one table through the ws forward (or the atomic one) against float64"""
    lib = L()
    ns = tables(which)[name]
    dtn = DTYPES[which][2]
    for target in ((0.0, 1.0) if mode == 1 else (0.0,)):
        a, b = loss_inputs(ns, which, mode, exact, 0)
        abuf, ap = placed(a, dev, [off[0]] * len(ns))
        bbuf, bp = placed(b, dev, [off[1]] * len(ns)) if mode == 0 else (None, None)
        tab = table_of(ap, bp, None, ns, which)
        nparts = int(lib.get().msmc_loss_multi_parts())
        assert nparts == 64 * WS_BX

        def run():
            out, part = Out((1,), dev, off=GUARD), Out((nparts,), dev)
            st = lib.stream(abuf)
            if atomic:
                if mode == 0:
                    lib.call('msmc_l1_multi_fwd', ctypes.byref(tab), lib.ptr(out.t), st)
                else:
                    lib.call('msmc_mse_const_multi_fwd', ctypes.byref(tab), target, lib.ptr(out.t), st)
            elif mode == 0:
                lib.call('msmc_l1_multi_fwd_ws', ctypes.byref(tab), lib.ptr(part.t), lib.ptr(out.t), st)
            else:
                lib.call('msmc_mse_const_multi_fwd_ws', ctypes.byref(tab), target, lib.ptr(part.t), lib.ptr(out.t), st)
            p = part.get(written=False)
            if not atomic:
                assert all_nan(p[len(ns) * WS_BX:]) and not bool(torch.isnan(p[:len(ns) * WS_BX]).any())
            return (out.get(),)

        got = run()[0] if atomic else twice(run)[0]
        terms = terms64(a, b, mode, target)
        means = [float(t.sum()) / n for t, n in zip(terms, ns)]
        ref = torch.tensor([sum(means)], dtype=torch.float64)
        tag = '%s %s %s%s%s' % (('l1', 'mse t%g' % target)[mode], name, dtn, ' atomic' if atomic else '',
                                ' off a%d b%d' % off if any(off) else '')
        if exact and not atomic:
            q = 8.0 if mode == 0 else 4.0
            for t, n in zip(terms, ns):
                assert float(t.sum()) * q < 2 ** 24 and bool((t * q == (t * q).round()).all()), 'the sums of this case are not exact'
            depth = math.ceil(math.log2(len(ns))) if len(ns) > 1 else 0
            bound = (1 + depth) * U * sum(means) * ONE
            what = 'fwd exact'
        else:
            bound = sum(d_fwd(n, which, mode, atomic, max(ns), len(ns)) * U * m for n, m in zip(ns, means)) * ONE
            what = 'fwd atomic' if atomic else 'fwd random'
        held(what, tag, got, ref, torch.tensor([bound], dtype=torch.float64))


def check_backward(dev, which, mode, name, off=(0, 0, 0), ns=None, gout=0.75):
    """both gradients kernels over one table: the L1 gradient bit for bit, the MSE gradient within 3 u"""
    lib = L()
    ns = tables(which)[name] if ns is None else ns
    code, dtype, dtn = DTYPES[which]
    g32 = torch.tensor([f32(gout)], dtype=torch.float32)
    for target in ((0.0, 1.0) if mode == 1 else (0.0,)):
        a, b = loss_inputs(ns, which, mode, False, 1)
        abuf, ap = placed(a, dev, [off[0]] * len(ns))
        bbuf, bp = placed(b, dev, [off[1]] * len(ns)) if mode == 0 else (None, None)
        gd = g32.to(dev)

        def run():
            per = 16 // a[0].element_size()
            pos, o = [], GUARD
            for n in ns:
                o = (o + per - 1) // per * per + off[2]
                pos.append(o)
                o += n + GUARD
            gbuf = _nan((o,), dev, dtype)
            assert gbuf.data_ptr() % 16 == 0
            tab = table_of(ap, bp, [gbuf.data_ptr() + a[0].element_size() * s for s in pos], ns, which)
            if mode == 0:
                lib.call('msmc_l1_multi_bwd', ctypes.byref(tab), lib.ptr(gd), lib.stream(gd))
            else:
                lib.call('msmc_mse_const_multi_bwd', ctypes.byref(tab), target, lib.ptr(gd), lib.stream(gd))
            vs, clean = views_of(gbuf.cpu(), pos, ns)
            assert clean, 'an element outside the gradients was written'
            return tuple(vs)

        got = twice(run)
        tag = '%s %s %s%s' % (('l1', 'mse t%g' % target)[mode], name, dtn, ' off a%d b%d ga%d' % off if any(off) else '')
        for i, (n, g) in enumerate(zip(ns, got)):
            scale32 = g32 / torch.tensor([float(n)], dtype=torch.float32)          # one correctly rounded fp32 quotient
            if mode == 0:
                d = a[i].double() - b[i].double()
                want = torch.where(d > 0, scale32, torch.where(d < 0, -scale32, torch.zeros(1))).to(dtype)
                assert bool((d == 0).any()) or n < 3
                assert same_bits(g, want), '%s tensor %d: the L1 gradient is not +-fp32(gout / n) or +0' % (tag, i)
            else:
                ref = 2.0 * (a[i].double() - target) * (f32(gout) / n)
                held('bwd mse', '%s #%d' % (tag, i), g, ref, 3 * U * ref.abs() * ONE + half_ulp(ref, dtype))
        if mode == 0:
            MEASURED.append(('bwd l1', tag, 0.0, 'bit equality'))
            print('losses %-26s %-34s bit-equal' % ('bwd l1', tag))


def check_multi_refusals(dev):
    lib = L()
    G = lib.get()
    a = torch.randn(40).to(dev)
    nparts = int(G.msmc_loss_multi_parts())
    out, part = Out((1,), dev), Out((nparts,), dev)
    ga = Out((40,), dev)
    gout = torch.ones(1).to(dev)
    st = lib.stream(a)

    def tab(count, n0=40):
        t = lib.TensorTable()
        t.count, t.dtype = count, 0
        for i in range(min(max(count, 1), 64)):
            t.a[i], t.b[i], t.ga[i], t.n[i] = a.data_ptr(), a.data_ptr(), ga.t.data_ptr(), 40
        t.n[0] = n0
        return t

    bad = [tab(0), tab(65), tab(-1), tab(2, 0), tab(2, -5)]
    for t in bad:
        r = ctypes.byref(t)
        rcs = [G.msmc_l1_multi_fwd_ws(r, lib.ptr(part.t), lib.ptr(out.t), st), G.msmc_mse_const_multi_fwd_ws(r, 1.0, lib.ptr(part.t), lib.ptr(out.t), st),
               G.msmc_l1_multi_fwd(r, lib.ptr(out.t), st), G.msmc_mse_const_multi_fwd(r, 1.0, lib.ptr(out.t), st),
               G.msmc_l1_multi_bwd(r, lib.ptr(gout), st), G.msmc_mse_const_multi_bwd(r, 1.0, lib.ptr(gout), st)]
        assert rcs == [E_SHAPE] * 6, rcs
    rcs = [G.msmc_l1_multi_fwd_ws(None, lib.ptr(part.t), lib.ptr(out.t), st), G.msmc_mse_const_multi_fwd_ws(None, 1.0, lib.ptr(part.t), lib.ptr(out.t), st),
           G.msmc_l1_multi_fwd(None, lib.ptr(out.t), st), G.msmc_mse_const_multi_fwd(None, 1.0, lib.ptr(out.t), st),
           G.msmc_l1_multi_bwd(None, lib.ptr(gout), st), G.msmc_mse_const_multi_bwd(None, 1.0, lib.ptr(gout), st)]
    assert rcs == [E_SHAPE] * 6, rcs
    good = tab(1)
    assert G.msmc_l1_multi_fwd_ws(ctypes.byref(good), None, lib.ptr(out.t), st) == E_WORKSPACE
    assert G.msmc_mse_const_multi_fwd_ws(ctypes.byref(good), 1.0, None, lib.ptr(out.t), st) == E_WORKSPACE
    assert all_nan(out.get(written=False)) and all_nan(part.get(written=False)) and all_nan(ga.get(written=False)), \
        'a refused call wrote something'


# ---- mse_const_halves (hip/losses.py) -------------------------------------------------------------------------------------------------
HALF_ROWS = ((1,), (3,), (5,), (2, 4))


def check_halves(dev, which, B, use):
    """use: 'both' | 'first' | 'second' -- which outputs enter the scalar that is differentiated"""
    from msmctts_amd.hip import losses
    code, dtype, dtn = DTYPES[which]
    gen = gen_for(700, which, B)
    xs = [(torch.randint(-4, 5, (2 * B,) + r, generator=gen).float() / 2).to(dtype) for r in HALF_ROWS]
    ts = [x.clone().to(dev).requires_grad_(True) for x in xs]
    assert any(t[B:].data_ptr() % 16 for t in ts), 'no second half starts off a 16-byte boundary'
    w = {'both': (1.0, 0.5), 'first': (1.0, None), 'second': (None, 0.5)}[use]
    o0, o1 = losses.mse_const_halves(ts, B, 0.0, 1.0)
    tot = sum(wk * o for wk, o in zip(w, (o0, o1)) if wk is not None)
    tot.backward()
    rs = [x.double().requires_grad_(True) for x in xs]
    r0 = sum((r[:B] ** 2).mean() for r in rs)
    r1 = sum(((r[B:] - 1.0) ** 2).mean() for r in rs)
    sum(wk * o for wk, o in zip(w, (r0, r1)) if wk is not None).backward()
    tag = 'B%d %s %s' % (B, dtn, use)
    for got, ref in ((o0, r0), (o1, r1)):
        ref = ref.detach().reshape(1)
        held('halves value', tag, got.detach().cpu().reshape(1), ref, (1 + 2) * U * ref.abs() * ONE)
    for i, (t, r) in enumerate(zip(ts, rs)):
        g = t.grad.cpu()
        assert g.dtype == dtype and g.shape == r.shape
        held('halves grad', '%s #%d' % (tag, i), g, r.grad, 3 * U * r.grad.abs() * ONE + half_ulp(r.grad, dtype))
        for k, rows in enumerate((g[:B], g[B:])):
            if w[k] is None:
                assert same_bits(rows, torch.zeros_like(rows)), '%s #%d: the rows of the unused half are not +0' % (tag, i)


# ---- masked means ----------------------------------------------------------------------------------------------------------------------
MM_SHAPES = {(1, 1, 1): ((1,), (6,)), (2, 7, 5): ((12, -2), (7, 0)), (9, 3, 4): ((0, 1, 3, 8, -2, 3, 2, 1, 0),),
             (3, 50, 80): ((50, 55, 1),), (2, 103, 80): ((103, 108),)}
MM_PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1))


def mm_d(B, T, C, mode):
    return (T * C + 8191) // 8192 + (2 if mode == 1 else 0) + 8 + (32 * B + 255) // 256 + 8 + 2


def check_masked_mean(dev, shape, wa, wb, mode, len64, exact, grads=('both', 'ga', 'gb'), gout=1.5):
    lib = L()
    B, T, C = shape
    ta, tb = DTYPES[wa][1], DTYPES[wb][1]
    for li, lens in enumerate(MM_SHAPES[shape]):
        assert sum(lens) > 0
        gen = gen_for(800, B, T, C, wa, wb, mode, li)
        if exact:
            a, b = ((torch.randint(-4, 5, (B, T, C), generator=gen).float() / 2) for _ in range(2))
        else:
            a, b = torch.randn(B, T, C, generator=gen), torch.randn(B, T, C, generator=gen)
        a, b = a.to(ta), (b.to(tb) if mode == 1 else None)
        ln = torch.tensor(lens, dtype=torch.int64 if len64 else torch.int32)
        ad, bd, ld = a.to(dev), (b.to(dev) if mode == 1 else None), ln.to(dev)
        nparts = int(lib.get().msmc_masked_mean_parts(B))
        assert nparts == 32 * B
        gd = torch.tensor([f32(gout)]).to(dev)
        valid = (torch.arange(T)[None, :] < ln.clamp(0, T)[:, None].long())[:, :, None].expand(B, T, C)
        tag = '%dx%dx%d %s/%s m%d %s len %s' % (B, T, C, DTYPES[wa][2], DTYPES[wb][2], mode, 'i64' if len64 else 'i32', list(lens))

        def run():
            out, part = Out((2,), dev, off=GUARD), Out((nparts,), dev)
            lib.call('msmc_masked_mean_fwd', lib.ptr(ad), lib.ptr(bd), lib.ptr(ld), int(len64), B, T, C, wa, wb, mode,
                     lib.ptr(part.t), lib.ptr(out.t), lib.stream(ad))
            part.get()
            res = [out.get()]
            for which in grads:
                ga = Out((B, T, C), dev, ta, off=GUARD) if which != 'gb' else None
                gb = Out((B, T, C), dev, tb if mode == 1 else ta, off=GUARD) if which != 'ga' else None
                lib.call('msmc_masked_mean_bwd', lib.ptr(ad), lib.ptr(bd), lib.ptr(ld), int(len64), B, T, C, wa, wb, mode,
                         lib.ptr(out.t), lib.ptr(gd), lib.ptr(ga.t) if ga else None, lib.ptr(gb.t) if gb else None, lib.stream(ad))
                res += [ga.get() if ga else torch.zeros(0), gb.get() if gb else torch.zeros(0)]
            return tuple(res)

        got = twice(run)
        out = got[0]
        term = a.double() if mode == 0 else (a.double() - b.double()) ** 2
        term = torch.where(valid, term, torch.zeros_like(term))
        tot = float(sum(lens))
        ref = torch.tensor([float(term.sum()) / tot / C, 1.0 / tot / C], dtype=torch.float64)
        if exact:
            q = 2.0 if mode == 0 else 4.0
            assert float(term.abs().sum()) * q < 2 ** 24 and bool((term * q == (term * q).round()).all())
            held('masked mean exact', tag, out, ref, 2 * U * ref.abs() * ONE)
        else:
            bound = torch.tensor([mm_d(B, T, C, mode) * U * float(term.abs().sum()) / tot / C, 2 * U * float(ref[1])], dtype=torch.float64)
            held('masked mean random', tag, out, ref, bound * ONE)
        k32 = torch.tensor([f32(gout)]) * out[1:2]                                   # fp32 product, as the kernel forms it
        for j, which in enumerate(grads):
            ga, gb = got[1 + 2 * j], got[2 + 2 * j]
            for name, g, sign, dt in (('ga', ga, 1.0, ta), ('gb', gb, -1.0, tb if mode == 1 else ta)):
                if g.numel() == 0:
                    continue
                assert same_bits(g[~valid], torch.zeros(int((~valid).sum()), dtype=dt)), '%s %s %s: a padding row is not +0' % (tag, which, name)
                if mode == 0:
                    want = (sign * k32).to(dt).expand(int(valid.sum()))
                    assert same_bits(g[valid], want.contiguous()), '%s %s %s: not gout * out[1] bit for bit' % (tag, which, name)
                else:
                    r = sign * 2.0 * (a.double() - b.double()) * float(k32)
                    held('masked mean ' + name, '%s %s' % (tag, which), g[valid], r[valid], 2 * U * r[valid].abs() * ONE + half_ulp(r[valid], dt))


def check_masked_mean_refusals(dev):
    lib = L()
    G = lib.get()
    B, T, C = 2, 3, 4
    a = torch.randn(B, T, C).to(dev)
    ln = torch.tensor([3, 2], dtype=torch.int32).to(dev)
    out, part, ga = Out((2,), dev), Out((32 * B,), dev), Out((B, T, C), dev)
    gout = torch.ones(1).to(dev)
    st = lib.stream(a)
    A, Ln, O, P, GA, GO = lib.ptr(a), lib.ptr(ln), lib.ptr(out.t), lib.ptr(part.t), lib.ptr(ga.t), lib.ptr(gout)
    f, bw = G.msmc_masked_mean_fwd, G.msmc_masked_mean_bwd
    rcs = [f(A, A, Ln, 0, 0, T, C, 0, 0, 1, P, O, st), f(A, A, Ln, 0, B, 0, C, 0, 0, 1, P, O, st), f(A, A, Ln, 0, B, T, -1, 0, 0, 1, P, O, st),
           f(None, A, Ln, 0, B, T, C, 0, 0, 1, P, O, st), f(A, A, None, 0, B, T, C, 0, 0, 1, P, O, st), f(A, A, Ln, 0, B, T, C, 0, 0, 1, P, None, st),
           f(A, A, Ln, 0, B, T, C, 0, 0, 2, P, O, st), f(A, None, Ln, 0, B, T, C, 0, 0, 1, P, O, st), f(A, A, Ln, 0, B, T, C, 2, 0, 1, P, O, st),
           f(A, A, Ln, 0, B, T, C, 0, 2, 1, P, O, st),
           bw(A, A, Ln, 0, B, T, C, 0, 0, 1, O, None, GA, None, st), bw(A, None, Ln, 0, B, T, C, 0, 0, 1, O, GO, GA, None, st),
           bw(A, A, Ln, 0, B, T, C, 0, 0, 1, None, GO, GA, None, st), bw(A, A, Ln, 0, 0, T, C, 0, 0, 1, O, GO, GA, None, st)]
    assert rcs == [E_SHAPE] * len(rcs), rcs
    assert f(A, A, Ln, 0, B, T, C, 0, 0, 1, None, O, st) == E_WORKSPACE and f(A, None, Ln, 0, B, T, C, 0, 0, 0, None, O, st) == E_WORKSPACE
    assert all_nan(out.get(written=False)) and all_nan(part.get(written=False)) and all_nan(ga.get(written=False)), \
        'a refused call wrote something'


# ---- weighted sums of scalars ---------------------------------------------------------------------------------------------------------
def check_wsum(dev, n):
    lib = L()
    gen = gen_for(900, n)
    x, w = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    gout = torch.randn(1, generator=gen)
    xd, gd = at(x, dev, 1), gout.to(dev)
    vp, fp = ctypes.c_void_p * n, ctypes.c_float * n
    terms, ws = vp(*[xd.data_ptr() + 4 * i for i in range(n)]), fp(*w.tolist())

    def run():
        out, gv = Out((1,), dev, off=GUARD), Out((n,), dev, off=GUARD)
        lib.call('msmc_scalar_wsum_fwd', terms, ws, n, lib.ptr(out.t), lib.stream(gd))
        lib.call('msmc_scalar_wsum_bwd', lib.ptr(gd), ws, n, lib.ptr(gv.t), lib.stream(gd))
        return out.get(), gv.get()

    out, gv = twice(run)
    prod = w.double() * x.double()
    held('wsum fwd', 'n%d' % n, out, prod.sum().reshape(1), n * U * prod.abs().sum().reshape(1) * ONE)
    assert same_bits(gv, gout * w), 'n%d: the gradients are not gout * w[i] bit for bit' % n


def check_wsum_refusals(dev):
    lib = L()
    G = lib.get()
    x = torch.randn(70).to(dev)
    out, gv = Out((1,), dev), Out((70,), dev)
    gout = torch.ones(1).to(dev)
    st = lib.stream(x)
    vp, fp = ctypes.c_void_p * 65, ctypes.c_float * 65
    terms, ws = vp(*[x.data_ptr() + 4 * i for i in range(65)]), fp(*([1.0] * 65))
    holed = vp(*[x.data_ptr() if i != 1 else None for i in range(65)])
    f, b = G.msmc_scalar_wsum_fwd, G.msmc_scalar_wsum_bwd
    rcs = [f(terms, ws, 0, lib.ptr(out.t), st), f(terms, ws, 65, lib.ptr(out.t), st), f(terms, ws, -1, lib.ptr(out.t), st),
           f(holed, ws, 3, lib.ptr(out.t), st), f(None, ws, 3, lib.ptr(out.t), st), f(terms, None, 3, lib.ptr(out.t), st),
           f(terms, ws, 3, None, st), b(lib.ptr(gout), ws, 0, lib.ptr(gv.t), st), b(lib.ptr(gout), ws, 65, lib.ptr(gv.t), st),
           b(None, ws, 3, lib.ptr(gv.t), st), b(lib.ptr(gout), None, 3, lib.ptr(gv.t), st), b(lib.ptr(gout), ws, 3, None, st)]
    assert rcs == [E_SHAPE] * len(rcs), rcs
    assert all_nan(out.get(written=False)) and all_nan(gv.get(written=False)), 'a refused call wrote something'


def check_weighted_sum_function(dev):
    """hip/losses.py weighted_sum: a bf16 term, weights of 1.0, 65 terms (the stock chain), gradients by autograd"""
    from msmctts_amd.hip import losses
    gen = gen_for(950)
    for n, weights, bf in ((3, (0.5, -2.25, 1.0), 1), (4, None, None), (64, tuple(0.1 * (i - 30) for i in range(64)), 7), (65, tuple([0.5] * 65), None)):
        vals = torch.randn(n, generator=gen)
        ts = [vals[i].clone().to(torch.bfloat16 if i == bf else torch.float32).to(dev).requires_grad_(True) for i in range(n)]
        tot = losses.weighted_sum(ts, weights)
        assert tot.dtype == torch.float32 and tot.dim() == 0
        (tot * 1.5).backward()
        w = torch.tensor([1.0] * n if weights is None else [f32(x) for x in weights], dtype=torch.float64)
        x = torch.stack([t.detach().cpu().double() for t in ts])
        held('weighted_sum', 'n%d' % n, tot.detach().cpu().reshape(1), (w * x).sum().reshape(1), n * U * (w * x).abs().sum().reshape(1) * ONE)
        for i, t in enumerate(ts):
            want = (torch.tensor(1.5) * w[i].float()).to(t.dtype)
            assert t.grad is not None and t.grad.dtype == t.dtype and same_bits(t.grad.cpu().reshape(1), want.reshape(1)), (n, i)
