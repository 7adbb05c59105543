"""Shared cases of the kernels of csrc/optim.hip (opt_gradsq_kernel, opt_norm_kernel, opt_adamw_kernel) through the C entry
msmc_opt_clip_adamw with hand-built msmc_opt_tensor tables, and of three steps through the host layer
(trainers/optimizers/hip_adamw.py): tests/test_optim_emu.py runs them on the kernel interpreter, tests/test_gpu_optim.py on the
GPU.

Reference of every comparison: plain float64 torch on the CPU from the same fp32 input bits,
    norm = sqrt(sum g^2),  coef = min(1, max_norm / (norm + 1e-6)) (1 for max_norm <= 0),  g' = coef g,
    m' = b1 m + (1 - b1) g',  v' = b2 v + (1 - b2) g'^2,
    p' = p (1 - lr wd) - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps),  t = step + 1,
with every scalar that crosses the ABI as float (betas, eps, weight decay, lr, max_norm) and the 1e-6 of the clip rounded to fp32
first: 1 - b2^t at small t carries the rounding of b2 at about 1e-5 relative, a reference with double betas is another function.
check_reference_pins_torch (CPU only) holds this restated formula to 1e-12 relative against torch.optim.AdamW +
clip_grad_norm_ on float64 tensors with the same rounded hyperparameters over three steps, so it is not a restatement of the
kernel.  No reference restates chunks, lanes or alignment.  The per-element comparisons take coef as the fp32 value the kernel
wrote into norm_coef[1] (exact in float64); norm_coef itself is held against float64 on its own.

p, g, m, v of every tensor are views into four NaN-filled buffers (one per operand kind), each view at a chosen element offset
from a 16-byte boundary with at least GUARD NaN elements before it, behind it and between neighbours; partial, norm_coef and step
have GUARD NaN elements behind them and partial is NaN-filled.  Everything outside the views must keep its bits.  Every case runs
twice from fresh buffers and the two results agree bit for bit.

Bars (u = 2^-24; all times ONE2 = 1 + 2^-8, which covers the products of two relative errors left out of the first-order
bounds below: the test asserts that the largest relative term, the conditioning of 1 - b2^t, is below 2^-10).  The device build
may contract b m + (1 - b) g into an fma and the interpreter is built with -ffp-contract=off: an fma drops one rounding, so the
bars, counted without contraction, hold for both; no bit equality between the back-ends is asked for.
  sum g^2         D u relative (every term is positive).  A work-item of opt_gradsq_kernel folds 16 elements by fmaf (16 roundings:
                  the product is not rounded), the workgroup tree adds 8 steps, a work-item of opt_norm_kernel adds
                  ceil(nblocks / 256) partials, its tree 8 more: D = 16 + 8 + ceil(nblocks / 256) + 8.
  norm            sqrtf: (D / 2 + 1) u norm.      coef   the add of 1e-6 and the division: (D / 2 + 3) u coef; exactly 1 when clamped.
  exact-sum cases gradients that are multiples of 1/2 in [-2, 2]: g^2 is a multiple of 1/4, 16 n < 2^24 (checked in float64 in
                  the test), so every partial sum is exact in fp32 in any order and D = 0: norm within 1 u, coef within 3 u, and
                  the partials add up to sum g^2 exactly.  An omitted or doubled element moves sum g^2 by at least 1/4.
  clip boundary   max_norm = norm (1 -+ 1e-4): the float64 max_norm / (norm + 1e-6) differs from 1 by more than 8 x the bar of
                  coef on either side (asserted before the kernel runs), so the side the kernel takes is decided.
  g'              one product: u |g'|; bit-equal to g when coef == 1.  With max_norm <= 0 or write_grads = 0 the gradients keep
                  their bits; with max_norm <= 0 the NaN-filled partial keeps its bits too (with max_norm > 0 the norm is computed
                  and partial written whatever write_grads says).
  m'              E_m = (1 - b1) u |g'| + 2 u |(1 - b1) g'| + u |b1 m| + u (|b1 m| + |(1 - b1) g'|)
                  (g', fl(1 - b1), the two products, the addition)
  v'              c = (1 - b2) g'^2:  E_v = 5 u c + u b2 v + u (b2 v + c)      (g' twice, fl(1 - b2), two products; b2 v; the sum)
  step_size, rs2  r_ss = eps_pow b1^t / (1 - b1^t) + 2 u,   r_rs2 = (eps_pow b2^t / (1 - b2^t) + u) / 2 + 2 u: powf is within
                  eps_pow relative of b^t, the difference 1 - b^t magnifies that by b^t / (1 - b^t) (the conditioning term).
                  eps_pow is MEASURED ON THE REFERENCE, never on the kernel: the largest relative error of fp32 numpy.power
                  against float64 over the (beta, t) pairs the cases use, times 4 (the device's powf is another implementation of
                  a few ulp).  Measured 0.687 u (beta 0.8, t 2), so eps_pow = 2.75 u; eps_pow() computes it again on every run.
  p'              decay = 1 - lr wd: E_dc = u lr wd + u decay.   s = sqrt(v') rs2, d = s + eps, q = m' / d, ss = lr / (1 - b1^t):
                      E_sq = sqrt(v') (E_v / (2 v') + u)        (0 at v' = 0)
                      E_d  = rs2 E_sq + s (r_rs2 + u) + u d
                      E_q  = E_m / d + |q| E_d / d + u |q|
                      E_p  = |p| E_dc + u |p decay| + ss E_q + |ss q| (r_ss + u) + u (|p decay| + |ss q|)
                  p decay - ss q cancels, hence absolute terms throughout and no bar relative to |p'|.
  step            exactly t + 1, bit for bit.

Which case reaches which path:
  opt_find                tables of 1, 2, 3, 14 and 302 tensors (binary search nine levels deep); empty tensors (n = 0) first, in
                          the middle and last share a first_chunk with their neighbour and must never be chosen
  opt_norm_kernel         nblocks = 305 > 256: the second trip of the k += 256 loop (LONG); max_norm <= 0: no partial is read
  opt_gradsq_kernel       vector branch: whole chunk with g aligned (4096, 8192, the first chunks of 4097 and 8192 + 5, ALIGN with
                          g at offset 0); element branch: the tail chunks, every sub-chunk tensor, ALIGN with g at offset 1 and 2
  opt_adamw_kernel        chunk fast path: whole chunks with all four operands aligned; 4-wide fallback: the aligned part of a tail
                          chunk or sub-chunk tensor (1023: 255 vectors and 3 elements; 5: one vector and 1); scalar tail: the rest,
                          and every element of a tensor with an operand off a 16-byte boundary -- ALIGN: all aligned, each of p, g,
                          m, v alone one and two elements off, all four off (1, 2, 3, 1), each over 4096 (whole chunk), 8192 + 5
                          (chunks plus tail) and 1023 (sub-chunk)
  sizes                   1, 3, 4, 5, 1023, 4095, 4096, 4097, 8192, 8192 + 5 and 0 (SIZES)
  states                  STATES: t = 0 -> 1, 1 -> 2, 9 -> 10, 999 -> 1000, 200000 -> 200001; betas (0.8, 0.99), (0.9, 0.999),
                          (0, 0); weight decay 0, 0.01, 0.5 at lr 0.1; m = v = g = 0 (p' = p decay, no NaN); |g| in 1e-15 .. 1e-12
                          (eps dominates the denominator); |g| in 0.5e-8 .. 2e-8 at t = 1 (sqrt(v') rs2 within a factor 2 of eps);
                          |g| about 1e3 clipped and unclipped.  No intermediate is an fp32 denormal: g^2 (1 - b2) >= 1e-33.
  clip                    CLIPS: norm << max_norm (coef exactly 1), norm >> max_norm, the two boundary cases, a norm of 1e-3
                          (where the 1e-6 of the clip is 0.1 % of coef), max_norm = 0 and -1; write_grads 0 and 1 on each
  refusals                NULL table / partial / norm_coef / lr / step, ntensors <= 0, nblocks <= 0: MSMC_E_SHAPE, nothing written
  host layer              HipAdamW over parameters of 7, 165, 4096, 5000 and 27 elements (flat-state offsets 7, 172, 4268, 9268:
                          m / v of tensors 1 .. 4 off a 16-byte boundary), gradients that are views one element into a buffer.
Every comparison is appended to MEASURED and printed; the figures are recorded in profiles/loss_optim_direct.md.
"""
import ctypes
import math

import numpy as np
import torch

from _spectralcases import _nan, same_bits, twice
from _normcases import U, E_SHAPE, GUARD, L, gen_for
from _wnormcases import all_nan, dev_table
import _normcases

ONE2 = 1.0 + 2.0 ** -8
MEASURED = []
FLOOR_HELD = set()
BOOK = (MEASURED, FLOOR_HELD, 'optim')
CHUNK = 4096


def f32(x):
    return float(np.float32(x))


EPS_CLIP = f32(1e-6)
HP = dict(lr=1e-1, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
BETAS = ((0.8, 0.99), (0.9, 0.999), (0.0, 0.0))
STEPS = (1, 2, 3, 10, 1000, 200001)                  # every t = step + 1 a case runs (2, 3: the host layer's second and third step)


def held(what, case, got, ref, bound):
    _normcases.held(what, case, got, ref, bound, book=BOOK)


def eps_pow():
    """4 x the largest relative error of fp32 numpy.power against float64 over the tested (beta, t) pairs"""
    worst = 0.0
    for pair in BETAS:
        for b in pair:
            for t in STEPS:
                ref = f32(b) ** t
                if b == 0.0 or ref < 2.0 ** -120:
                    continue                       # 0^t is exact; b^t far below u leaves 1 - b^t == 1 whatever powf returns
                worst = max(worst, abs(float(np.power(np.float32(b), np.float32(t))) - ref) / ref)
    return 4.0 * worst


def hp_of(**kw):
    h = dict(HP)
    h.update(kw)
    return {k: f32(v) for k, v in h.items()}


# ---- the float64 reference and its bars -----------------------------------------------------------------------------------------------
def clip_ref(gs, max_norm):
    """-> sum g^2, norm, coef in float64 (python floats)"""
    ss = float(sum((g.double() ** 2).sum() for g in gs))
    norm = math.sqrt(ss)
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, f32(max_norm) / (norm + EPS_CLIP))
    return ss, norm, coef


def adamw_ref(p, g, m, v, t, hp, coef):
    """one step in float64 -> p', g', m', v'"""
    b1, b2 = hp['b1'], hp['b2']
    g1 = g * coef
    m1 = b1 * m + (1.0 - b1) * g1
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    ss = hp['lr'] / (1.0 - b1 ** t)
    d = v1.sqrt() / math.sqrt(1.0 - b2 ** t) + hp['eps']
    return p * (1.0 - hp['lr'] * hp['wd']) - ss * (m1 / d), g1, m1, v1


def adamw_bars(p, g, m, v, t, hp, coef, ep):
    """the bounds E_g, E_m, E_v, E_p of the module docstring, float64 tensors"""
    b1, b2, lr = hp['b1'], hp['b2'], hp['lr']
    p1, g1, m1, v1 = adamw_ref(p, g, m, v, t, hp, coef)
    a1, a2 = (b1 * m).abs(), ((1.0 - b1) * g1).abs()
    E_g = U * g1.abs()
    E_m = (1.0 - b1) * E_g + 2 * U * a2 + U * a1 + U * (a1 + a2)
    c = (1.0 - b2) * g1 * g1
    E_v = 5 * U * c + U * b2 * v + U * (b2 * v + c)
    p1t, p2t = b1 ** t, b2 ** t
    cond = max(ep * p1t / (1.0 - p1t), ep * p2t / (1.0 - p2t))
    assert cond < 2.0 ** -10, 'the conditioning of 1 - beta^t leaves the range ONE2 covers'
    r_ss = ep * p1t / (1.0 - p1t) + 2 * U
    r_rs2 = (ep * p2t / (1.0 - p2t) + U) / 2 + 2 * U
    rs2, ss, decay = 1.0 / math.sqrt(1.0 - p2t), lr / (1.0 - p1t), 1.0 - lr * hp['wd']
    sq = v1.sqrt()
    E_sq = torch.where(v1 > 0, sq * (E_v / (2 * v1.clamp_min(1e-300)) + U), torch.zeros_like(v1))
    s = sq * rs2
    d = s + hp['eps']
    E_d = rs2 * E_sq + s * (r_rs2 + U) + U * d
    q = m1 / d
    E_q = E_m / d + q.abs() * E_d / d + U * q.abs()
    E_dc = U * lr * hp['wd'] + U * decay
    pd, sq_ = (p * decay).abs(), (ss * q).abs()
    E_p = p.abs() * E_dc + U * pd + ss * E_q + sq_ * (r_ss + U) + U * (pd + sq_)
    return (p1, g1, m1, v1), (E_g * ONE2, E_m * ONE2, E_v * ONE2, E_p * ONE2)


def d_norm(nblocks):
    return 16 + 8 + (nblocks + 255) // 256 + 8


def check_reference_pins_torch():
    """CPU only: adamw_ref + clip_ref against torch.optim.AdamW + clip_grad_norm_ in float64, three steps, 1e-12 relative"""
    for (b1, b2), wd, mn in zip(BETAS, (0.0, 0.01, 0.5), (1.0, 30.0, 1e6)):
        hp = hp_of(b1=b1, b2=b2, wd=wd)
        gen = gen_for(100, int(b1 * 1000), int(wd * 100))
        ps = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in (5, 33, 1)]
        opt = torch.optim.AdamW(ps, lr=hp['lr'], betas=(hp['b1'], hp['b2']), eps=hp['eps'], weight_decay=hp['wd'])
        mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
        for t in (1, 2, 3):
            gs = [torch.randn(p.shape, generator=gen, dtype=torch.float64) * (3.0 if t != 2 else 0.1) for p in ps]
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            ss, norm, coef = clip_ref(gs, mn)
            tn = float(torch.nn.utils.clip_grad_norm_(ps, f32(mn)))
            assert abs(tn - norm) <= 1e-12 * norm
            opt.step()
            nxt = []
            for p, g, (p0, m0, v0) in zip(ps, gs, mine):
                p1, g1, m1, v1 = adamw_ref(p0, g, m0, v0, t, hp, coef)
                st = opt.state[p]
                assert float(st['step']) == t
                for a, b, scale in ((p1, p.detach(), p0.abs()), (g1, p.grad, g.abs()), (m1, st['exp_avg'], m1.abs()),
                                    (v1, st['exp_avg_sq'], v1.abs())):
                    assert bool(((a - b).abs() <= 1e-12 * scale).all()), (b1, wd, t)
                nxt.append((p1, m1, v1))
            mine = nxt


# ---- one call over a hand-built table ------------------------------------------------------------------------------------------------
def tensor(n, offs=(0, 0, 0, 0), g=None, p=None, m=None, v=None, key=0, exact=False, state=True):
    """one table entry: fp32 CPU tensors p, g, m, v of n elements and the element offsets of the four views"""
    gen = gen_for(200, n, key, *offs)
    d = dict(n=n, offs=offs)
    d['p'] = torch.randn(n, generator=gen) if p is None else p
    if g is None:
        g = (torch.randint(-4, 5, (n,), generator=gen).float() * 0.5) if exact else torch.randn(n, generator=gen)
    d['g'] = g
    d['m'] = (torch.randn(n, generator=gen) * 0.1 if state else torch.zeros(n)) if m is None else m
    d['v'] = (torch.rand(n, generator=gen) * 0.01 + 1e-4 if state else torch.zeros(n)) if v is None else v
    return d


def arena(vals, offs, dev):
    """the 1-D tensors ``vals`` in one NaN-filled buffer, view k starting offs[k] elements behind a 16-byte boundary, GUARD NaN
    elements (and the padding up to the boundary) before, between and behind -> the buffer on ``dev``, the start of each view"""
    pos, o = [], GUARD
    for val, off in zip(vals, offs):
        o = (o + 3) // 4 * 4 + off
        pos.append(o)
        o += val.numel() + GUARD
    buf = _nan((o,), 'cpu')
    for val, s in zip(vals, pos):
        buf[s:s + val.numel()] = val
    buf = buf.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, pos


def views_of(buf, pos, ns):
    """the views of a buffer that came back, and whether everything outside them still has its NaN bits"""
    rest = torch.ones(buf.numel(), dtype=torch.bool)
    out = []
    for s, n in zip(pos, ns):
        rest[s:s + n] = False
        out.append(buf[s:s + n].clone())
    return out, all_nan(buf[rest])


def opt_call(dev, T, hp, max_norm, write_grads, t0, expect=0, null=None, nt=None, nblocks=None):
    """msmc_opt_clip_adamw over the table ``T`` from fresh buffers, twice -> dict(p, g, m, v: lists; partial, norm_coef, step)"""
    lib = L()
    ns = [d['n'] for d in T]
    first, blk = [], 0
    for n in ns:
        first.append(blk)
        blk += (n + CHUNK - 1) // CHUNK
    nb = blk

    def run():
        bufs, poss = {}, {}
        for k, kind in enumerate('pgmv'):
            bufs[kind], poss[kind] = arena([d[kind] for d in T], [d['offs'][k] for d in T], dev)
        items = (lib.OptTensor * len(T))()
        for i, it in enumerate(items):
            it.p, it.g, it.m, it.v = (bufs[kind].data_ptr() + 4 * poss[kind][i] for kind in 'pgmv')
            it.n, it.first_chunk = ns[i], first[i]
        table = dev_table(items, dev)
        partial = _nan((max(nb, 1) + GUARD,), dev)
        nc = _nan((2 + GUARD,), dev)
        step = _nan((1 + GUARD,), 'cpu')
        step[0] = float(t0)
        step = step.to(dev)
        lr = torch.tensor([hp['lr']], dtype=torch.float32).to(dev)
        args = dict(table=lib.ptr(table), partial=lib.ptr(partial), norm_coef=lib.ptr(nc), lr=lib.ptr(lr), step=lib.ptr(step))
        if null:
            args[null] = None
        rc = lib.get().msmc_opt_clip_adamw(args['table'], len(T) if nt is None else nt, nb if nblocks is None else nblocks,
                                           float(max_norm), args['partial'], args['norm_coef'], args['lr'], args['step'], hp['b1'],
                                           hp['b2'], hp['eps'], hp['wd'], write_grads, lib.stream(partial))
        assert rc == expect, (rc, expect)
        if dev != 'cpu':
            torch.cuda.synchronize()
        res = []
        for kind in 'pgmv':
            vs, clean = views_of(bufs[kind].cpu(), poss[kind], ns)
            assert clean, 'an element of the %s buffer outside the tensors was written' % kind
            res += vs
        return tuple(res) + (partial.cpu(), nc.cpu(), step.cpu())

    got = twice(run)
    k = len(T)
    out = dict(p=got[0:k], g=got[k:2 * k], m=got[2 * k:3 * k], v=got[3 * k:4 * k], partial=got[4 * k], norm_coef=got[4 * k + 1],
               step=got[4 * k + 2], nblocks=nb)
    for name, n in (('partial', max(nb, 1)), ('norm_coef', 2), ('step', 1)):
        assert all_nan(out[name][n:]), 'a guard of %s was overwritten' % name
    return out


def compare(tag, T, got, hp, max_norm, write_grads, t0, exact=False, ep=None):
    ep = eps_pow() if ep is None else ep
    nb = got['nblocks']
    ss, norm, coef = clip_ref([d['g'] for d in T], max_norm)
    kn, kc = float(got['norm_coef'][0]), float(got['norm_coef'][1])
    assert same_bits(got['step'][:1], torch.tensor([float(t0 + 1)])), tag + ': step is not t + 1'
    if max_norm > 0:
        D = 0 if exact else d_norm(nb)
        if exact:
            assert 16 * sum(d['n'] for d in T) < 2 ** 24 and all(bool((d['g'].double() * 2 == (d['g'].double() * 2).round()).all())
                                                                 and float(d['g'].abs().max() if d['n'] else 0) <= 2 for d in T)
            assert float(got['partial'][:nb].double().sum()) == ss, tag + ': the partials do not add up to the exact sum g^2'
        assert not bool(torch.isnan(got['partial'][:nb]).any()), tag + ': a partial was not written'
        held('norm', tag, got['norm_coef'][0:1], torch.tensor([norm], dtype=torch.float64),
             torch.tensor([(D / 2.0 + 1) * U * norm * ONE2], dtype=torch.float64))
        if f32(max_norm) / (norm + EPS_CLIP) >= 1.0 + 8 * (D / 2.0 + 3) * U:
            assert kc == 1.0, tag + ': coef is not clamped to exactly 1'
        held('coef', tag, got['norm_coef'][1:2], torch.tensor([coef], dtype=torch.float64),
             torch.tensor([(D / 2.0 + 3) * U * coef * ONE2], dtype=torch.float64))
    else:
        assert same_bits(got['norm_coef'][:2], torch.tensor([0.0, 1.0])), tag + ': norm_coef is not (+0, 1) without a clip'
        assert all_nan(got['partial']), tag + ': partial was written without a clip'
    if not (max_norm > 0 and write_grads):
        for d, g in zip(T, got['g']):
            assert same_bits(g, d['g']), tag + ': a gradient changed although nothing asked for it'
    ok = [d for d in T if d['n']]
    cat = lambda xs: torch.cat([x.double() for x in xs]) if xs else torch.zeros(0, dtype=torch.float64)
    sel = lambda kind: cat([x for x, d in zip(got[kind], T) if d['n']])
    (p1, g1, m1, v1), (E_g, E_m, E_v, E_p) = adamw_bars(cat([d['p'] for d in ok]), cat([d['g'] for d in ok]), cat([d['m'] for d in ok]),
                                                         cat([d['v'] for d in ok]), t0 + 1, hp, kc, ep)
    if max_norm > 0 and write_grads:
        if kc == 1.0:
            for d, g in zip(T, got['g']):
                assert same_bits(g, d['g']), tag + ': coef == 1 and a gradient changed bits'
        held('g', tag, sel('g'), g1, E_g)
    held('m', tag, sel('m'), m1, E_m)
    held('v', tag, sel('v'), v1, E_v)
    held('p', tag, sel('p'), p1, E_p)
    return kc


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 3, 4, 5, 1023, 0, 4095, 4096, 4097, 8192, 8192 + 5, 0, 0)
ALIGN = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2),
         (1, 2, 3, 1))
ALIGN_SIZES = (4096, 8192 + 5, 1023)


def check_sizes(dev, which):
    """'all': the table of every size with the empty tensors; 'one', 'two': tables of 1 and 2 tensors.  Exact-sum gradients"""
    ns = {'all': SIZES, 'one': (5,), 'two': (4097, 3), 'empty': (0, 7)}[which]
    T = [tensor(n, key=i, exact=True) for i, n in enumerate(ns)]
    hp = hp_of()
    for max_norm in (1.0, 0.0):
        got = opt_call(dev, T, hp, max_norm, 1, 4)
        compare('sizes %s mn%g' % (which, max_norm), T, got, hp, max_norm, 1, 4, exact=True)


def check_long_table(dev):
    """300 tensors of 1 .. 7 elements and two multi-chunk ones: nblocks = 305"""
    ns = [1 + i % 7 for i in range(150)] + [4097] + [1 + (i * 3) % 7 for i in range(150)] + [8192 + 5]
    assert len(ns) == 302 and sum(ns) < 30000
    hp = hp_of(b1=0.8, b2=0.99)
    for exact in (True, False):
        T = [tensor(n, offs=(i % 4, (i // 4) % 4, (i // 16) % 4, (i // 64) % 4), key=i, exact=exact) for i, n in enumerate(ns)]
        got = opt_call(dev, T, hp, 2.0, 1, 1)
        assert got['nblocks'] == 305
        compare('long exact%d' % exact, T, got, hp, 2.0, 1, 1, exact=exact)


def check_alignment(dev, offs):
    T = [tensor(n, offs=offs, key=i, exact=True) for i, n in enumerate(ALIGN_SIZES)]
    hp = hp_of()
    got = opt_call(dev, T, hp, 1.0, 1, 9)
    compare('align %s' % (offs,), T, got, hp, 1.0, 1, 9, exact=True)
    T = [tensor(n, offs=offs, key=i + 10) for i, n in enumerate(ALIGN_SIZES)]
    got = opt_call(dev, T, hp, 1.0, 1, 0)
    compare('align %s random' % (offs,), T, got, hp, 1.0, 1, 0)


STATE_SIZES = (4096 + 5, 1023, 3)
# name -> (t0, betas, wd, eps, gradient scale | (lo, hi) of log-uniform |g|, state given, max_norm)
STATES = {
    't0 b.9 wd.01': (0, BETAS[1], 0.01, 1e-8, 1.0, False, 1.0),
    't1 b.8 wd0': (1, BETAS[0], 0.0, 1e-8, 1.0, True, 1.0),
    't9 b.9 wd.5': (9, BETAS[1], 0.5, 1e-8, 1.0, True, 0.0),
    't999 b.8 wd.01': (999, BETAS[0], 0.01, 1e-8, 0.01, True, 1.0),
    't200000 b.9 wd0': (200000, BETAS[1], 0.0, 1e-8, 1.0, True, 1.0),
    't9 b0 wd.01': (9, BETAS[2], 0.01, 1e-8, 1.0, True, 1.0),
    't0 b0 wd.5': (0, BETAS[2], 0.5, 1e-8, 1.0, False, 0.0),
    'zero t0 b.9': (0, BETAS[1], 0.01, 1e-8, 0.0, False, 1.0),
    'zero t0 b0': (0, BETAS[2], 0.5, 1e-8, 0.0, False, 0.0),
    'tiny t0 b.9': (0, BETAS[1], 0.01, 1e-8, (1e-15, 1e-12), False, 1.0),
    'tiny t1 b.8': (1, BETAS[0], 0.0, 1e-8, (1e-15, 1e-12), False, 1.0),
    'near eps t0 b.9': (0, BETAS[1], 0.01, 1e-8, (0.5e-8, 2e-8), False, 1.0),
    'near eps t0 b.8': (0, BETAS[0], 0.0, 1e-8, (0.5e-8, 2e-8), False, 0.0),
    'near eps 1e-3 t1 b.8': (1, BETAS[0], 0.0, 1e-3, (0.5e-3, 2e-3), False, 0.0),
    'large clipped': (9, BETAS[1], 0.01, 1e-8, 1e3, True, 1.0),
    'large unclipped': (1, BETAS[0], 0.01, 1e-8, 1e3, True, 0.0),
}


def check_state(dev, name):
    t0, (b1, b2), wd, eps, scale, state, max_norm = STATES[name]
    assert t0 + 1 in STEPS
    hp = hp_of(b1=b1, b2=b2, wd=wd, eps=eps)
    T = []
    for i, n in enumerate(STATE_SIZES):
        gen = gen_for(300, i, t0, int(b1 * 10))
        if isinstance(scale, tuple):
            lo, hi = math.log(scale[0]), math.log(scale[1])
            g = torch.exp(torch.rand(n, generator=gen) * (hi - lo) + lo) * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
        else:
            g = torch.randn(n, generator=gen) * scale
        T.append(tensor(n, g=g, key=i, state=state))
    got = opt_call(dev, T, hp, max_norm, 1, t0)
    compare('state ' + name, T, got, hp, max_norm, 1, t0)
    for kind in 'pmv':
        for x in got[kind]:
            assert bool(torch.isfinite(x).all())
    if scale == 0.0:
        for d, p in zip(T, got['p']):                                     # p' = fl(p fl(1 - fl(lr wd))): p decay - ss 0 / eps
            held('p == p decay', 'state ' + name, p, d['p'].double() * (1.0 - hp['lr'] * hp['wd']),
                 (2 * U * (1.0 - hp['lr'] * hp['wd']) + U * hp['lr'] * hp['wd']) * d['p'].double().abs() * ONE2)
            assert same_bits(p, d['p'] * (torch.tensor(1.0) - torch.tensor(hp['lr']) * torch.tensor(hp['wd'])))
        for kind in 'mv':
            for x in got[kind]:
                assert same_bits(x, torch.zeros_like(x)), 'm, v of a zero gradient on a zero state are not +0'


CLIP_SIZES = (4096, 4097 + 1023, 5)
CLIPS = ('far below', 'far above', 'just below', 'just above', 'small norm', 'zero', 'negative')


def check_clip(dev, name, write_grads):
    scale = 1e-5 if name == 'small norm' else 1.0
    T = [tensor(n, key=i + 40, g=torch.randn(n, generator=gen_for(400, i)) * scale) for i, n in enumerate(CLIP_SIZES)]
    ss, norm, _ = clip_ref([d['g'] for d in T], 1.0)
    max_norm = {'far below': 1e6, 'far above': 1e-2, 'just below': f32(norm * (1 + 1e-4)), 'just above': f32(norm * (1 - 1e-4)),
                'small norm': f32(norm / 2), 'zero': 0.0, 'negative': -1.0}[name]
    hp = hp_of(b1=0.8, b2=0.99)
    bar = (d_norm(3) / 2.0 + 3) * U
    if name.startswith('just'):
        ratio = max_norm / (norm + EPS_CLIP)
        assert abs(ratio - 1.0) > 8 * bar and (ratio > 1) == (name == 'just below'), 'the boundary case is not decided in float64'
    if name == 'small norm':
        assert EPS_CLIP / norm > 8 * bar, 'the 1e-6 of the clip does not show against the bar'
    got = opt_call(dev, T, hp, max_norm, write_grads, 9)
    kc = compare('clip %s wg%d' % (name, write_grads), T, got, hp, max_norm, write_grads, 9)
    if name in ('far below', 'just below', 'zero', 'negative'):
        assert kc == 1.0
    else:
        assert kc < 1.0


def check_refusals(dev):
    T = [tensor(5), tensor(4097, key=1)]
    hp = hp_of()
    for kw in (dict(null='table'), dict(null='partial'), dict(null='norm_coef'), dict(null='lr'), dict(null='step'), dict(nt=0),
               dict(nt=-1), dict(nblocks=0), dict(nblocks=-3)):
        got = opt_call(dev, T, hp, 1.0, 1, 3, expect=E_SHAPE, **kw)
        for kind in 'pgmv':
            for d, x in zip(T, got[kind]):
                assert same_bits(x, d[kind]), 'a refused call wrote %s (%s)' % (kind, kw)
        assert all_nan(got['partial']) and all_nan(got['norm_coef']) and float(got['step'][0]) == 3.0, 'a refused call wrote (%s)' % kw


HOST_SHAPES = ((7,), (33, 5), (4096,), (5000,), (3, 3, 3))


def check_host_layer(dev):
    """three steps of HipAdamW with gradients that are views one element into a buffer; every step against the float64 chain
    re-seeded from the kernel's own previous state"""
    from msmctts_amd.trainers.optimizers.hip_adamw import HipAdamW
    hp = hp_of(lr=1e-1, b1=0.8, b2=0.99, wd=0.01)
    gen = gen_for(500)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(dev)) for s in HOST_SHAPES]
    opt = HipAdamW(ps, lr=hp['lr'], betas=(hp['b1'], hp['b2']), eps=hp['eps'], weight_decay=hp['wd'])
    ep = eps_pow()
    nb = sum((p.numel() + CHUNK - 1) // CHUNK for p in ps)
    for t in (1, 2, 3):
        base = (torch.randn(1 + sum(p.numel() for p in ps), generator=gen) * (3.0 if t != 2 else 0.01)).to(dev)
        off, gs = 1, []
        for p in ps:
            p.grad = base[off:off + p.numel()].view_as(p)
            assert p.grad.data_ptr() == base.data_ptr() + 4 * off
            gs.append(p.grad.detach().cpu().clone().reshape(-1))
            off += p.numel()
        assert ps[0].grad.data_ptr() % 16 == 4
        if t == 1:
            before = [(p.detach().cpu().clone().reshape(-1), torch.zeros(p.numel()), torch.zeros(p.numel())) for p in ps]
        else:
            before = [(p.detach().cpu().clone().reshape(-1), opt.state[p]['exp_avg'].cpu().clone().reshape(-1),
                       opt.state[p]['exp_avg_sq'].cpu().clone().reshape(-1)) for p in ps]
        opt.step(max_norm=1.0)
        flat = opt.param_groups[0]['flat']
        if t == 1:
            assert any(opt.state[p]['exp_avg'].data_ptr() % 16 for p in ps) and any(opt.state[p]['exp_avg_sq'].data_ptr() % 16 for p in ps)
        T = [dict(n=g.numel(), p=b[0], g=g, m=b[1], v=b[2]) for g, b in zip(gs, before)]
        got = dict(p=[p.detach().cpu().reshape(-1) for p in ps], g=[p.grad.detach().cpu().reshape(-1) for p in ps],
                   m=[opt.state[p]['exp_avg'].cpu().reshape(-1) for p in ps], v=[opt.state[p]['exp_avg_sq'].cpu().reshape(-1) for p in ps],
                   partial=torch.zeros(nb), norm_coef=flat['norm_coef'].cpu(), step=flat['step'].cpu(), nblocks=nb)
        compare('host step %d' % t, T, got, hp, 1.0, 1, t - 1, ep=ep)
        assert float(opt.grad_norm) == float(flat['norm_coef'][0])
        for p in ps:
            assert same_bits(opt.state[p]['step'].cpu().reshape(1), torch.tensor([float(t)]))
