"""Shared cases of the LayerNorm, gate and glue kernels (csrc/norm.hip without its BatchNorm half: msmc_add_ln_fwd / _bwd,
msmc_add_ln_param_multi, msmc_fc_add_ln_fwd, the gate / tanh family, msmc_sum_n, msmc_dropout_add_fwd / msmc_dropout_bwd,
msmc_row_mask, msmc_fft_prologue) through the C entries, and of one pass through hip/norm.py: tests/test_norm_emu.py runs them on
the kernel interpreter, tests/test_gpu_norm.py on the GPU.

Reference of every comparison: stock torch operators on the CPU in float64 (F.layer_norm, var_mean, tanh, sigmoid, +, F.embedding,
matmul) from the same fp32 / bf16 input bits, and their autograd gradients.  No reference restates a kernel's lane or index
arithmetic.  Every output is pre-filled with NaN and none may remain in the part the entry owns; every output carries GUARD
elements behind its end which must keep their NaN bits; every case runs twice and the two results must agree bit for bit.

Bars (u = 2^-24, the build uses -ffp-contract=off; h(r) = half a bf16 ulp of the float64 reference r, added wherever the output
is bf16):
  copies, masks   bit equality: row_mask, keep_row, key_bias, v without dropout and residual, dropped elements == +0, sum_n and
                  dropout_add (p = 0) against the one correctly rounded fp32 sum (in the documented order ((a + b) + c) + d).
                  Dead rows of y are +0 bit for bit.  Dead rows of gx / gres are held to == 0 only, a zero of either sign, which
                  is less than the bit equality with +0 asked of them: the backward kernel forms 0 * gamma, -0 for a negative
                  gamma, and carries that sign through to rstd * (-0) (numerically harmless; profiles/norm_direct.md).
  sum_n           also against float64: (k - 1) u sum |operand| for k operands (k - 1 additions, each within u of its result).
  dropout         a kept element is x * fl(1 / (1 - p)): two roundings of the scale (1 - p, the quotient), one of the product:
                  3 u |ref|; with a residual one more addition: 3 u |x| / (1 - p) + u |ref|.
  tanh_bwd        g (1 - y y): the product y y (u y^2), the difference (u |1 - y^2|), the product with g (u): |g| (u y^2 +
                  2 u |1 - y^2|) (1 + 2^-20); exactly 0 at y = +-1.
  prologue        one fp32 addition: u |ref|; fp32 -> fp32 bit-equal to torch's fp32 sum.
  tanh, gate      tanhf / expf are library code: the yardstick rule below against torch's own fp32 tanh / sigmoid (and their fp32
                  autograd) on the CPU.
  LayerNorm       the project's yardstick rule (tests/_attn32cases.py, tests/_spectralcases.py), per quantity (y, mean, rstd; gx,
                  gres, dgamma, dbeta), in the max norm and in the L2 norm: the error against float64 is at most RATIO = 4 x the
                  error of the same chain written with elementary torch operators in fp32 on the CPU (mean, subtract, square, mean,
                  + eps, rsqrt, multiply, add; gradients by fp32 autograd).  The factor is for another order of the sums.
  ... or a floor  torch's chain can be exact by luck where the kernel is not (rows of 1 .. 6 channels, a constant row, an integer
                  mean): 4 x 0 is no bar.  A comparison that misses 4 x passes only if EVERY element lies inside the rounding-count
                  bound below; MEASURED records which of the two held.  D = 48 bounds the additions one sum passes through in any
                  of the kernels (at most 40 in a lane of the fused kernel, 16 in the others, 6 butterfly steps or 2 + 3 through
                  LDS, the quotient by C).  Per row, with e_v the bound on what the kernel's fp32 v differs from the float64 v by
                  (2 u |v|: the scale and the residual addition), a1 = mean |v|, d = v - mean, r = rstd:
                      mean    dm = D u a1 + mean(e_v)
                      d       ed = dm + e_v + u |d|
                      var     dvar = (D + 6) u var + 2 mean(|d| e_v) + mean(ed^2)       (sum d = 0 cancels dm to first order)
                      rstd    B_r = the larger distance of r to 1 / sqrt(var + eps -+ dvar), plus 4 u r (+ eps, sqrtf, the quotient)
                      y       |gamma| (ed (r + B_r) + |d| B_r) + 4 u (|d r gamma| + |beta|)
                  Backward, from mean and rstd rounded to fp32 (u |mean|, u r), xh = d r, dxh = gy gamma, m1 = mean(dxh),
                  m2 = mean(dxh xh):
                      xh      e_x = 3 u |xh| + u |mean| r
                      m1, m2  E1 = (D + 2) u mean |dxh|,  E2 = (D + 2) u mean |dxh xh| + mean(|dxh| e_x)
                      dv      r (u |dxh| + E1 + e_x |m2| + (|xh| + e_x) E2) + 4 u r (|dxh| + |m1| + |xh m2|)
                      dgamma  sum_rows |gy| e_x + DP u sum_rows |gy xh|,   dbeta  DP u sum_rows |gy|
                  DP = 32: at most 4 rows in a wave, 3 additions between the waves, ceil(blocks / 16) <= 9 per slice, 16 slices.
  fc + LayerNorm  v bit-equal to bf16(bf16(h) + res), h = a W^T + bias in float64, but for elements where h - E and
                  h + E round to different bf16 values, E = K u sum_k |a_k W_k| + u |h| the fp32 accumulation error: those may
                  differ by one bf16 ulp and are at most 1 % of a case (asserted on the reference alone).  bf16(h) + res is a sum
                  of two bf16 values, exact in fp32 as in float64: its own rounding, ties included, leaves nothing out.  y against the
                  float64 LayerNorm of the RETURNED v: the kernel normalises its unrounded fp32 v, which lies within h(v) of the
                  returned one, so the yardstick (a chain that starts from the returned v) does not apply; the floor above with
                  e_v = h(v) + 2 u |v| is the bar.  mean / rstd against the statistics of the unrounded float64 sum, floor with
                  e_v = one bf16 ulp of h at the elements named above, 2 u |v| elsewhere.
Dropout: every kernel's mask is compared with the one msmc_dropout_add_fwd draws for the same (seed word, salt, element index) on
a tensor of ones.  A first element index beyond 2^32 would need a 16 GB tensor and is left out.

Which case reaches which instantiation:
  add_ln_fwd <V=4>        A: C = 4, 252, 256, 260, 512, 768, 1024 (C = 1024: all four lane groups), C dropout (9, 256)
  add_ln_fwd <V=1>        A: C = 1, 6, 67, 1023 (16 groups, the last short); C dropout (9, 67); every misaligned case
  add_ln_bwd <V=4, NG=1>  B: C = 4, 8, 256     NG=2: C = 260     NG=3: C = 516, 768     NG=4: C = 772, 1024
  add_ln_bwd <V=1, NG=16> B: C = 67, 1023; every misaligned case
  fc_add_ln <4,4>: K = 128, 256   <4,2>: (5, 256, 64)   <4,1>: K = 32 at C <= 256   <10,2>: (18, 384, 64), (2, 640, 64)
  <10,1>: (3, 260, 32)
  fft_prologue            G: C = 24, 260 (V=4) and C = 1, 6, 67 (V=1), each with all four dtype pairs
each in fp32 and in bf16 (the fused kernel is bf16 only).  Every comparison is appended to MEASURED and printed; the figures are
recorded in profiles/norm_direct.md.
"""
import ctypes
import math

import torch
import torch.nn.functional as F_

from _spectralcases import _bits, _nan, same_bits, twice

U = 2.0 ** -24
E_SHAPE, E_WORKSPACE = -2, -3
RATIO = 4.0
D_SUM, D_PARAM = 48, 32
GUARD = 8
LN_PARAM_MAX = 32
MEASURED = []          # (what, case, figure, how it was held)
# the comparisons that may miss 4 x and be held by the rounding-count floor, each shown right in profiles/norm_direct.md: torch's
# fp32 rstd of these five rows happens to lie within 0.4 ulp of the float64 one, the kernel's at 5 % of the floor.  Any other
# comparison may use the floor only where the yardstick is no bar at all (torch's chain is exact: its error is 0)
FLOOR_HELD = {('ln fwd rstd', '5x256 fp32'), ('ln fwd rstd', '5x256 fp32 keep')}
DTYPES = ((0, torch.float32, 'fp32'), (1, torch.bfloat16, 'bf16'))


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def held(what, case, got, ref, bound, book=None):
    """|got - ref| <= bound element by element (a NaN in ``got`` fails); records the largest share of the bound used.  ``book``:
    another module's (MEASURED, FLOOR_HELD, print prefix) in place of this one's"""
    measured, _, prefix = book or (MEASURED, FLOOR_HELD, 'norm')
    got, err = got.double(), (got.double() - ref).abs()
    assert not bool(torch.isnan(got).any()), '%s %s: an element was not written' % (what, case)
    bound = bound.expand_as(err)
    pos = bound > 0
    used = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    measured.append((what, case, used, 'bound'))
    print('%s %-26s %-34s share of the bound used %.3f' % (prefix, what, case, used))
    bad = ~(err <= bound)
    assert not bool(bad.any()), '%s %s: %d elements outside the bound, worst err %.3e at bound %.3e' % (
        what, case, int(bad.sum()), float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def half_ulp(ref, dtype):
    """half a bf16 ulp of every element of the float64 ``ref`` (0 for fp32 outputs and at an exact 0)"""
    if dtype != torch.bfloat16:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref)                                              # ref = f 2^e, f in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def yard(what, case, got, t32, ref, floor=None, half=None, book=None):
    """the yardstick rule in both norms, ``half`` (the bf16 half-ulp of the output) added to the bar; a comparison that misses it
    passes only if it is listed in FLOOR_HELD (or torch's chain is exact) and every element lies inside ``floor + half`` (the
    module docstring).  ``book``: as for ``held``"""
    measured, floor_held, prefix = book or (MEASURED, FLOOR_HELD, 'norm')
    got, ref = got.double(), ref.double()
    assert not bool(torch.isnan(got).any()), '%s %s: an element was not written' % (what, case)
    half = torch.zeros_like(ref) if half is None else half
    err, e32 = (got - ref).abs(), (t32.double() - ref).abs()
    worst, ok = 0.0, True
    for f in (lambda d: float(d.max()) if d.numel() else 0.0, lambda d: float(d.norm())):
        ek, bar = f(err), RATIO * f(e32) + f(half)
        ok = ok and ek <= bar
        worst = max(worst, (ek / bar * RATIO) if bar > 0 else (0.0 if ek == 0 else float('inf')))
    how = 'yardstick'
    if not ok:
        assert floor is not None, '%s %s: %.2f x the fp32 chain and no derived bound' % (what, case, worst)
        assert (what, case) in floor_held or float(e32.max()) == 0.0, \
            '%s %s: %.2f x the fp32 chain, and the case is not one of those held by the derived bound' % (what, case, worst)
        bound = floor.expand_as(err) + half
        inside = err <= bound
        used = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
        how = 'floor %.3f' % used
        assert bool(inside.all()), '%s %s: %.2f x the fp32 chain and %d elements outside the derived bound (share %.2f)' % (
            what, case, worst, int((~inside).sum()), used)
    measured.append((what, case, worst, how))
    print('%s %-26s %-34s %7.2f x torch fp32 of %.0f allowed  (%s)' % (prefix, what, case, worst, RATIO, how))


class Out(object):
    """an output of ``shape`` that starts ``off`` elements into a NaN-filled buffer and has GUARD elements behind it"""

    def __init__(self, shape, dev, dtype=torch.float32, off=0):
        self.shape, self.off, self.n = tuple(shape), off, int(math.prod(shape))
        self.buf = _nan((off + self.n + GUARD,), dev, dtype)
        self.t = self.buf[off:off + max(self.n, 1)]          # (an empty tensor has no pointer: N = 0 still passes one)

    def get(self, written=True):
        b = self.buf.cpu()
        fresh = _nan(b.shape, 'cpu', b.dtype)
        assert same_bits(b[:self.off], fresh[:self.off]) and same_bits(b[self.off + self.n:], fresh[self.off + self.n:]), \
            'a guard element was overwritten'
        r = b[self.off:self.off + self.n].clone().view(self.shape)
        if written:
            assert not bool(torch.isnan(r.float()).any()), 'an element was not written'
        return r


def at(t, dev, off=0):
    """``t`` on ``dev``, contiguous, starting ``off`` elements into a larger buffer"""
    if t is None:
        return None
    buf = torch.zeros(off + t.numel() + GUARD, dtype=t.dtype)
    buf[off:off + t.numel()] = t.reshape(-1)
    return buf.to(dev)[off:off + max(t.numel(), 1)]


def L():
    from msmctts_amd.hip import lib
    return lib


def gen_for(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def keep_rows(N, block=4):
    """a dead first row, a dead last row and, where N allows, a fully dead workgroup (rows block .. 2 block - 1)"""
    k = torch.ones(N, dtype=torch.uint8)
    if N:
        k[0] = 0
        k[N - 1] = 0
    if N > 2 * block:
        k[block:2 * block] = 0
    return k


# ---- the mask source -----------------------------------------------------------------------------------------------------------------
def seed_tensor(dev, word):
    return None if word is None else torch.tensor([word], dtype=torch.int64).to(dev)


def drop_mask(dev, word, salt, n, p, which=0):
    """the keep mask of elements 0 .. n - 1 for (seed word, salt): msmc_dropout_add_fwd on ones, without a residual.  A kept element
    must be the fp32 1 / (1 - p) exactly (scaled once), a dropped one +0"""
    lib = L()
    code, dtype, _ = DTYPES[which]
    n4 = (n + 3) // 4 * 4
    ones = torch.ones(n4, dtype=dtype).to(dev)
    seed = seed_tensor(dev, word)
    y = Out((n4,), dev, dtype)
    lib.call('msmc_dropout_add_fwd', lib.ptr(ones), None, lib.ptr(y.t), n4, p, lib.ptr(seed), salt, code, lib.stream(ones))
    y = y.get()
    m = y != 0
    scale = (torch.ones(1) / (torch.ones(1) - torch.tensor([p]))).to(dtype)               # fp32 1 / (1 - p), rounded to the dtype
    assert bool((_bits(y[m]) == _bits(scale)).all()), 'a kept 1 is not 1 / (1 - p)'
    assert bool((_bits(y[~m]) == 0).all()), 'a dropped element is not +0'
    return m[:n]


# ---- A / B: LayerNorm references and floors --------------------------------------------------------------------------------------------
def ln_ref(v64, gamma, beta, keep, eps):
    C = v64.shape[-1]
    y = F_.layer_norm(v64, (C,), gamma.double(), beta.double(), eps)
    if keep is not None:
        y = y * keep.double()[:, None]
    var, mean = torch.var_mean(v64, -1, unbiased=False)
    return y, mean, 1.0 / torch.sqrt(var + eps)


def ln_chain(v, gamma, beta, keep, eps):
    """the same chain with elementary operators in the dtype of ``v`` -> y, mean, rstd"""
    m = v.mean(-1, keepdim=True)
    d = v - m
    r = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    y = d * r * gamma.to(v.dtype) + beta.to(v.dtype)
    if keep is not None:
        y = y * keep.to(v.dtype)[:, None]
    return y, m.squeeze(-1), r.squeeze(-1)


def ln_floor_fwd(v64, gamma, beta, eps, e_v=None):
    """the rounding-count bounds of mean, rstd, y (module docstring)"""
    g, b = gamma.double().abs(), beta.double().abs()
    e_v = 2 * U * v64.abs() if e_v is None else e_v
    var, mean = torch.var_mean(v64, -1, unbiased=False, keepdim=True)
    d, r = (v64 - mean).abs(), 1.0 / torch.sqrt(var + eps)
    dm = D_SUM * U * v64.abs().mean(-1, keepdim=True) + e_v.mean(-1, keepdim=True)
    ed = dm + e_v + U * d
    dvar = (D_SUM + 6) * U * var + 2 * (d * e_v).mean(-1, keepdim=True) + (ed * ed).mean(-1, keepdim=True)
    lo = 1.0 / torch.sqrt(var + eps + dvar)
    hi = 1.0 / torch.sqrt(torch.clamp(var + eps - dvar, min=1e-300))
    b_r = torch.maximum(r - lo, hi - r) + 4 * U * r
    b_y = g * (ed * (r + b_r) + d * b_r) + 4 * U * (d * r * g + b)
    return dm.squeeze(-1), b_r.squeeze(-1), b_y


def ln_bwd_ref(g, v, gamma, keep, eps, dtype):
    """gradients of layer_norm(v) * keep for the output gradient g in ``dtype`` (float64: the reference, float32: the yardstick,
    there with the elementary chain) -> dv, dgamma, dbeta"""
    v_ = v.detach().clone().to(dtype).requires_grad_(True)
    ga = gamma.detach().clone().to(dtype).requires_grad_(True)
    be = torch.zeros_like(ga).requires_grad_(True)
    C = v.shape[-1]
    if dtype == torch.float64:
        y = F_.layer_norm(v_, (C,), ga, be, eps)
        if keep is not None:
            y = y * keep.double()[:, None]
    else:
        y, _, _ = ln_chain(v_, ga, be, keep, eps)
    y.backward(g.to(dtype))
    return v_.grad, ga.grad, be.grad


def ln_floor_bwd(g, v, gamma, keep, eps):
    g64, v64, ga = g.double(), v.double(), gamma.double().abs()
    if keep is not None:
        g64 = g64 * keep.double()[:, None]
    var, mean = torch.var_mean(v64, -1, unbiased=False, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xh, gy = ((v64 - mean) * r), g64.abs()
    dxh = gy * ga
    m1 = (g64 * gamma.double()).mean(-1, keepdim=True).abs()
    m2 = (g64 * gamma.double() * xh).mean(-1, keepdim=True).abs()
    xh = xh.abs()
    e_x = 3 * U * xh + U * mean.abs() * r
    e1 = (D_SUM + 2) * U * dxh.mean(-1, keepdim=True)
    e2 = (D_SUM + 2) * U * (dxh * xh).mean(-1, keepdim=True) + (dxh * e_x).mean(-1, keepdim=True)
    b_dv = r * (U * dxh + e1 + e_x * m2 + (xh + e_x) * e2) + 4 * U * r * (dxh + m1 + xh * m2)
    b_dg = (gy * e_x).sum(0) + D_PARAM * U * (gy * xh).sum(0)
    b_db = D_PARAM * U * gy.sum(0)
    return b_dv, b_dg, b_db


# ---- A: msmc_add_ln_fwd ----------------------------------------------------------------------------------------------------------------
LN_FWD_SHAPES = ((1, 1), (3, 4), (5, 6), (4, 252), (5, 256), (6, 260), (3, 67), (7, 1023), (2, 1024), (9, 768), (17, 512), (0, 8))


def ln_fwd(dev, x, res, gamma, beta, keep, eps, p=0.0, word=None, salt=0, off=()):
    """-> y, v, mean, rstd on the CPU; ``off``: names of the operands that start one element into a larger buffer"""
    lib = L()
    N, C = x.shape
    code = 0 if x.dtype == torch.float32 else 1
    o = lambda name: 1 if name in off else 0
    xd, rd = at(x, dev, o('x')), at(res, dev, o('res'))
    gd, bd = at(gamma, dev, o('gamma')), at(beta, dev, o('beta'))
    kd, seed = at(keep, dev), seed_tensor(dev, word)

    def run():
        y, v = Out((N, C), dev, x.dtype, o('y')), Out((N, C), dev, x.dtype, o('v'))
        mean, rstd = Out((N,), dev), Out((N,), dev)
        lib.call('msmc_add_ln_fwd', lib.ptr(xd), lib.ptr(rd), lib.ptr(gd), lib.ptr(bd), lib.ptr(kd), lib.ptr(y.t), lib.ptr(v.t),
                 lib.ptr(mean.t), lib.ptr(rstd.t), N, C, eps, p, lib.ptr(seed), salt, code, lib.stream(gd))
        return y.get(), v.get(), mean.get(), rstd.get()

    return twice(run)


def ln_inputs(N, C, dtype, key):
    gen = gen_for(2000, N, C, key)
    x = torch.randn(N, C, generator=gen).to(dtype)
    res = torch.randn(N, C, generator=gen).to(dtype)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=gen)
    beta = 0.5 * torch.randn(C, generator=gen)
    return x, res, gamma, beta


def compare_ln_fwd(tag, got, v64, v32, gamma, beta, keep, eps, dtype, e_v=None):
    y, _, mean, rstd = got
    ref_y, ref_m, ref_r = ln_ref(v64, gamma, beta, keep, eps)
    t_y, t_m, t_r = ln_chain(v32, gamma, beta, keep, eps)
    f_m, f_r, f_y = ln_floor_fwd(v64, gamma, beta, eps, e_v)
    yard('ln fwd y', tag, y, t_y, ref_y, f_y, half_ulp(ref_y, dtype))
    yard('ln fwd mean', tag, mean, t_m, ref_m, f_m)
    yard('ln fwd rstd', tag, rstd, t_r, ref_r, f_r)
    if keep is not None:
        assert bool((_bits(y)[keep == 0] == 0).all()), 'a dead row of y is not +0'


def check_ln_fwd(dev, N, C, which):
    code, dtype, name = DTYPES[which]
    x, res, gamma, beta = ln_inputs(N, C, dtype, which)
    eps = 1e-5
    if N == 0:
        lib = L()
        y, v, mean, rstd = (Out((4, C), dev, dtype) for _ in range(4))
        z = torch.zeros(4, C, dtype=dtype).to(dev)
        g = torch.zeros(C).to(dev)
        assert lib.get().msmc_add_ln_fwd(lib.ptr(z), None, lib.ptr(g), lib.ptr(g), None, lib.ptr(y.t), lib.ptr(v.t), lib.ptr(mean.t),
                                         lib.ptr(rstd.t), 0, C, eps, 0.0, None, 0, code, lib.stream(z)) == 0
        for o in (y, v, mean, rstd):
            assert bool(torch.isnan(o.get(written=False).float()).all()), 'N = 0 wrote something'
        return
    for with_res in (False, True):
        for keep in (None, keep_rows(N)):
            tag = '%dx%d %s%s%s' % (N, C, name, ' res' if with_res else '', ' keep' if keep is not None else '')
            r = res if with_res else None
            got = ln_fwd(dev, x, r, gamma, beta, keep, eps)
            v64 = x.double() + (r.double() if with_res else 0.0)
            v32 = x.float() + r.float() if with_res else x.float()
            assert same_bits(got[1], v64.to(dtype)), '%s: v is not x + res rounded once' % tag
            compare_ln_fwd(tag, got, v64, v32, gamma, beta, keep, eps, dtype)


def check_ln_planted(dev, C, eps):
    """fp32 rows: a constant one (rstd = 1 / sqrt(eps), y = beta), 1000 + randn (E[x^2] - E[x]^2 loses it), one element 1e4 among
    1e-3; and two ordinary rows"""
    gen = gen_for(2100, C)
    x = torch.randn(5, C, generator=gen)
    x[1] = 0.37
    x[2] = 1000.0 + torch.randn(C, generator=gen)
    x[3] = 1e-3
    x[3, C // 3] = 1e4
    gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
    tag = 'planted C%d eps %g' % (C, eps)
    got = ln_fwd(dev, x, None, gamma, beta, None, eps)
    assert same_bits(got[1], x)
    compare_ln_fwd(tag, got, x.double(), x, gamma, beta, None, eps, torch.float32)
    y, _, mean, rstd = got
    # the constant row by itself, against what it must be
    _, b_r, b_y = ln_floor_fwd(x.double(), gamma, beta, eps)
    held('ln fwd rstd constant', tag, rstd[1:2], torch.full((1,), 1.0 / math.sqrt(eps), dtype=torch.float64), b_r[1:2])
    held('ln fwd y constant', tag, y[1], beta.double(), b_y[1])
    # the offset row: E[x^2] - E[x]^2 in fp32 is off by ~1e6 u / var; the floor of rstd is far below that
    ref_r = ln_ref(x.double(), gamma, beta, None, eps)[2]
    assert float(b_r[2] / ref_r[2]) < 1e-3
    held('ln fwd rstd offset', tag, rstd[2:3], ref_r[2:3], b_r[2:3])


# ---- B: msmc_add_ln_bwd and msmc_add_ln_param_multi -------------------------------------------------------------------------------------
LN_BWD_SHAPES = ((1, 4), (16, 8), (17, 8), (33, 256), (19, 260), (18, 516), (18, 768), (5, 772), (3, 1024), (21, 67), (6, 1023),
                 (0, 8))


def ws_bytes(N, C):
    return int(L().get().msmc_add_ln_bwd_workspace(N, C))


def ln_bwd(dev, g, v, mean, rstd, gamma, keep, want_gres=True, params='own', prefill=None, p=0.0, word=None, salt=0, off=()):
    """-> gx, gres | None, dgamma | None, dbeta | None, workspace (all on the CPU).  params: 'own' (accumulate = 0), 'acc'
    (accumulate = 1 onto ``prefill``), 'none' (partials only)"""
    lib = L()
    N, C = g.shape
    code = 0 if g.dtype == torch.float32 else 1
    o = lambda name: 1 if name in off else 0
    gd, vd, md, rd = at(g, dev, o('g')), at(v, dev, o('v')), at(mean, dev), at(rstd, dev)
    gmd, kd, seed = at(gamma, dev, o('gamma')), at(keep, dev), seed_tensor(dev, word)
    nbytes = ws_bytes(N, C)

    def run():
        gx = Out((N, C), dev, g.dtype, o('gx'))
        gres = Out((N, C), dev, g.dtype, o('gres')) if want_gres else None
        ws = Out((nbytes // 4,), dev)
        dg = db = None
        if params != 'none':
            dg, db = Out((C,), dev), Out((C,), dev)
            if params == 'acc':
                dg.t.copy_(prefill[0].to(dev))
                db.t.copy_(prefill[1].to(dev))
        lib.call('msmc_add_ln_bwd', lib.ptr(gd), lib.ptr(vd), lib.ptr(md), lib.ptr(rd), lib.ptr(gmd), lib.ptr(kd), lib.ptr(gx.t),
                 lib.ptr(gres.t) if gres else None, lib.ptr(dg.t) if dg else None, lib.ptr(db.t) if db else None, lib.ptr(ws.t),
                 nbytes, N, C, p, lib.ptr(seed), salt, 1 if params == 'acc' else 0, code, lib.stream(gd))
        return tuple(t.get() if t is not None else torch.zeros(0) for t in (gx, gres, dg, db, ws))

    return twice(run)


def ln_bwd_inputs(N, C, dtype, key):
    gen = gen_for(2200, N, C, key)
    g = torch.randn(N, C, generator=gen).to(dtype)
    v = (0.3 + 1.5 * torch.randn(N, C, generator=gen)).to(dtype)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=gen)
    var, mean = torch.var_mean(v.double(), -1, unbiased=False) if N else (torch.zeros(0, dtype=torch.float64),) * 2
    eps = 1e-5
    return g, v, gamma, mean.float(), (1.0 / torch.sqrt(var + eps)).float(), eps, gen


def param_item(part, dgamma, dbeta, nblocks, C, accumulate):
    it = L().LnParamItem()
    it.part, it.dgamma, it.dbeta = part.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
    it.nblocks, it.C, it.accumulate, it.reserved = nblocks, C, accumulate, 0
    return it


def param_multi(items, like):
    lib = L()
    arr = (lib.LnParamItem * max(1, len(items)))(*items)
    return lib.get().msmc_add_ln_param_multi(arr, len(items), lib.stream(like))


def check_ln_bwd(dev, N, C, which):
    code, dtype, name = DTYPES[which]
    g, v, gamma, mean, rstd, eps, gen = ln_bwd_inputs(N, C, dtype, which)
    pre = (torch.randn(C, generator=gen), torch.randn(C, generator=gen))
    tag0 = '%dx%d %s' % (N, C, name)
    if N == 0:
        _, _, dg, db, _ = ln_bwd(dev, g, v, mean, rstd, gamma, None)
        assert bool((_bits(dg) == 0).all()) and bool((_bits(db) == 0).all()), 'N = 0: dgamma / dbeta are not +0'
        _, _, dg, db, _ = ln_bwd(dev, g, v, mean, rstd, gamma, None, params='acc', prefill=pre)
        assert same_bits(dg, pre[0]) and same_bits(db, pre[1]), 'N = 0 with accumulate changed dgamma / dbeta'
        return
    for keep in (None, keep_rows(N, 16 if N > 32 else 4)):
        tag = tag0 + (' keep' if keep is not None else '')
        ref = ln_bwd_ref(g, v, gamma, keep, eps, torch.float64)
        t32 = ln_bwd_ref(g, v, gamma, keep, eps, torch.float32)
        fl = ln_floor_bwd(g, v, gamma, keep, eps)
        gx, gres, dg, db, ws = ln_bwd(dev, g, v, mean, rstd, gamma, keep)
        h = half_ulp(ref[0], dtype)
        yard('ln bwd gx', tag, gx, t32[0], ref[0], fl[0], h)
        yard('ln bwd gres', tag, gres, t32[0], ref[0], fl[0], h)
        yard('ln bwd dgamma', tag, dg, t32[1], ref[1], fl[1])
        yard('ln bwd dbeta', tag, db, t32[2], ref[2], fl[2])
        assert same_bits(gx, gres), 'without dropout gx and gres differ'
        if keep is not None:
            dead = keep == 0                     # (a zero of either sign: 0 * gamma carries gamma's sign through the kernel's chain)
            assert bool((gx[dead] == 0).all()) and bool((gres[dead] == 0).all()), 'a dead row is not 0'
        # gres == nullptr: the same gx bits
        gx2, _, dg2, db2, _ = ln_bwd(dev, g, v, mean, rstd, gamma, keep, want_gres=False)
        assert same_bits(gx2, gx) and same_bits(dg2, dg) and same_bits(db2, db), 'gres == NULL changed a result'
        # accumulate = 1: the pre-fill plus the accumulate = 0 result, one rounding
        _, _, dga, dba, _ = ln_bwd(dev, g, v, mean, rstd, gamma, keep, params='acc', prefill=pre)
        for nm, got, p0, own in (('dgamma', dga, pre[0], dg), ('dbeta', dba, pre[1], db)):
            want = p0.double() + own.double()
            assert same_bits(got, want.float()), '%s: accumulate is not pre-fill + result rounded once' % nm
        # partials only, then msmc_add_ln_param_multi: bit-equal to the one-call route, with and without accumulate
        gx3, _, _, _, part = ln_bwd(dev, g, v, mean, rstd, gamma, keep, params='none')
        assert same_bits(gx3, gx) and same_bits(part, ws), 'the partial-only call differs'
        nblocks = (N + 15) // 16
        pd = part.to(dev)

        def multi():
            a, b, c, d = Out((C,), dev), Out((C,), dev), Out((C,), dev), Out((C,), dev)
            c.t.copy_(pre[0].to(dev))
            d.t.copy_(pre[1].to(dev))
            assert param_multi([param_item(pd, a.t, b.t, nblocks, C, 0), param_item(pd, c.t, d.t, nblocks, C, 1)], pd) == 0
            return a.get(), b.get(), c.get(), d.get()

        a, b, c, d = twice(multi)
        assert same_bits(a, dg) and same_bits(b, db), 'msmc_add_ln_param_multi differs from the one-call route'
        assert same_bits(c, dga) and same_bits(d, dba), 'msmc_add_ln_param_multi with accumulate differs from the one-call route'


def check_param_multi(dev):
    """0 items; 1 item; MSMC_LN_PARAM_MAX + 3 items of mixed C, nblocks (0 and 17 among them) and accumulate: every item equals
    the float64 sum of its partials over the blocks within (nblocks + 16) u sum |partial| and the pre-fill is added once"""
    lib = L()
    z = torch.zeros(4).to(dev)
    assert param_multi([], z) == 0
    assert lib.get().msmc_add_ln_param_multi(None, 0, lib.stream(z)) == 0
    assert lib.get().msmc_add_ln_param_multi(None, 1, lib.stream(z)) == E_SHAPE
    gen = gen_for(2300)
    shapes = [(8, 1), (67, 17), (260, 0), (1024, 3), (8, 16), (67, 2), (260, 17), (8, 33)]
    for count in (1, LN_PARAM_MAX + 3):
        spec = [shapes[(i + (1 if count == 1 else 0)) % len(shapes)] + (i % 3 == 1,) for i in range(count)]
        parts = [torch.randn(max(nb, 1), 2, C, generator=gen) for C, nb, _ in spec]
        pres = [torch.randn(2, C, generator=gen) for C, _, _ in spec]
        pd = [p.to(dev) for p in parts]

        def run():
            outs, items = [], []
            for (C, nb, acc), p, pre in zip(spec, pd, pres):
                a, b = Out((C,), dev), Out((C,), dev)
                if acc:
                    a.t.copy_(pre[0].to(dev))
                    b.t.copy_(pre[1].to(dev))
                outs += [a, b]
                items.append(param_item(p, a.t, b.t, nb, C, int(acc)))
            assert param_multi(items, z) == 0
            return tuple(o.get() for o in outs)

        got = twice(run)
        for i, ((C, nb, acc), p, pre) in enumerate(zip(spec, parts, pres)):
            p64 = p.double()[:nb]
            for k in (0, 1):
                want = p64[:, k].sum(0) + (pre[k].double() if acc else 0.0)
                bound = (nb + 16) * U * p64[:, k].abs().sum(0) + U * want.abs()
                held('param_multi %s' % ('dgamma', 'dbeta')[k], 'item %d of %d C%d nb%d acc%d' % (i, count, C, nb, acc), got[2 * i + k],
                     want, bound)
                if nb == 0 and not acc:
                    assert bool((_bits(got[2 * i + k]) == 0).all())


def check_ln_bwd_refusals(dev):
    """a workspace one byte short -> MSMC_E_WORKSPACE; p_drop outside [0, 1) -> MSMC_E_SHAPE in msmc_add_ln_bwd and msmc_gate_bwd,
    as in their forward entries; nothing is launched"""
    lib = L()
    N, C = 17, 8
    g, v, gamma, mean, rstd, eps, _ = ln_bwd_inputs(N, C, torch.float32, 0)
    gd, vd, md, rd, gmd = (t.to(dev) for t in (g, v, mean, rstd, gamma))
    gx, dg, db, ws = Out((N, C), dev), Out((C,), dev), Out((C,), dev), Out((ws_bytes(N, C) // 4,), dev)
    st = lib.stream(gd)

    def bwd(nbytes, p):
        return lib.get().msmc_add_ln_bwd(lib.ptr(gd), lib.ptr(vd), lib.ptr(md), lib.ptr(rd), lib.ptr(gmd), None, lib.ptr(gx.t), None,
                                         lib.ptr(dg.t), lib.ptr(db.t), lib.ptr(ws.t), nbytes, N, C, p, None, 0, 0, 0, st)

    assert ws_bytes(N, C) == 2 * 2 * C * 4
    assert bwd(ws_bytes(N, C) - 1, 0.0) == E_WORKSPACE
    for p in (-0.01, 1.0, 1.5):
        assert bwd(ws_bytes(N, C), p) == E_SHAPE, p
    x = torch.zeros(N, 2 * C).to(dev)
    gy = Out((N, 2 * C), dev)
    y = Out((N, C), dev)
    for p in (-0.01, 1.0, 1.5):
        assert lib.get().msmc_gate_bwd(lib.ptr(x), lib.ptr(gd), lib.ptr(gy.t), N, C, p, None, 0, 0, st) == E_SHAPE, p
        assert lib.get().msmc_gate_fwd(lib.ptr(x), lib.ptr(y.t), N, C, p, None, 0, 0, st) == E_SHAPE, p
        assert lib.get().msmc_add_ln_fwd(lib.ptr(vd), None, lib.ptr(gmd), lib.ptr(gmd), None, lib.ptr(gx.t), lib.ptr(gx.t), lib.ptr(dg.t),
                                         lib.ptr(db.t), N, C, eps, p, None, 0, 0, st) == E_SHAPE, p
    for o in (gx, dg, db, ws, gy, y):
        assert bool(torch.isnan(o.get(written=False)).all()), 'a refused call launched'
    # the largest accepted value below 1 and 0 itself are taken
    assert bwd(ws_bytes(N, C), 0.0) == 0
    assert lib.get().msmc_gate_bwd(lib.ptr(x), lib.ptr(gd), lib.ptr(gy.t), N, C, 0.999, None, 0, 0, st) == 0
    assert bwd(ws_bytes(N, C), 0.999) == 0
    gx.get()


# ---- misaligned operands (after the guard in csrc/norm.hip: the element path) ---------------------------------------------------------
MISALIGNED_FWD = ('x', 'res', 'y', 'v', 'gamma', 'beta')
MISALIGNED_BWD = ('g', 'v', 'gx', 'gres', 'gamma')


def check_misaligned(dev, which):
    """x, res, y, v, gamma, beta (forward) and g, v, gx, gres, gamma (backward), each in turn one element into a larger buffer at
    C % 4 == 0: the bars of A and B, and v bit-equal to the aligned call's"""
    code, dtype, name = DTYPES[which]
    N, C, eps = 6, 260, 1e-5
    x, res, gamma, beta = ln_inputs(N, C, dtype, 50 + which)
    keep = keep_rows(N)
    v64, v32 = x.double() + res.double(), x.float() + res.float()
    base = ln_fwd(dev, x, res, gamma, beta, keep, eps)
    for nm in MISALIGNED_FWD:
        got = ln_fwd(dev, x, res, gamma, beta, keep, eps, off=(nm,))
        assert same_bits(got[1], base[1]), nm
        compare_ln_fwd('%dx%d %s %s + 1' % (N, C, name, nm), got, v64, v32, gamma, beta, keep, eps, dtype)
    g, v, gamma, mean, rstd, eps, _ = ln_bwd_inputs(N, C, dtype, 60 + which)
    ref = ln_bwd_ref(g, v, gamma, keep, eps, torch.float64)
    t32 = ln_bwd_ref(g, v, gamma, keep, eps, torch.float32)
    fl = ln_floor_bwd(g, v, gamma, keep, eps)
    h = half_ulp(ref[0], dtype)
    for nm in MISALIGNED_BWD:
        tag = '%dx%d %s %s + 1' % (N, C, name, nm)
        gx, gres, dg, db, _ = ln_bwd(dev, g, v, mean, rstd, gamma, keep, off=(nm,))
        yard('ln bwd gx', tag, gx, t32[0], ref[0], fl[0], h)
        yard('ln bwd gres', tag, gres, t32[0], ref[0], fl[0], h)
        yard('ln bwd dgamma', tag, dg, t32[1], ref[1], fl[1])
        yard('ln bwd dbeta', tag, db, t32[2], ref[2], fl[2])


# ---- C: dropout ----------------------------------------------------------------------------------------------------------------------
P_DROP, WORD, SALT = 0.25, 12345, 77


def check_dropout_ln(dev, C, which):
    """msmc_add_ln_fwd / _bwd at p = 0.25 against the mask of msmc_dropout_add_fwd for the same seed word and salt"""
    code, dtype, name = DTYPES[which]
    N, eps, p = 9, 1e-5, P_DROP
    tag = '%dx%d %s p %.2f' % (N, C, name, p)
    x, res, gamma, beta = ln_inputs(N, C, dtype, 70 + which)
    x[x == 0] = 1.0
    M = drop_mask(dev, WORD, SALT, N * C, p).view(N, C)
    assert 0.6 < float(M.double().mean()) < 0.9
    m64 = M.double() / (1.0 - p)
    scale32 = torch.ones(1) / (torch.ones(1) - torch.tensor([p]))
    keep = keep_rows(N)
    got = ln_fwd(dev, x, res, gamma, beta, keep, eps, p, WORD, SALT)
    v = got[1]
    v64 = x.double() * m64 + res.double()
    held('dropout v', tag, v, v64, 3 * U * (x.double() * m64).abs() + U * v64.abs() + half_ulp(v64, dtype))
    # the zeros of v - res: exactly the dropped elements (x has no zero and a kept x / (1 - p) cannot vanish)
    assert torch.equal(v.double() - res.double() == 0, ~M) or dtype == torch.bfloat16
    assert bool((_bits(v)[~M] == _bits(res)[~M]).all()), 'a dropped element of v is not res'
    if dtype == torch.bfloat16:                  # a kept bf16 element may round back onto res only if |x| is far below |res|
        same = (v.double() == res.double()) & M
        assert bool(((x.double().abs() / (1 - p))[same] <= 2 * half_ulp(res.double(), dtype)[same]).all())
    compare_ln_fwd(tag, got, v64, x.float() * (M.float() * scale32) + res.float(), gamma, beta, keep, eps, dtype)
    # without a residual the dropped elements of v are +0
    got0 = ln_fwd(dev, x, None, gamma, beta, None, eps, p, WORD, SALT)
    assert torch.equal(got0[1] == 0, ~M) and bool((_bits(got0[1])[~M] == 0).all())
    # backward: gx = gres * M / (1 - p), one rounding of the product (three with the scale); gres as without dropout
    g, v_in, gamma, mean, rstd, eps, _ = ln_bwd_inputs(N, C, dtype, 80 + which)
    _, gres0, dg0, db0, _ = ln_bwd(dev, g, v_in, mean, rstd, gamma, keep)
    gx, gres, dg, db, _ = ln_bwd(dev, g, v_in, mean, rstd, gamma, keep, p=p, word=WORD, salt=SALT)
    assert same_bits(gres, gres0) and same_bits(dg, dg0) and same_bits(db, db0), 'dropout changed gres or a parameter gradient'
    assert bool((_bits(gx)[~M] == 0).all()), 'a dropped element of gx is not +0'
    # (gres is the rounded copy of the fp32 dv that gx scales: in bf16 both carry their own half-ulp)
    ref = ln_bwd_ref(g, v_in, gamma, keep, eps, torch.float64)[0] * m64
    if dtype == torch.float32:
        want = gres.double() * m64
        held('dropout gx', tag, gx, want, 3 * U * want.abs())
    else:
        want = gres.double() * m64
        held('dropout gx', tag, gx, want, (3 * U * want.abs() + (half_ulp(gres.double(), dtype) / (1 - p)) * M + half_ulp(want, dtype)))
    fl = ln_floor_bwd(g, v_in, gamma, keep, eps)[0] / (1 - p) + 3 * U * ref.abs()
    held('dropout gx vs float64', tag, gx, ref, fl + half_ulp(ref, dtype))


def check_dropout_gate_and_bwd(dev, which):
    """msmc_gate_fwd / _bwd take the mask at the OUTPUT index of [N][C]; msmc_dropout_bwd equals g * M / (1 - p)"""
    lib = L()
    code, dtype, name = DTYPES[which]
    N, C, p = 23, 48, P_DROP
    tag = '%dx%d %s p %.2f' % (N, C, name, p)
    gen = gen_for(2400, which)
    x = torch.randn(N, 2 * C, generator=gen).to(dtype)
    x[x == 0] = 0.5
    g = torch.randn(N, C, generator=gen).to(dtype)
    g[g == 0] = 0.5
    M = drop_mask(dev, WORD, SALT + 1, N * C, p).view(N, C)
    m64 = M.double() / (1 - p)
    y0, gx0 = gate_run(dev, x, g, 0.0, None, 0)
    y, gx = gate_run(dev, x, g, p, WORD, SALT + 1)
    assert torch.equal(y == 0, ~M) and bool((_bits(y)[~M] == 0).all()), 'the gate drops other elements than the mask'
    want = gate_ref(x, g, torch.float64, m64)
    t32 = gate_ref(x, g, torch.float32, m64)
    yard('gate fwd dropout', tag, y, t32[0], want[0], None, half_ulp(want[0], dtype) + 3 * U * want[0].abs())
    yard('gate bwd dropout', tag, gx, t32[1], want[1], None, half_ulp(want[1], dtype) + 3 * U * want[1].abs())
    dead = torch.cat((~M, ~M), 1)
    assert bool((gx[dead] == 0).all()), 'a dropped element has a gradient'
    assert bool((gx0[dead] != 0).any())
    # msmc_dropout_bwd
    n = N * C
    gd = g.to(dev)
    seed = seed_tensor(dev, WORD)

    def run():
        o = Out((n,), dev, dtype)
        lib.call('msmc_dropout_bwd', lib.ptr(gd), lib.ptr(o.t), n, p, lib.ptr(seed), SALT + 1, code, lib.stream(gd))
        return (o.get(),)

    (dgx,) = twice(run)
    want = g.double().view(-1) * m64.view(-1)
    held('dropout_bwd', tag, dgx, want, 3 * U * want.abs() + half_ulp(want, dtype))
    assert bool((_bits(dgx)[~M.view(-1)] == 0).all())
    # msmc_dropout_add_fwd with a residual
    res = torch.randn(n, generator=gen).to(dtype)
    rd = res.to(dev)

    def run2():
        o = Out((n,), dev, dtype)
        lib.call('msmc_dropout_add_fwd', lib.ptr(gd), lib.ptr(rd), lib.ptr(o.t), n, p, lib.ptr(seed), SALT + 1, code, lib.stream(gd))
        return (o.get(),)

    (ya,) = twice(run2)
    want2 = want + res.double()
    held('dropout_add', tag, ya, want2, 3 * U * want.abs() + U * want2.abs() + half_ulp(want2, dtype))
    assert bool((_bits(ya)[~M.view(-1)] == _bits(res)[~M.view(-1)]).all())


def check_seeding_and_rate(dev):
    """seed == NULL is seed word 0; another salt or the next seed word gives another mask that agrees with the first on about
    1 - 2 p (1 - p) of the elements; the keep rate over 65 536 elements lies within 5 sigma of 1 - p; V = 1 and V = 4 rows and both
    dtypes see the same mask"""
    n = 65536
    for p in (0.1, 0.25, 0.5):
        sigma = math.sqrt(p * (1 - p) / n)
        base = drop_mask(dev, 0, 5, n, p)
        assert torch.equal(drop_mask(dev, None, 5, n, p), base), 'seed == NULL is not seed word 0'
        assert torch.equal(drop_mask(dev, 0, 5, n, p, which=1), base), 'bf16 draws another mask'
        rate = float(base.double().mean())
        MEASURED.append(('keep rate', 'p %.2f' % p, rate, '%.2f sigma' % ((rate - (1 - p)) / sigma)))
        print('norm keep rate p %.2f: %.5f (%.2f sigma from %.2f)' % (p, rate, (rate - (1 - p)) / sigma, 1 - p))
        assert abs(rate - (1 - p)) <= 5 * sigma
        expect = 1 - 2 * p * (1 - p)
        s2 = math.sqrt(expect * (1 - expect) / n)
        for word, salt in ((0, 6), (1, 5)):
            other = drop_mask(dev, word, salt, n, p)
            agree = float((other == base).double().mean())
            MEASURED.append(('mask agreement', 'p %.2f word %d salt %d' % (p, word, salt), agree, 'expected %.4f' % expect))
            assert abs(agree - expect) <= 5 * s2, (p, word, salt, agree, expect)
            assert abs(float(other.double().mean()) - (1 - p)) <= 5 * sigma


# ---- D: msmc_fc_add_ln_fwd ------------------------------------------------------------------------------------------------------------
FC_SHAPES = ((1, 4, 32), (16, 16, 32), (17, 36, 32), (5, 256, 64), (33, 256, 128), (3, 260, 32), (18, 384, 64), (2, 640, 64),
             (4, 256, 256))


FC_BIAS = {32: 1.0, 48: 1.0, 64: 4.0, 128: 8.0, 256: 32.0}


def fc_inputs(N, C, K, cap=True):
    """a, W ~ 1 / sqrt(K), res ~ 1 and a bias of either sign in [b, 2 b), b = FC_BIAS[K].  The share of elements within the
    accumulation error E ~ 0.64 u K^1.5 of a rounding boundary is about 4 E / ulp(h): below half a percent it needs
    ulp(h) = 2^-7 b >= K^1.5 / 102 * 2^-8, which is how b grows with K.  The first seed of the case's own sequence whose float64
    reference keeps at most 1 % of the elements out is taken (found on the reference alone, never on a kernel's output)"""
    for attempt in range(64):
        gen = gen_for(2500, N, C, K, attempt)
        a = torch.randn(N, K, generator=gen).bfloat16()
        W = (torch.randn(C, K, generator=gen) / math.sqrt(K)).bfloat16()
        b0 = FC_BIAS[K]
        bias = (b0 * (1.0 + torch.rand(C, generator=gen))) * (torch.randint(0, 2, (C,), generator=gen).float() * 2 - 1)
        res = torch.randn(N, C, generator=gen).bfloat16()
        gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
        if not cap or int(fc_reference(a, W, bias, res)[3].sum()) <= 0.01 * N * C:
            return a, W, bias, res, gamma, beta
    raise AssertionError('no seed of the case keeps the elements left out below 1 %')


def fc_call(dev, ops, keep, N, C, K, eps, p=0.0, word=None, salt=0, outs=None):
    """ops: a, W, bias, res, gamma, beta already on the device -> rc, (y, v, mean, rstd) as Out"""
    lib = L()
    n_, c_ = max(N, 1), max(C, 4)
    y, v, mean, rstd = outs or (Out((n_, c_), dev, torch.bfloat16), Out((n_, c_), dev, torch.bfloat16), Out((n_,), dev), Out((n_,), dev))
    kd, seed = at(keep, dev), seed_tensor(dev, word)
    pt = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in ops]
    rc = lib.get().msmc_fc_add_ln_fwd(pt[0], pt[1], pt[2], pt[3], pt[4], pt[5], lib.ptr(kd), lib.ptr(y.t), lib.ptr(v.t),
                                      lib.ptr(mean.t), lib.ptr(rstd.t), N, C, K, eps, p, lib.ptr(seed), salt, lib.stream(y.t))
    return rc, (y, v, mean, rstd)


def fc_reference(a, W, bias, res, m64=None):
    """float64 h, v_ref = bf16(bf16(h) * m + res), the unrounded sum, and the elements within the accumulation error of a boundary"""
    a64, W64 = a.double(), W.double()
    h = a64 @ W64.t() + bias.double()
    K = a.shape[1]
    E = K * U * (a64.abs() @ W64.abs().t()) + U * h.abs()
    hb = h.bfloat16().double()
    m64 = torch.ones_like(h) if m64 is None else m64
    s = hb * m64 + res.double()
    # (bf16(h) + res is exact in fp32 and in float64 alike -- both are sums of two bf16 values -- so its rounding, ties included,
    # is the same on both sides: only the rounding of h itself can fall either way)
    amb = (h - E).bfloat16() != (h + E).bfloat16()
    return h, s.bfloat16(), s, amb


def check_fc(dev, n):
    N, C, K = FC_SHAPES[n]
    eps = 1e-5
    a, W, bias, res, gamma, beta = fc_inputs(N, C, K)
    ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
    h, v_ref, s, amb = fc_reference(a, W, bias, res)
    left = int(amb.sum())
    MEASURED.append(('fc v left out', '%dx%dx%d' % (N, C, K), left, 'of %d' % amb.numel()))
    print('norm fc %dx%dx%d: %d of %d elements within the accumulation error of a rounding boundary' % (N, C, K, left, amb.numel()))
    assert left <= 0.01 * amb.numel(), 'the case leaves more than 1 % out'
    for keep in (None, keep_rows(N)):
        tag = '%dx%dx%d%s' % (N, C, K, ' keep' if keep is not None else '')

        def run():
            rc, outs = fc_call(dev, ops, keep, N, C, K, eps)
            assert rc == 0
            return tuple(o.get() for o in outs)

        y, v, mean, rstd = twice(run)
        exact = _bits(v) == _bits(v_ref)
        assert bool(exact[~amb].all()), '%s: %d elements of v are not bf16(bf16(h) + res)' % (tag, int((~exact[~amb]).sum()))
        # one bf16 ulp of h moves the sum by as much: one ulp of v, or of h where v is the smaller (the larger ulp across a binade)
        one_ulp = 4 * torch.maximum(half_ulp(v_ref.double(), torch.bfloat16), half_ulp(h, torch.bfloat16))
        assert bool(((v.double() - v_ref.double()).abs() <= one_ulp)[amb].all()), 'an element differs by more than one bf16 ulp'
        # y against the LayerNorm of the returned v, mean / rstd against the statistics of the unrounded sum (module docstring)
        vr = v.double()
        ref_y = ln_ref(vr, gamma, beta, keep, eps)[0]
        f_y = ln_floor_fwd(vr, gamma, beta, eps, half_ulp(vr, torch.bfloat16) + 2 * U * vr.abs())[2]
        held('fc y', tag, y, ref_y, f_y + half_ulp(ref_y, torch.bfloat16))
        _, ref_m, ref_r = ln_ref(s, gamma, beta, None, eps)
        e_v = 2 * U * s.abs() + torch.where(amb, 4 * half_ulp(h, torch.bfloat16), torch.zeros_like(h))
        f_m, f_r, _ = ln_floor_fwd(s, gamma, beta, eps, e_v)
        held('fc mean', tag, mean, ref_m, f_m)
        held('fc rstd', tag, rstd, ref_r, f_r)
        if keep is not None:
            assert bool((_bits(y)[keep == 0] == 0).all()), 'a dead row of y is not +0'


def check_fc_dropout(dev):
    """the fused kernel with the same seed word and salt as the mask source: dropped positions and values of the two-step chain"""
    N, C, K, eps, p = 17, 36, 32, 1e-5, P_DROP
    a, W, bias, res, gamma, beta = fc_inputs(N, C, K)
    ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
    M = drop_mask(dev, WORD, SALT + 2, N * C, p).view(N, C)
    scale32 = float((torch.ones(1) / (torch.ones(1) - torch.tensor([p])))[0])
    h, _, _, _ = fc_reference(a, W, bias, res)
    hb = h.bfloat16().double()
    assert bool((hb != 0).all())

    def run():
        rc, outs = fc_call(dev, ops, None, N, C, K, eps, p, WORD, SALT + 2)
        assert rc == 0
        return tuple(o.get() for o in outs)

    y, v, mean, rstd = twice(run)
    assert bool((_bits(v)[~M] == _bits(res)[~M]).all()), 'a dropped element of v is not res'
    kept_same = (v.double() == res.double()) & M
    assert bool(((hb.abs() / (1 - p))[kept_same] <= 2 * half_ulp(res.double(), torch.bfloat16)[kept_same]).all()), \
        'an element the mask keeps was dropped'
    # values: bf16(h) ambiguous by one bf16 ulp of h near a boundary (scaled by 1 / (1 - p)), three roundings of the scaled product,
    # one of the sum, the bf16 rounding of v
    want = hb * M.double() * scale32 + res.double()
    bound = (4 * half_ulp(h, torch.bfloat16) / (1 - p) + 3 * U * hb.abs() / (1 - p)) * M + U * want.abs() + half_ulp(want, torch.bfloat16)
    held('fc dropout v', '%dx%dx%d p %.2f' % (N, C, K, p), v, want, bound)
    vr = v.double()
    ref_y = ln_ref(vr, gamma, beta, None, eps)[0]
    f_y = ln_floor_fwd(vr, gamma, beta, eps, half_ulp(vr, torch.bfloat16) + 2 * U * vr.abs())[2]
    held('fc dropout y', '%dx%dx%d p %.2f' % (N, C, K, p), y, ref_y, f_y + half_ulp(ref_y, torch.bfloat16))


def check_fc_refusals(dev):
    """C = 644, C = 6, K = 48, bias / gamma / beta / a off by 4 bytes, res off by 2 bytes, a null operand: MSMC_E_SHAPE, outputs NaN"""
    N, C, K, eps = 5, 36, 32, 1e-5
    outs = None
    calls = []
    for n_, c_, k_ in ((N, 644, K), (N, 6, K), (N, C, 48), (N, 0, K), (N, C, 0), (-1, C, K)):
        a, W, bias, res, gamma, beta = fc_inputs(max(n_, 1), max(c_, 4), max(k_, 32), cap=False)
        ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
        rc, o = fc_call(dev, ops, None, n_, c_, k_, eps)
        calls.append((('shape', n_, c_, k_), rc, o))
    a, W, bias, res, gamma, beta = fc_inputs(N, C, K)
    for k, nm in enumerate(('a', 'W', 'bias', 'res', 'gamma', 'beta')):
        ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
        ops[k] = None
        rc, o = fc_call(dev, ops, None, N, C, K, eps)
        calls.append((('null', nm), rc, o))
        t = (a, W, bias, res, gamma, beta)[k]
        step = 1 if (t.dtype == torch.float32 or nm == 'res') else 2          # 4 bytes (a, W, fp32) or 2 bytes (res)
        ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
        ops[k] = at(t, dev, step)
        rc, o = fc_call(dev, ops, None, N, C, K, eps)
        calls.append((('offset', nm), rc, o))
    for p in (-0.1, 1.0):
        ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
        rc, o = fc_call(dev, ops, None, N, C, K, eps, p)
        calls.append((('p', p), rc, o))
    # misaligned or missing outputs
    ops = [t.to(dev) for t in (a, W, bias, res, gamma, beta)]
    for k in (0, 1):
        o = [Out((N, C), dev, torch.bfloat16), Out((N, C), dev, torch.bfloat16), Out((N,), dev), Out((N,), dev)]
        o[k] = Out((N, C), dev, torch.bfloat16, off=1)
        rc, o = fc_call(dev, ops, None, N, C, K, eps, outs=tuple(o))
        calls.append((('offset out', k), rc, o))
    wrong = [(w, rc) for w, rc, _ in calls if rc != E_SHAPE]
    assert not wrong, wrong
    for _, _, o in calls:
        for t in o:
            assert bool(torch.isnan(t.get(written=False).float()).all()), 'a refused call launched'


# ---- E: gate and tanh ------------------------------------------------------------------------------------------------------------------
GATE_SHAPES = ((1, 1), (3, 5), (23, 48), (7, 257))
TANH_SIZES = (1, 255, 256, 257, 1000)
# past the 8 * MSMC_NUM_CU workgroups of the MI355X: elements for the kernels with one element per work-item (gate, tanh, row_mask),
# and for those with four (sum_n, dropout_add, dropout_bwd: 2 098 180 elements, 4 MB in bf16)
PAST_CAP_GPU = (8 * 256 * 256 + 257, 4 * 8 * 256 * 256 + 1028)
PLANTED_B = (0.0, 1e-4, -1e-4, 9.0, -9.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0)


def past_cap_emu():
    """the two sizes past the interpreter's own 8 * MSMC_NUM_CU workgroups (3 compute units unless MSMC_EMU_CUS says otherwise)"""
    import os
    cap = 8 * int(os.environ.get('MSMC_EMU_CUS', '3')) * 256
    return cap + 257, 4 * cap + 1028


def gate_run(dev, x, g, p, word, salt):
    lib = L()
    N, C = g.shape
    code = 0 if x.dtype == torch.float32 else 1
    xd, gd, seed = x.to(dev), g.to(dev), seed_tensor(dev, word)

    def run():
        y, gx = Out((N, C), dev, x.dtype), Out((N, 2 * C), dev, x.dtype)
        lib.call('msmc_gate_fwd', lib.ptr(xd), lib.ptr(y.t), N, C, p, lib.ptr(seed), salt, code, lib.stream(xd))
        lib.call('msmc_gate_bwd', lib.ptr(xd), lib.ptr(gd), lib.ptr(gx.t), N, C, p, lib.ptr(seed), salt, code, lib.stream(xd))
        return y.get(), gx.get()

    return twice(run)


def gate_ref(x, g, dtype, m=None):
    x_ = x.detach().clone().to(dtype).requires_grad_(True)
    C = g.shape[1]
    y = torch.tanh(x_[:, :C]) * torch.sigmoid(x_[:, C:])
    if m is not None:
        y = y * m.to(dtype)
    y.backward(g.to(dtype))
    return y.detach(), x_.grad


def gate_inputs(N, C, dtype, key):
    gen = gen_for(2600, N, C, key)
    x = (2.0 * torch.randn(N, 2 * C, generator=gen))
    flat = x.view(-1)
    k = min(len(PLANTED_B), flat.numel() // 2)
    if N * C >= len(PLANTED_B):
        x[0, C:C + min(C, k)] = torch.tensor(PLANTED_B[:min(C, k)])          # the sigmoid half
        x[-1, :min(C, k)] = torch.tensor(PLANTED_B[:min(C, k)])              # the tanh half
    return x.to(dtype), torch.randn(N, C, generator=gen).to(dtype)


def check_gate(dev, N, C, which):
    code, dtype, name = DTYPES[which]
    tag = '%dx%d %s' % (N, C, name)
    x, g = gate_inputs(N, C, dtype, which)
    y, gx = gate_run(dev, x, g, 0.0, None, 0)
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(gx.float()).all()), 'a gate value or gradient is not finite'
    want, t32 = gate_ref(x, g, torch.float64), gate_ref(x, g, torch.float32)
    yard('gate fwd', tag, y, t32[0], want[0], None, half_ulp(want[0], dtype))
    yard('gate bwd', tag, gx, t32[1], want[1], None, half_ulp(want[1], dtype))


def check_gate_overflow(dev, which):
    """b = -88.8 and below: expf(-b) is inf and the sigmoid 0; b = 100: expf(-b) is 0; tanh at +-20 is +-1: all finite, gradients too"""
    code, dtype, name = DTYPES[which]
    b = torch.tensor([-88.8, -89.0, -95.0, -1000.0, -3e38, 88.8, 100.0, 1000.0, 3e38, 0.0, 20.0, -20.0])
    C = b.numel()
    x = torch.cat((torch.tensor([0.5, -0.5, 20.0, -20.0, 3e38, -3e38, 0.0, 1e-4, -1e-4, 9.0, -9.0, 1.0]), b)).view(1, 2 * C).to(dtype)
    g = torch.full((1, C), 3.0).to(dtype)
    y, gx = gate_run(dev, x, g, 0.0, None, 0)
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(gx.float()).all()), (y, gx)
    want, t32 = gate_ref(x, g, torch.float64), gate_ref(x, g, torch.float32)
    assert bool(torch.isfinite(want[1]).all())
    # where expf(-b) is inf the kernel's sigmoid is 0 and the float64 one a positive number below the smallest normal fp32
    # (2^-126): that much, times |g| <= 4, is allowed on top of the bar
    tiny = 4 * 2.0 ** -126
    yard('gate fwd overflow', name, y, t32[0], want[0], None, half_ulp(want[0], dtype) + tiny)
    yard('gate bwd overflow', name, gx, t32[1], want[1], None, half_ulp(want[1], dtype) + tiny)
    assert bool((y[0, :5] == 0).all()), 'the sigmoid of b <= -88.8 is not 0'


def check_tanh(dev, n, which):
    lib = L()
    code, dtype, name = DTYPES[which]
    tag = 'n %d %s' % (n, name)
    gen = gen_for(2700, n, which)
    x = (2.0 * torch.randn(n, generator=gen))
    k = min(n, len(PLANTED_B))
    x[:k] = torch.tensor(PLANTED_B[:k])
    x = x.to(dtype)
    g = torch.randn(n, generator=gen)
    yin = torch.rand(n, generator=gen) * 2 - 1                          # the saved output the backward entries take
    if n >= 4:
        yin[0], yin[1], yin[2] = 1.0, -1.0, 0.0
    xd = x.to(dev)
    st = lib.stream(xd)

    def fwd():
        y, y32 = Out((n,), dev, dtype), Out((n,), dev)
        lib.call('msmc_tanh_fwd', lib.ptr(xd), lib.ptr(y.t), n, code, st)
        lib.call('msmc_tanh_f32_fwd', lib.ptr(xd), lib.ptr(y32.t), n, code, st)
        return y.get(), y32.get()

    y, y32 = twice(fwd)
    want, t32 = torch.tanh(x.double()), torch.tanh(x.float())
    yard('tanh fwd', tag, y, t32, want, None, half_ulp(want, dtype))
    yard('tanh_f32 fwd', tag, y32, t32, want)
    assert bool((y.float().abs() <= 1).all()) and bool((y32.abs() <= 1).all())
    # backward: from y in [-1, 1], +-1 included
    yb, gb = yin.to(dtype), g.to(dtype)
    ybd, gbd, y32d, g32d = yb.to(dev), gb.to(dev), yin.to(dev), g.to(dev)

    def bwd():
        gx, gx2 = Out((n,), dev, dtype), Out((n,), dev, dtype)
        lib.call('msmc_tanh_bwd', lib.ptr(ybd), lib.ptr(gbd), lib.ptr(gx.t), n, code, st)
        lib.call('msmc_tanh_f32_bwd', lib.ptr(y32d), lib.ptr(g32d), lib.ptr(gx2.t), n, code, st)
        return gx.get(), gx2.get()

    gx, gx2 = twice(bwd)
    for nm, got, yy, gg in (('tanh bwd', gx, yb.double(), gb.double()), ('tanh_f32 bwd', gx2, yin.double(), g.double())):
        want = gg * (1 - yy * yy)
        bound = gg.abs() * (U * yy * yy + 2 * U * (1 - yy * yy).abs()) * (1 + 2.0 ** -20) + half_ulp(want, dtype)
        held(nm, tag, got, want, bound)
        assert bool((got[yy.abs() == 1] == 0).all()), 'the gradient at y = +-1 is not 0'


# ---- F: sum_n, dropout_add at p = 0, row_mask -----------------------------------------------------------------------------------------
GLUE_SIZES = (0, 4, 1020, 1024, 1028)
ROW_MASK_SHAPES = ((1, 1), (4, 17), (3, 300))


def check_sum_n(dev, n, which):
    lib = L()
    code, dtype, name = DTYPES[which]
    gen = gen_for(2800, n, which)
    ops = [torch.randn(n, generator=gen).to(dtype) for _ in range(4)]
    dv = [t.to(dev) if n else torch.zeros(4, dtype=dtype).to(dev) for t in ops]
    st = lib.stream(dv[0])
    for k in (2, 3, 4):
        def run():
            out = Out((n,), dev, dtype)
            p = [lib.ptr(t) for t in dv[:k]] + [None] * (4 - k)
            lib.call('msmc_sum_n', p[0], p[1], p[2], p[3], lib.ptr(out.t) if n else lib.ptr(dv[0]), n, code, st)
            return (out.get(),)

        (got,) = twice(run)
        s32 = ops[0].float() + ops[1].float()
        for t in ops[2:k]:
            s32 = s32 + t.float()
        assert same_bits(got, s32.to(dtype)), 'sum_n of %d operands is not ((a + b) + c) + d rounded once' % k
        if n:
            want = sum(t.double() for t in ops[:k])
            held('sum_n %d' % k, 'n %d %s' % (n, name), got, want, (k - 1) * U * sum(t.double().abs() for t in ops[:k]) + half_ulp(want, dtype))
    # dropout_add at p = 0: x + res rounded once; without res a copy
    for with_res in (True, False):
        def run():
            out = Out((n,), dev, dtype)
            lib.call('msmc_dropout_add_fwd', lib.ptr(dv[0]), lib.ptr(dv[1]) if with_res else None, lib.ptr(out.t) if n else lib.ptr(dv[0]),
                     n, 0.0, None, 3, code, st)
            return (out.get(),)

        (got,) = twice(run)
        want = (ops[0].double() + ops[1].double()).to(dtype) if with_res else ops[0]
        assert same_bits(got, want), 'dropout_add at p = 0 is not x + res rounded once'


def check_glue_refusals(dev):
    """sum_n: d without c, n % 4 != 0, a misaligned operand; dropout_add / dropout_bwd: n % 4, misaligned, p outside [0, 1)"""
    lib = L()
    Lh = lib.get()
    for code, dtype, name in DTYPES:
        n = 64
        z = torch.zeros(n + 8, dtype=dtype).to(dev)
        out = Out((n,), dev, dtype)
        a, mis, o, st = lib.ptr(z[:n]), lib.ptr(z[1:n + 1]), lib.ptr(out.t), lib.stream(z)
        calls = [Lh.msmc_sum_n(a, a, None, a, o, n, code, st), Lh.msmc_sum_n(a, a, None, None, o, n - 2, code, st),
                 Lh.msmc_sum_n(mis, a, None, None, o, n, code, st), Lh.msmc_sum_n(a, mis, None, None, o, n, code, st),
                 Lh.msmc_sum_n(a, a, mis, None, o, n, code, st), Lh.msmc_sum_n(a, a, a, mis, o, n, code, st),
                 Lh.msmc_sum_n(a, a, None, None, mis, n, code, st), Lh.msmc_sum_n(None, a, None, None, o, n, code, st),
                 Lh.msmc_sum_n(a, a, None, None, o, n, 2, st), Lh.msmc_sum_n(a, a, None, None, o, -4, code, st),
                 Lh.msmc_dropout_add_fwd(a, None, o, n - 1, 0.0, None, 0, code, st), Lh.msmc_dropout_add_fwd(mis, None, o, n, 0.0, None, 0, code, st),
                 Lh.msmc_dropout_add_fwd(a, mis, o, n, 0.0, None, 0, code, st), Lh.msmc_dropout_add_fwd(a, None, o, n, 1.0, None, 0, code, st),
                 Lh.msmc_dropout_add_fwd(a, None, o, n, -0.5, None, 0, code, st), Lh.msmc_dropout_bwd(a, o, n, 1.0, None, 0, code, st),
                 Lh.msmc_dropout_bwd(mis, o, n, 0.5, None, 0, code, st), Lh.msmc_dropout_bwd(a, o, n - 3, 0.5, None, 0, code, st)]
        assert all(rc == E_SHAPE for rc in calls), calls
        assert bool(torch.isnan(out.get(written=False).float()).all()), 'a refused call launched'


def check_row_mask(dev, B, T):
    lib = L()
    lens = torch.tensor(([0, T, T + 5, -3, 1, T - 1] * B)[:B] if B > 1 else [T])
    want = torch.arange(T)[None, :] < lens[:, None]
    for lt in (torch.int32, torch.int64):
        ld = lens.to(lt).to(dev)
        for code, dtype, name in DTYPES:
            def run():
                keep = Out((B, T), dev, dtype)
                lib.call('msmc_row_mask', lib.ptr(ld), int(lt == torch.int64), lib.ptr(keep.t), B, T, code, lib.stream(ld))
                return (keep.get(),)

            (got,) = twice(run)
            assert same_bits(got, want.to(dtype)), 'row_mask %dx%d %s %s' % (B, T, lt, name)
    if B == 1:
        for b_, t_ in ((0, T), (B, 0), (-1, T)):
            keep = Out((4,), dev)
            ld = lens.to(torch.int32).to(dev)
            assert lib.get().msmc_row_mask(lib.ptr(ld), 0, lib.ptr(keep.t), b_, t_, 0, lib.stream(ld)) == E_SHAPE
            assert bool(torch.isnan(keep.get(written=False)).all())


def check_past_cap(dev, sizes):
    """sizes past the 8 * MSMC_NUM_CU workgroups of the grid-stride kernels, so that work-items take their stride a second time:
    ``n`` elements for gate, tanh and row_mask (one element per work-item), ``n_vec`` for sum_n, dropout_add and dropout_bwd (four
    per work-item: more than 4 * 256 * 8 * MSMC_NUM_CU elements), in bf16"""
    lib = L()
    n, n_vec = sizes
    assert n % 4 == 1 and n_vec % 4 == 0 and n_vec > 4 * (n - 257)
    check_tanh(dev, n, 0)
    check_row_mask(dev, 3, (n + 2) // 3)
    C = 257
    check_gate(dev, (n + C - 1) // C, C, 1)
    check_sum_n(dev, n_vec, 1)                                            # (sum_n of 2, 3, 4 operands and dropout_add at p = 0)
    p, word, salt = 0.25, 9, 9
    m = drop_mask(dev, word, salt, n_vec, p, which=1)
    sigma = math.sqrt(p * (1 - p) / n_vec)
    assert abs(float(m.double().mean()) - (1 - p)) <= 5 * sigma
    assert torch.equal(m[:1024], drop_mask(dev, word, salt, 1024, p)), 'the mask of an element depends on the grid'
    gen = gen_for(2850, n_vec)
    g = torch.randn(n_vec, generator=gen).bfloat16()
    res = torch.randn(n_vec, generator=gen).bfloat16()
    gd, rd, seed = g.to(dev), res.to(dev), seed_tensor(dev, word)

    def run():
        a, b = Out((n_vec,), dev, torch.bfloat16), Out((n_vec,), dev, torch.bfloat16)
        lib.call('msmc_dropout_bwd', lib.ptr(gd), lib.ptr(a.t), n_vec, p, lib.ptr(seed), salt, 1, lib.stream(gd))
        lib.call('msmc_dropout_add_fwd', lib.ptr(gd), lib.ptr(rd), lib.ptr(b.t), n_vec, p, lib.ptr(seed), salt, 1, lib.stream(gd))
        return a.get(), b.get()

    gx, y = twice(run)
    want = g.double() * m.double() / (1 - p)
    held('dropout_bwd', 'n %d bf16 p %.2f' % (n_vec, p), gx, want, 3 * U * want.abs() + half_ulp(want, torch.bfloat16))
    assert bool((_bits(gx)[~m] == 0).all())
    want2 = want + res.double()
    held('dropout_add', 'n %d bf16 p %.2f' % (n_vec, p), y, want2, 3 * U * want.abs() + U * want2.abs() + half_ulp(want2, torch.bfloat16))
    assert bool((_bits(y)[~m] == _bits(res)[~m]).all())


# ---- G: msmc_fft_prologue ---------------------------------------------------------------------------------------------------------------
PROLOGUE_SHAPES = ((1, 1, 1), (2, 5, 6), (3, 33, 24), (2, 45, 260), (5, 7, 67))


def prologue_call(dev, seq, lens, table, rows, out_dtype, Tp, with_bias=True, off=()):
    lib = L()
    B, T, C = seq.shape
    o = lambda name: 1 if name in off else 0
    sd, ld, td = at(seq, dev, o('seq')), lens.to(dev), at(table, dev, o('table'))
    out, keep = Out((B, T, C), dev, out_dtype, o('out')), Out((B * T,), dev, torch.float32)
    keep8 = torch.full((B * T + GUARD,), 0xAB, dtype=torch.uint8).to(dev)
    kb = Out((B, max(Tp, 1)), dev) if with_bias else None
    rc = lib.get().msmc_fft_prologue(lib.ptr(sd), lib.ptr(ld), int(lens.dtype == torch.int64), lib.ptr(td), rows, lib.ptr(out.t),
                                     lib.ptr(keep8), lib.ptr(kb.t) if kb else None, B, T, C, Tp, 0 if seq.dtype == torch.float32 else 1,
                                     0 if out_dtype == torch.float32 else 1, lib.stream(sd))
    return rc, out, keep8.cpu().to(torch.int16), kb


def check_prologue(dev, n):
    B, T, C = PROLOGUE_SHAPES[n]
    gen = gen_for(2900, B, T, C)
    table = torch.randn(T + 1, C, generator=gen)
    lens = torch.tensor(([T, 0, 1, T + 3, T - 1] * B)[:B])
    t_idx = torch.arange(T)[None, :]
    live = t_idx < lens[:, None]
    pos = torch.where(live, t_idx + 1, torch.zeros_like(t_idx))
    for which_in, (_, din, nin) in enumerate(DTYPES):
        seq = torch.randn(B, T, C, generator=gen).to(din)
        want = seq.double() + F_.embedding(pos, table.double())
        for _, dout, nout in DTYPES:
            for lt in (torch.int32, torch.int64):
                for Tp in (T, T + 1, T + 31, T + 63):
                    if (lt == torch.int64 or dout != din) and Tp not in (T, T + 63):
                        continue
                    tag = '%dx%dx%d %s->%s Tp %d' % (B, T, C, nin, nout, Tp)

                    def run():
                        rc, out, keep8, kb = prologue_call(dev, seq, lens.to(lt), table, T + 1, dout, Tp)
                        assert rc == 0
                        return out.get(), keep8, kb.get()

                    out, keep8, kb = twice(run)
                    held('prologue out', tag + (' int64' if lt == torch.int64 else ''), out, want, U * want.abs() + half_ulp(want, dout))
                    if din == dout == torch.float32:
                        assert same_bits(out, seq + F_.embedding(pos, table)), 'fp32 -> fp32 is not torch\'s fp32 sum'
                    assert torch.equal(keep8[:B * T].view(B, T), live.to(torch.int16)), 'keep_row'
                    assert bool((keep8[B * T:] == 0xAB).all()), 'keep_row was overrun'
                    wb = torch.full((B, Tp), float('-inf'))
                    wb[:, :T] = torch.where(live, torch.zeros(B, T), wb[:, :T])
                    assert same_bits(kb, wb), 'key_bias'
        # key_bias == NULL (Tp is then not looked at)
        rc, out, keep8, _ = prologue_call(dev, seq, lens, table, T + 1, din, 0, with_bias=False)
        assert rc == 0 and torch.equal(keep8[:B * T].view(B, T), live.to(torch.int16))
        held('prologue out', '%dx%dx%d %s no bias' % (B, T, C, nin), out.get(), want, U * want.abs() + half_ulp(want, din))
        # refusals: table_rows = T, Tp = T + 64, Tp < T
        for rows, Tp in ((T, T), (T + 1, T + 64), (T + 1, T - 1)):
            rc, out, keep8, kb = prologue_call(dev, seq, lens, table, rows, din, Tp)
            assert rc == E_SHAPE, (rows, Tp)
            assert bool(torch.isnan(out.get(written=False).float()).all()) and bool((keep8 == 0xAB).all())
            assert bool(torch.isnan(kb.get(written=False)).all())
        # misaligned seq / out / table at C % 4 == 0: the element path, same bars
        if C % 4 == 0:
            for nm in ('seq', 'out', 'table'):
                rc, out, keep8, kb = prologue_call(dev, seq, lens, table, T + 1, din, T + 5, off=(nm,))
                assert rc == 0
                held('prologue out', '%dx%dx%d %s %s + 1' % (B, T, C, nin, nm), out.get(), want, U * want.abs() + half_ulp(want, din))
                kb.get()


# ---- H: one pass through hip/norm.py ----------------------------------------------------------------------------------------------------
def check_host_route(dev):
    """add_layer_norm with leaf gamma / beta: two different LayerNorms and one applied twice in one backward pass (the deferred
    route: LN_PARAM_DEFER, _ln_flush), then a second pass that accumulates into the live .grad"""
    from msmctts_amd.hip import norm
    assert norm.LN_PARAM_DEFER
    N, C, eps = 19, 260, 1e-5
    gen = gen_for(3000)
    x0 = torch.randn(N, C, generator=gen)
    res = [torch.randn(N, C, generator=gen) for _ in range(3)]
    go = torch.randn(N, C, generator=gen)
    gb = [(1.0 + 0.5 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)) for _ in range(2)]
    keep = keep_rows(N)

    def chain(dtype, ln):
        x = x0.to(dtype)
        ps = [(g.clone().to(dtype).requires_grad_(True), b.clone().to(dtype).requires_grad_(True)) for g, b in gb]
        h = ln(x, res[0].to(dtype), ps[0][0], ps[0][1], None)
        h = ln(h, res[1].to(dtype), ps[1][0], ps[1][1], keep)
        h = ln(h, res[2].to(dtype), ps[0][0], ps[0][1], None)              # the first LayerNorm a second time
        return h, ps

    def stock(x, r, g, b, k):
        y = F_.layer_norm(x + r, (C,), g, b, eps) if x.dtype == torch.float64 else ln_chain(x + r, g, b, None, eps)[0]
        return y if k is None else y * k.to(x.dtype)[:, None]

    ref, ref_p = chain(torch.float64, stock)
    ref.backward(go.double())
    t32, t32_p = chain(torch.float32, stock)
    t32.backward(go)
    x = x0.to(dev)
    ps = [(g.clone().to(dev).requires_grad_(True), b.clone().to(dev).requires_grad_(True)) for g, b in gb]
    before = len(MEASURED)
    for rnd in (1, 2):
        h = norm.add_layer_norm(x, res[0].to(dev), ps[0][0], ps[0][1], None, eps=eps)
        h = norm.add_layer_norm(h, res[1].to(dev), ps[1][0], ps[1][1], keep.to(dev), eps=eps)
        h = norm.add_layer_norm(h, res[2].to(dev), ps[0][0], ps[0][1], None, eps=eps)
        h.backward(go.to(dev))
        if rnd == 1:
            yard('host route y', '19x260', h.detach().cpu(), t32.detach(), ref.detach())
        for i in (0, 1):
            for j, nm in ((0, 'dgamma'), (1, 'dbeta')):
                got = ps[i][j].grad.detach().cpu()
                yard('host route %s' % nm, 'LayerNorm %d pass %d' % (i, rnd), got, rnd * t32_p[i][j].grad, rnd * ref_p[i][j].grad)
    assert len(MEASURED) - before == 9
    assert not norm._LN_PENDING['items']
