"""Shared cases of the spectral front-end kernels (csrc/spectral.hip: framing, magnitude, the two-channel image, log-clamp, the
multi-stage launch) and of the two chains hip/spectral.py builds on them: tests/test_spectral_emu.py runs them on the kernel
interpreter, tests/test_gpu_spectral.py on the GPU.

Reference of every comparison: stock torch operators on the CPU in float64, from the same fp32 input bits, and their autograd
gradients.  No reference restates a kernel's index formula.  Every output is pre-filled with NaN (none may remain); every padding
column of an INPUT holds NaN too, so a kernel that reads one is caught the same way.  Every case runs twice and the two results
must agree bit for bit.

Bars (u = 2^-24, the build uses -ffp-contract=off):
  framing       forward: bit-exact (a copy), padding columns +0.  Backward with integer gradients: bit-exact (every fp32 sum is
                exact).  Backward with random gradients: n u A, A the same autograd applied to |g|, n = 3 ceil(n_fft / hop) the
                largest number of terms of one sample.  Adjointness to 1e-6.
  magnitude     forward 4 u |ref| (two products, a sum, + lo in mode 0, a root: <= 2.5 u), backward 8 u |ref| (the forward error
                of the saved magnitude, a product, a quotient: <= 4.5 u); sqrtf and / are correctly rounded in the gfx950 code
                (v_sqrt_f32 corrected by one ulp either way from two fma residuals; v_div_scale / v_rcp / fma chain /
                v_div_fmas / v_div_fixup; fp32 denormals on, no fast-math flag: profiles/spectral_direct.md), so nothing is
                added to the count.  Padding columns and the gradient under the mode-1 clamp exactly 0.
  image         channel 0: the input bits (bf16: round to nearest even, as ``.to(torch.bfloat16)``).  Channel 1:
                8 u (|20 log10 m| + 100) / 100, bf16 plus one bf16 half-ulp of the reference.  Backward
                8 u (|g0| + |g1 0.2 / (ln 10 m)|), padding columns exactly 0.
  log-clamp     forward 4 u max(1, |ref|), backward 2 u |ref| above the gate and exactly 0 below.
  chains        the project's yardstick rule (tests/_attn32cases.py): at most RATIO = 4 x the error of torch's own fp32 chain
                on the CPU against float64, in the max norm and in the L2 norm, output and waveform gradient.
Every comparison is appended to MEASURED and printed; the figures are recorded in profiles/spectral_direct.md.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F_

U = 2.0 ** -24
E_SHAPE = -2
RATIO = 4.0
MEASURED = []          # (what, case, share of the bound used | ratio to torch's fp32 chain)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _nan(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), float('nan'), dtype=dtype).to(dev)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def twice(run):
    """``run()`` -> tuple of result tensors from freshly NaN-filled outputs; run two times, bit-identical; -> the first"""
    first, second = run(), run()
    for a, b in zip(first, second):
        assert same_bits(a, b), 'a repeated call changed bits'
    return first


def held(what, case, got, ref, bound):
    """|got - ref| <= bound element by element (a NaN in ``got`` fails); records the largest share of the bound used"""
    got, err = got.double(), (got.double() - ref).abs()
    assert not bool(torch.isnan(got).any()), '%s %s: an element was not written' % (what, case)
    pos = bound > 0
    used = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    MEASURED.append((what, case, used))
    print('spectral %-28s %-30s share of the bound used %.3f' % (what, case, used))
    bad = ~(err <= bound)
    assert not bool(bad.any()), '%s %s: %d elements outside the bound, worst err %.3e at bound %.3e' % (
        what, case, int(bad.sum()), float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def _op(kind, a, out, b=None, c=None, dtype=0, **kw):
    from msmctts_amd.hip import lib
    o = lib.SpectralOp()
    o.kind, o.dtype = kind, dtype
    o.a, o.out = (a.data_ptr() if a is not None else None), (out.data_ptr() if out is not None else None)
    o.b, o.c = (b.data_ptr() if b is not None else None), (c.data_ptr() if c is not None else None)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _multi(ops, like):
    from msmctts_amd.hip import lib
    return lib.get().msmc_spectral_multi((lib.SpectralOp * len(ops))(*ops), len(ops), lib.stream(like))


# ---- 1: framing -------------------------------------------------------------------------------------------------------------------
# B, L, n_fft, NP, hop, pad, T
FRAME_CASES = (
    (1, 9, 8, 8, 2, 4, 5),                   # smallest centred shape
    (2, 5, 8, 8, 1, 4, 6),                   # L = pad + 1: every sample reflected on both sides, last index exactly 2L - 2
    (3, 50, 12, 12, 5, 6, 11),               # hop divides L
    (2, 53, 12, 12, 5, 6, 11),               # L % hop != 0: the right reflection partly covered
    (2, 64, 10, 12, 3, 2, 22),               # trimmed window: NP > n_fft, pad < n_fft / 2
    (2, 40, 6, 8, 7, 3, 6),                  # hop > n_fft: samples no frame reads
    (1, 30, 8, 8, 2, 4, 7),                  # T short of full coverage: tail samples get exactly 0
    (2, 2400, 200, 200, 50, 100, 49),        # a hop-50 front-end's shape
)
FRAME_IDS = ['B%d L%d n%d NP%d hop%d pad%d T%d' % c for c in FRAME_CASES]


def frames_ref(x64, n_fft, hop, pad, T):
    """frames [B, T, n_fft] of the reflect-padded signal by stock pad + unfold; R: the smallest right pad that covers frame T - 1"""
    L = x64.shape[-1]
    R = max(0, (T - 1) * hop + n_fft - pad - L)
    assert pad <= L - 1 and R <= L - 1, 'the case leaves the single reflection'
    return F_.pad(x64, (pad, R), mode='reflect').unfold(-1, n_fft, hop)[:, :T]


def frames_grad_ref(g64, L, n_fft, hop, pad, T):
    x = torch.zeros(g64.shape[0], L, dtype=torch.float64, requires_grad=True)
    frames_ref(x, n_fft, hop, pad, T).backward(g64)
    return x.grad


def frames_fwd(dev, x, case):
    from msmctts_amd.hip import lib
    B, L, n_fft, NP, hop, pad, T = case
    xd, fr = x.to(dev), _nan((B, T, NP), dev)
    lib.call('msmc_stft_frames_fwd', lib.ptr(xd), lib.ptr(fr), B, L, T, n_fft, NP, hop, pad, lib.stream(xd))
    return fr.cpu()


def frames_bwd(dev, g, case):
    from msmctts_amd.hip import lib
    B, L, n_fft, NP, hop, pad, T = case
    gd, gx = g.to(dev), _nan((B, L), dev)
    lib.call('msmc_stft_frames_bwd', lib.ptr(gd), lib.ptr(gx), B, L, T, n_fft, NP, hop, pad, lib.stream(gd))
    return gx.cpu()


def frame_inputs(n):
    """x [B, L]; integer-valued and random gradients [B, T, NP] whose padding columns hold NaN (no sample is read through them)"""
    B, L, n_fft, NP, hop, pad, T = FRAME_CASES[n]
    gen = torch.Generator().manual_seed(1100 + n)
    x = torch.randn(B, L, generator=gen)
    gi = torch.randint(-8, 9, (B, T, NP), generator=gen).float()
    gr = torch.randn(B, T, NP, generator=gen)
    gi[..., n_fft:] = float('nan')
    gr[..., n_fft:] = float('nan')
    return x, gi, gr


def check_frames_forward(dev, n):
    case = FRAME_CASES[n]
    B, L, n_fft, NP, hop, pad, T = case
    x, _, _ = frame_inputs(n)
    want = frames_ref(x.double(), n_fft, hop, pad, T).float()          # (a copy: exact in fp32)
    (fr,) = twice(lambda: (frames_fwd(dev, x, case),))
    assert not bool(torch.isnan(fr).any()), 'an element of frames was not written'
    assert same_bits(fr[..., :n_fft], want), 'frames differ from pad + unfold'
    assert bool((_bits(fr[..., n_fft:]) == 0).all()), 'a padding column is not +0'


def check_frames_backward(dev, n):
    case = FRAME_CASES[n]
    B, L, n_fft, NP, hop, pad, T = case
    x, gi, gr = frame_inputs(n)
    reads = frames_grad_ref(torch.ones(B, T, n_fft, dtype=torch.float64), L, n_fft, hop, pad, T)      # how often a sample is read
    if n in (5, 6):
        assert bool((reads == 0).any()), 'the case was chosen for samples that no frame reads'
    # integer-valued gradient: every fp32 partial sum is an integer below 2^24, so the result is the float64 one bit for bit
    want = frames_grad_ref(gi[..., :n_fft].double(), L, n_fft, hop, pad, T)
    (gx,) = twice(lambda: (frames_bwd(dev, gi, case),))
    assert not bool(torch.isnan(gx).any()), 'an element of gx was not written'
    assert bool((gx.double() == want).all()), 'the overlap-add of an integer gradient is not exact: %d samples differ, first at %s' % (
        int((gx.double() != want).sum()), (gx.double() != want).nonzero()[0].tolist())
    assert bool((_bits(gx)[reads == 0] == 0).all()), 'a sample that no frame reads is not +0'
    assert bool((_bits(gx)[gx == 0] == 0).all()), 'a zero sum is -0'
    # random gradient: n u A
    want = frames_grad_ref(gr[..., :n_fft].double(), L, n_fft, hop, pad, T)
    A = frames_grad_ref(gr[..., :n_fft].double().abs(), L, n_fft, hop, pad, T)
    terms = 3 * int(math.ceil(n_fft / float(hop)))
    assert float(reads.max()) <= terms
    (gx,) = twice(lambda: (frames_bwd(dev, gr, case),))
    held('frames bwd', FRAME_IDS[n], gx, want, terms * U * A)
    # adjointness <frames(x), g> = <x, frames_bwd(g)> on the kernels' own outputs, in float64
    fr = frames_fwd(dev, x, case)[..., :n_fft].double()
    lhs, rhs = float((fr * gr[..., :n_fft].double()).sum()), float((x.double() * gx.double()).sum())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    MEASURED.append(('frames adjoint', FRAME_IDS[n], rel / 1e-6))
    print('spectral %-28s %-30s <Ax, g> %.9e  <x, A*g> %.9e  rel %.2e' % ('frames adjoint', FRAME_IDS[n], lhs, rhs, rel))
    assert rel <= 1e-6, (lhs, rhs)


# ---- 2: magnitude -------------------------------------------------------------------------------------------------------------------
# R, F, CP, FP
MAG_CASES = ((1, 1, 4, 4), (7, 5, 12, 8), (33, 101, 204, 104))
MAG_CASES_GPU = ((2100, 257, 516, 260),)                               # R * CP over a million: past the 2048-workgroup cap
MAG_LO = {1: 1e-7, 0: 1e-9}                                            # clamp_mode -> the lo the host layer passes with it


def mag_inputs(case, mode):
    """spec [R, CP] (re | im | NaN padding), gmag [R, FP] (NaN padding), lo as the fp32 the kernel receives.  Planted by flat index
    mod 11: 1 re = 0, 2 im = 0, 3 both, 4 re^2 + im^2 <= lo / 4, 5 re^2 + im^2 >= 4 lo (just above); the rest randn"""
    R, F, CP, FP = case
    lo = float(np.float32(MAG_LO[mode]))
    gen = torch.Generator().manual_seed(1200 + 7 * R + mode)
    re, im = torch.randn(R, F, generator=gen), torch.randn(R, F, generator=gen)
    k = torch.arange(R * F).view(R, F) % 11
    ang = torch.rand(R, F, generator=gen, dtype=torch.float64) * 2 * math.pi
    frac = torch.rand(R, F, generator=gen, dtype=torch.float64)
    small = math.sqrt(lo / 4) * (0.05 + 0.9 * frac)                    # radius: s <= 0.9025 lo / 4
    above = math.sqrt(4 * lo) * (1.05 + frac)                          # radius: s >= 1.1 * 4 lo
    for sel, rad in ((k == 4, small), (k == 5, above)):
        re[sel] = (rad * torch.cos(ang))[sel].float()
        im[sel] = (rad * torch.sin(ang))[sel].float()
    while True:
        re[(k == 1) | (k == 3)] = 0.0
        im[(k == 2) | (k == 3)] = 0.0
        s = re.double() ** 2 + im.double() ** 2
        near = (s > lo / 4) & (s < 4 * lo)                            # a randn pair (or single, beside a planted 0) in between
        if not bool(near.any()):
            break
        re[near], im[near] = torch.randn(int(near.sum()), generator=gen), torch.randn(int(near.sum()), generator=gen)
    spec =torch.full((R, CP), float('nan'))
    spec[:, :F], spec[:, F:2 * F] = re, im
    gmag = torch.full((R, FP), float('nan'))
    gmag[:, :F] = torch.randn(R, F, generator=gen)
    return spec, gmag, lo


def mag_ref(spec, gmag, F, lo, mode):
    re, im = spec[:, :F].double().requires_grad_(True), spec[:, F:2 * F].double().requires_grad_(True)
    s = re * re + im * im
    assert not bool(((s > lo / 2) & (s < 2 * lo)).any()), 'an element lies within a factor 2 of lo: the gate would be ambiguous'
    mag = torch.sqrt(torch.clamp(s, min=lo)) if mode else torch.sqrt(s + lo)
    mag.backward(gmag[:, :F].double())
    return mag.detach(), torch.cat((re.grad, im.grad), 1), s.detach()


def check_magnitude(dev, case, mode):
    from msmctts_amd.hip import lib
    R, F, CP, FP = case
    tag = 'R%d F%d CP%d FP%d mode %d' % (case + (mode,))
    spec, gmag, lo = mag_inputs(case, mode)
    want, want_g, s = mag_ref(spec, gmag, F, lo, mode)
    if R * F >= 11:
        assert bool((s == 0).any()) and bool(((s > 0) & (s <= lo / 4)).any()) and bool(((s >= 4 * lo) & (s < 64 * lo)).any())
    sd, gd = spec.to(dev), gmag.to(dev)

    def fwd():
        mag = _nan((R, FP), dev)
        lib.call('msmc_spec_mag_fwd', lib.ptr(sd), lib.ptr(mag), R, F, CP, FP, lo, mode, lib.stream(sd))
        return (mag.cpu(),)

    (mag,) = twice(fwd)
    held('magnitude fwd', tag, mag[:, :F], want, 4 * U * want.abs())
    assert bool((_bits(mag[:, F:]) == 0).all()), 'a padding column of mag is not +0'
    saved = mag.clone()
    saved[:, F:] = float('nan')                                        # (the backward kernel reads no padding column)
    md = saved.to(dev)

    def bwd():
        gs = _nan((R, CP), dev)
        lib.call('msmc_spec_mag_bwd', lib.ptr(sd), lib.ptr(md), lib.ptr(gd), lib.ptr(gs), R, F, CP, FP, lo, mode, lib.stream(sd))
        return (gs.cpu(),)

    (gs,) = twice(bwd)
    held('magnitude bwd', tag, gs[:, :2 * F], want_g, 8 * U * want_g.abs())
    assert bool((_bits(gs[:, 2 * F:]) == 0).all()), 'a padding column of gspec is not +0'
    if mode:
        under = torch.cat((s < lo, s < lo), 1)
        assert bool((gs[:, :2 * F][under] == 0).all()), 'the gradient under the clamp is not 0'
    # swapped halves would pass only if re and im had equal gradients
    assert R * F < 11 or not torch.equal(want_g[:, :F], want_g[:, F:])


# ---- 3: the two-channel image ---------------------------------------------------------------------------------------------------------
# B, T, F, FP
IMAGE_CASES = ((1, 1, 1, 4), (2, 7, 5, 8), (3, 49, 101, 104))
IMAGE_DTYPES = ((0, torch.float32, 'fp32'), (1, torch.bfloat16, 'bf16'))


def _log_channel(m64):
    return (20.0 * torch.log10(m64) + 80.0) / 100.0


def image_inputs(n):
    """mel [B, T, FP] positive, log-uniform over 1e-6 .. 1e3 (log channel over -0.4 .. 1.4: both clamp ends), NaN padding columns, one
    exact 0 where there is more than one element; values whose log channel lies within 2e-4 of 0 or 1 are drawn again"""
    B, T, F, FP = IMAGE_CASES[n]
    gen = torch.Generator().manual_seed(1300 + n)

    def draw(k):
        return (10.0 ** (torch.rand(k, generator=gen, dtype=torch.float64) * 9.0 - 6.0)).float()

    m = draw(B * T * F)
    while True:
        lg = _log_channel(m.double())
        near = (lg.abs() < 2e-4) | ((lg - 1).abs() < 2e-4)
        if not bool(near.any()):
            break
        m[near] = draw(int(near.sum()))
    if m.numel() > 1:
        m[m.numel() // 2] = 0.0
    mel = torch.full((B, T, FP), float('nan'))
    mel[..., :F] = m.view(B, T, F)
    return mel


def image_ref(mel, F, gimg=None):
    """float64 image [B, F, T, 2] = stack(m, clamp((20 log10 m + 80) / 100, 0, 1)) and, with ``gimg``, its autograd gradient [B, T, F]"""
    m = mel[..., :F].double().requires_grad_(gimg is not None)
    lg = _log_channel(m)
    free = lg.detach()
    assert not bool(((free.abs() < 1e-4) | ((free - 1).abs() < 1e-4)).any()), 'a log value lies within 1e-4 of a clamp edge'
    img = torch.stack((m, torch.clamp(lg, 0.0, 1.0)), -1).permute(0, 2, 1, 3)
    if gimg is None:
        return img, None
    img.backward(gimg.double())
    return img.detach(), m.grad


def check_image(dev, n, which):
    from msmctts_amd.hip import lib
    code, dtype, name = IMAGE_DTYPES[which]
    B, T, F, FP = IMAGE_CASES[n]
    tag = 'B%d T%d F%d FP%d %s' % (B, T, F, FP, name)
    mel = image_inputs(n)
    gen = torch.Generator().manual_seed(1350 + n)
    gimg = torch.randn(B, F, T, 2, generator=gen).to(dtype)
    want, want_g = image_ref(mel, F, gimg)
    m = mel[..., :F].transpose(1, 2)                                      # [B, F, T] fp32
    zero = m == 0
    if m.numel() > 1:
        assert int(zero.sum()) == 1
    if m.numel() >= 50:
        free = _log_channel(m.double())
        assert bool((free < 0).any()) and bool((free > 1).any()) and bool(((free > 0) & (free < 1)).any())
    md, gd = mel.to(dev), gimg.to(dev)

    def fwd():
        img = _nan((B, F, T, 2), dev, dtype)
        lib.call('msmc_mrd_image_fwd_dt', lib.ptr(md), lib.ptr(img), B, T, F, FP, code, lib.stream(md))
        return (img.cpu(),)

    (img,) = twice(fwd)
    assert img.dtype == dtype
    assert same_bits(img[..., 0], m.to(dtype)), 'channel 0 is not the input (rounded to nearest even in bf16)'
    bound = 8 * U * ((20.0 * torch.log10(m.double())).abs() + 100.0) / 100.0
    ref1 = want[..., 1]
    if dtype == torch.bfloat16:
        _, e = torch.frexp(ref1)                                         # ref = f 2^e, f in [0.5, 1): half a bf16 ulp is 2^(e - 9)
        bound = bound + torch.where(ref1 == 0, torch.zeros_like(ref1), torch.ldexp(torch.ones_like(ref1), e - 9))
    assert bool((img[..., 1][zero] == 0).all()), 'the log channel of an exact 0 is not 0'
    held('image fwd ch1', tag, img[..., 1][~zero], ref1[~zero], bound[~zero])

    def bwd():
        gm = _nan((B, T, FP), dev)
        lib.call('msmc_mrd_image_bwd_dt', lib.ptr(md), lib.ptr(gd), lib.ptr(gm), B, T, F, FP, code, lib.stream(md))
        return (gm.cpu(),)

    (gm,) = twice(bwd)
    assert not bool(torch.isnan(gm).any()), 'an element of gmel was not written'
    assert bool((_bits(gm[..., F:]) == 0).all()), 'a padding column of gmel is not +0'
    got = gm[..., :F].transpose(1, 2)                                     # [B, F, T]
    want_g = want_g.transpose(1, 2)
    g0, g1 = gimg[..., 0].double(), gimg[..., 1].double()
    # float64 autograd gives 0 * inf = NaN at the exact 0 (and nowhere else); the clamp is active there: the gradient is g0 itself
    assert torch.equal(torch.isnan(want_g), zero)
    assert bool((got[zero].double() == g0[zero]).all()), 'the gradient at an exact 0 is not that of channel 0'
    bound = 8 * U * (g0.abs() + (g1 * 0.2 / (math.log(10.0) * m.double())).abs())
    held('image bwd', tag, got[~zero], want_g[~zero], bound[~zero])


# ---- 4: log-clamp -------------------------------------------------------------------------------------------------------------------
LOG_SIZES = (1, 1023, 4100)
LOG_SIZES_GPU = (2200000,)                                             # past the 2048-workgroup cap
LOG_LO = 1e-5


def log_inputs(n):
    """x [n] positive, log-uniform over 1e-3 .. 1e2; planted by index mod 7: 1 an exact 0, 2 a value <= lo / 4, 3 one >= 4 lo (just
    above); g [n] randn"""
    lo = float(np.float32(LOG_LO))
    gen = torch.Generator().manual_seed(1400 + n % 1000)
    x = (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 5.0 - 3.0)).float()
    frac = torch.rand(n, generator=gen, dtype=torch.float64)
    k = torch.arange(n) % 7
    x[k == 1] = 0.0
    x[k == 2] = ((lo / 4) * (0.05 + 0.9 * frac))[k == 2].float()
    x[k == 3] = ((4 * lo) * (1.05 + frac))[k == 3].float()
    return x, torch.randn(n, generator=gen), lo


def check_log_clamp(dev, n):
    from msmctts_amd.hip import lib
    x, g, lo = log_inputs(n)
    x64 = x.double().requires_grad_(True)
    assert not bool(((x64 > lo / 2) & (x64 < 2 * lo)).any()), 'an element lies within a factor 2 of lo'
    want = torch.log(torch.clamp(x64, min=lo))
    want.backward(g.double())
    want, want_g = want.detach(), x64.grad
    if n >= 7:
        assert bool((x == 0).any()) and bool(((x > 0) & (x <= lo / 4)).any()) and bool(((x >= 4 * lo) & (x < 16 * lo)).any())
    xd, gd = x.to(dev), g.to(dev)

    def fwd():
        y = _nan((n,), dev)
        lib.call('msmc_log_clamp_fwd', lib.ptr(xd), lib.ptr(y), n, lo, lib.stream(xd))
        return (y.cpu(),)

    def bwd():
        gx = _nan((n,), dev)
        lib.call('msmc_log_clamp_bwd', lib.ptr(xd), lib.ptr(gd), lib.ptr(gx), n, lo, lib.stream(xd))
        return (gx.cpu(),)

    (y,) = twice(fwd)
    held('log-clamp fwd', 'n %d' % n, y, want, 4 * U * torch.clamp(want.abs(), min=1.0))
    (gx,) = twice(bwd)
    held('log-clamp bwd', 'n %d' % n, gx, want_g, 2 * U * want_g.abs())
    assert bool((gx[x.double() < lo] == 0).all()), 'the gradient below the gate is not 0'


# ---- 5: several stages in one launch --------------------------------------------------------------------------------------------------
def check_multi(dev):
    """one edge case of every kind hip/spectral.py issues through ``_multi`` -- 0 1 2 3 4 5 6 8 9; it calls msmc_log_clamp_bwd (kind 7)
    directly, so kind 7 is left to the product tests -- against the single entries on the same buffers, bit for bit.  The launch holds
    at most MSMC_SPECTRAL_MULTI_MAX = 8 operations and there are nine kinds: two launches, the first eight and the last eight, so
    that every kind runs next to seven others."""
    from msmctts_amd.hip import lib
    st = None
    fcase = FRAME_CASES[3]
    B, L, n_fft, NP, hop, pad, T = fcase
    x, _, gr = frame_inputs(3)
    mcase, mode = MAG_CASES[1], 1
    R, F, CP, FP = mcase
    spec, gmag, lo = mag_inputs(mcase, mode)
    iB, iT, iF, iFP = IMAGE_CASES[1]
    mel = image_inputs(1)
    gen = torch.Generator().manual_seed(1500)
    gimg2 = torch.randn(iB, iF, iT, 2, generator=gen)
    gimg1 = torch.randn(iB, iF, iT, 1, generator=gen).bfloat16()
    n = LOG_SIZES[1]
    lx, _, llo = log_inputs(n)
    xd, grd, sd, gmd, md, g2d, g1d, lxd = (v.to(dev) for v in (x, gr, spec, gmag, mel, gimg2, gimg1, lx))
    st = lib.stream(xd)
    mag = _nan((R, FP), dev)
    lib.call('msmc_spec_mag_fwd', lib.ptr(sd), lib.ptr(mag), R, F, CP, FP, lo, mode, st)
    shapes = [((B, T, NP), torch.float32), ((B, L), torch.float32), ((R, FP), torch.float32), ((R, CP), torch.float32),
              ((iB, iF, iT, 2), torch.bfloat16), ((iB, iT, iFP), torch.float32), ((n,), torch.float32),
              ((iB, iF, iT, 1), torch.float32), ((iB, iT, iFP), torch.float32)]

    def outputs():
        return [_nan(s, dev, d) for s, d in shapes]

    single = outputs()
    lib.call('msmc_stft_frames_fwd', lib.ptr(xd), lib.ptr(single[0]), B, L, T, n_fft, NP, hop, pad, st)
    lib.call('msmc_stft_frames_bwd', lib.ptr(grd), lib.ptr(single[1]), B, L, T, n_fft, NP, hop, pad, st)
    lib.call('msmc_spec_mag_fwd', lib.ptr(sd), lib.ptr(single[2]), R, F, CP, FP, lo, mode, st)
    lib.call('msmc_spec_mag_bwd', lib.ptr(sd), lib.ptr(mag), lib.ptr(gmd), lib.ptr(single[3]), R, F, CP, FP, lo, mode, st)
    lib.call('msmc_mrd_image_fwd_dt', lib.ptr(md), lib.ptr(single[4]), iB, iT, iF, iFP, 1, st)
    lib.call('msmc_mrd_image_bwd_dt', lib.ptr(md), lib.ptr(g2d), lib.ptr(single[5]), iB, iT, iF, iFP, 0, st)
    lib.call('msmc_log_clamp_fwd', lib.ptr(lxd), lib.ptr(single[6]), n, llo, st)
    lib.call('msmc_mrd_image1_fwd_dt', lib.ptr(md), lib.ptr(single[7]), iB, iT, iF, iFP, 1, 0, st)
    lib.call('msmc_mrd_image1_bwd_dt', lib.ptr(md), lib.ptr(g1d), lib.ptr(single[8]), iB, iT, iF, iFP, 1, 1, st)
    single = [v.cpu() for v in single]
    assert not any(bool(torch.isnan(v.float()).any()) for v in single)

    def ops_for(out):
        return [_op(0, xd, out[0], B=B, L=L, T=T, n_fft=n_fft, NP=NP, hop=hop, pad=pad),
                _op(1, grd, out[1], B=B, L=L, T=T, n_fft=n_fft, NP=NP, hop=hop, pad=pad),
                _op(2, sd, out[2], R=R, F=F, CP=CP, FP=FP, lo=lo, clamp_mode=mode),
                _op(3, sd, out[3], b=mag, c=gmd, R=R, F=F, CP=CP, FP=FP, lo=lo, clamp_mode=mode),
                _op(4, md, out[4], dtype=1, B=iB, T=iT, F=iF, FP=iFP),
                _op(5, md, out[5], b=g2d, dtype=0, B=iB, T=iT, F=iF, FP=iFP),
                _op(6, lxd, out[6], R=n, lo=llo),
                _op(8, md, out[7], dtype=0, B=iB, T=iT, F=iF, FP=iFP, channel=1),
                _op(9, md, out[8], b=g1d, dtype=1, B=iB, T=iT, F=iF, FP=iFP, channel=1)]

    for part in (slice(0, 8), slice(1, 9)):
        def run():
            out = outputs()
            assert _multi(ops_for(out)[part], xd) == 0
            return tuple(v.cpu() for v in out[part])
        got = twice(run)
        for k, (a, b) in enumerate(zip(got, single[part])):
            assert same_bits(a, b), 'operation %d of the launch differs from its single entry' % (part.start + k)


# ---- 6: the chains through the host layer ---------------------------------------------------------------------------------------------
CHAIN_B, CHAIN_L, CHAIN_MELS = 2, 403, 10
# tag, chain, n_fft, hop, window length
CHAIN_CASES = (
    ('stft full window', 'stft', 64, 16, 64),
    ('stft window 40 in 64', 'stft', 64, 16, 40),                      # the trimmed form
    ('log_mel hop 20', 'log_mel', 64, 20, 40),                         # pad (64 - 20) / 2 = 22 does not centre
)
CHAIN_IDS = [c[0] for c in CHAIN_CASES]


def torch_chain(kind, x, win, fb, go, n_fft, hop, dtype):
    """the stock chain (torch.stft) and its waveform gradient in ``dtype`` on the CPU"""
    x = x.to(dtype).requires_grad_(True)
    if kind == 'stft':
        sp = torch.stft(x, n_fft, hop_length=hop, win_length=win.numel(), window=win.to(dtype), center=True, pad_mode='reflect',
                        normalized=False, onesided=True, return_complex=True)
        s = sp.real ** 2 + sp.imag ** 2
        out = torch.sqrt(torch.clamp(s, min=float(np.float32(1e-7)))).transpose(1, 2)                 # [B, T, F]
    else:
        pad = int((n_fft - hop) / 2)
        y = F_.pad(x.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
        sp = torch.stft(y, n_fft, hop_length=hop, win_length=win.numel(), window=win.to(dtype), center=False, normalized=False,
                        onesided=True, return_complex=True)
        mag = torch.sqrt(sp.real ** 2 + sp.imag ** 2 + float(np.float32(1e-9)))
        mel = torch.matmul(fb.to(dtype), mag)                                                          # [B, M, T]
        out = torch.log(torch.clamp(mel, min=float(np.float32(1e-5)))).transpose(1, 2).unsqueeze(1)    # [B, 1, T, M]
    (out * go.to(dtype)).sum().backward()
    return out.detach(), x.grad


def check_chain(dev, n):
    from msmctts_amd.hip import spectral
    tag, kind, n_fft, hop, wl = CHAIN_CASES[n]
    F = n_fft // 2 + 1
    gen = torch.Generator().manual_seed(1600 + n)
    x = torch.randn(CHAIN_B, CHAIN_L, generator=gen)
    win = torch.rand(wl, generator=gen) * 0.9 + 0.1
    fb = torch.rand(CHAIN_MELS, F, generator=gen)
    left = (n_fft - wl) // 2
    dft = spectral.dft_basis(n_fft, F_.pad(win, (left, n_fft - wl - left)), False, dev)
    xd = x.clone().to(dev).requires_grad_(True)
    if kind == 'stft':
        out = spectral.stft_magnitude(xd, n_fft, hop, dft, 1e-7)
    else:
        out = spectral.log_mel(xd, n_fft, hop, dft, spectral.projection(fb.t(), dev), CHAIN_MELS)
    go = torch.randn(out.shape, generator=gen)
    out.backward(go.to(dev))
    ref, ref_g = torch_chain(kind, x, win, fb, go, n_fft, hop, torch.float64)
    t32, t32_g = torch_chain(kind, x, win, fb, go, n_fft, hop, torch.float32)
    assert tuple(out.shape) == tuple(ref.shape)
    failed = []
    for name, got, mid, want in (('out', out.detach().cpu(), t32, ref), ('grad', xd.grad.cpu(), t32_g, ref_g)):
        assert not bool(torch.isnan(got).any())
        for norm, f in (('max', lambda d: float(d.abs().max())), ('l2', lambda d: float(d.norm()))):
            ek, et = f(got.double() - want), f(mid.double() - want)
            MEASURED.append(('chain %s %s' % (name, norm), tag, ek / et))
            print('spectral chain %-22s %-4s %-3s err kernels %.3e  torch fp32 %.3e  ratio %.2f' % (tag, name, norm, ek, et, ek / et))
            if not ek <= RATIO * et:
                failed.append('%s %s: kernels %.3e > %.0f x torch fp32 %.3e' % (name, norm, ek, RATIO, et))
    assert not failed, (tag, failed)


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------
def first_refused_T(L, n_fft, hop, pad):
    """the smallest T whose last frame reads past the single right reflection (position 2L - 2)"""
    T = 1
    while (T - 1) * hop + n_fft - 1 - pad <= 2 * L - 2:
        T += 1
    return T


def check_frames_past_the_reflection_are_refused(dev):
    """msmc_stft_frames_fwd / _bwd and kinds 0 / 1 of msmc_spectral_multi return the shape error for the first T whose last frame
    passes position 2L - 2 and launch nothing (the NaN-filled outputs stay NaN); the largest T before it is accepted and equals the
    pad + unfold reference, its last index being the last one a single reflection reaches"""
    from msmctts_amd.hip import lib, spectral
    Lh = lib.get()
    for n, (B, L, n_fft, NP, hop, pad, _) in enumerate(FRAME_CASES[:7]):
        bad = first_refused_T(L, n_fft, hop, pad)
        x, _, _ = frame_inputs(n)
        xd = x.to(dev)
        st = lib.stream(xd)
        for T in (bad, bad + 1, bad + 1000):
            fr, gx = _nan((B, bad, NP), dev), _nan((B, L), dev)
            g = torch.zeros(B, bad, NP).to(dev)
            assert Lh.msmc_stft_frames_fwd(lib.ptr(xd), lib.ptr(fr), B, L, T, n_fft, NP, hop, pad, st) == E_SHAPE, (n, T)
            assert Lh.msmc_stft_frames_bwd(lib.ptr(g), lib.ptr(gx), B, L, T, n_fft, NP, hop, pad, st) == E_SHAPE, (n, T)
            assert _multi([_op(0, xd, fr, B=B, L=L, T=T, n_fft=n_fft, NP=NP, hop=hop, pad=pad)], xd) == E_SHAPE, (n, T)
            assert _multi([_op(1, g, gx, B=B, L=L, T=T, n_fft=n_fft, NP=NP, hop=hop, pad=pad)], xd) == E_SHAPE, (n, T)
            assert bool(torch.isnan(fr.cpu()).all()) and bool(torch.isnan(gx.cpu()).all()), 'a refused call launched'
        if bad > 1:
            case = (B, L, n_fft, NP, hop, pad, bad - 1)
            fr = frames_fwd(dev, x, case)
            assert same_bits(fr[..., :n_fft], frames_ref(x.double(), n_fft, hop, pad, bad - 1).float()), n
    x = torch.randn(2, 5).to(dev)
    with _raises(RuntimeError, 'msmc_stft_frames_fwd failed with code -2'):
        spectral._Frames.apply(x, 7, 8, 8, 1, 4)


def check_host_shapes_are_accepted(dev):
    """every shape the host layer produces passes the predicate: the centred form T = L // hop + 1, pad = n_fft / 2 (less the
    trimmed window's offset) and the log_mel form T = (L + 2 pad - n_fft) // hop + 1, pad = (n_fft - hop) / 2, on the framing table's
    (L, n_fft, hop), the chain cases and the resolution front-ends' n_fft = 4 hop"""
    from msmctts_amd.hip import lib
    Lh = lib.get()
    forms = []
    for B, L, n_fft, NP, hop, pad, _ in FRAME_CASES:
        if L > n_fft // 2:
            forms.append((L, L // hop + 1, n_fft, hop, n_fft // 2))
        p = int((n_fft - hop) / 2)
        if n_fft >= hop and L > p:
            forms.append((L, (L + 2 * p - n_fft) // hop + 1, n_fft, hop, p))
    for tag, kind, n_fft, hop, wl in CHAIN_CASES:
        lo = (n_fft - wl) // 2
        p = int((n_fft - hop) / 2)
        forms.append((CHAIN_L, CHAIN_L // hop + 1, wl, hop, n_fft // 2 - lo))
        forms.append((CHAIN_L, (CHAIN_L + 2 * p - n_fft) // hop + 1, wl, hop, p - lo))
    for hop in (25, 50, 100, 150, 300):
        for L in (2400, 2410, 601):
            forms.append((L, L // hop + 1, 4 * hop, hop, 2 * hop))
    assert len(forms) > 30
    for L, T, n_fft, hop, pad in forms:
        NP = (n_fft + 3) // 4 * 4
        x = torch.zeros(1, L).to(dev)
        fr, gx = _nan((1, T, NP), dev), _nan((1, L), dev)
        st = lib.stream(x)
        assert Lh.msmc_stft_frames_fwd(lib.ptr(x), lib.ptr(fr), 1, L, T, n_fft, NP, hop, pad, st) == 0, (L, T, n_fft, hop, pad)
        assert Lh.msmc_stft_frames_bwd(lib.ptr(fr), lib.ptr(gx), 1, L, T, n_fft, NP, hop, pad, st) == 0, (L, T, n_fft, hop, pad)
        assert _multi([_op(0, x, fr, B=1, L=L, T=T, n_fft=n_fft, NP=NP, hop=hop, pad=pad),
                       _op(1, fr, gx, B=1, L=L, T=T, n_fft=n_fft, NP=NP, hop=hop, pad=pad)], x) == 0
        assert bool((fr.cpu() == 0).all()) and bool((gx.cpu() == 0).all())


class _raises(object):
    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc) and self.text in str(val), (tp, val)
        return True


def check_rejected_arguments(dev):
    """the refusals the entries already had -- null pointers, L <= pad, NP < n_fft, CP < 2F, FP < F, dtype outside 0 / 1, n <= 0 --
    return the shape error and launch nothing (the NaN-filled outputs stay NaN)"""
    from msmctts_amd.hip import lib
    Lh = lib.get()
    B, L, n_fft, NP, hop, pad, T = FRAME_CASES[0]
    R, F, CP, FP = MAG_CASES[1]
    iB, iT, iF, iFP = IMAGE_CASES[1]
    n = 64
    z = torch.zeros(4096).to(dev)                                      # (any input: larger than every operand here)
    out = _nan((4096,), dev)
    out16 = _nan((4096,), dev, torch.bfloat16)
    p, o, o16, st = lib.ptr(z), lib.ptr(out), lib.ptr(out16), lib.stream(z)
    calls = []
    # framing: (x, out, B, L, T, n_fft, NP, hop, pad)
    for a in ((None, o, B, L, T, n_fft, NP, hop, pad), (p, None, B, L, T, n_fft, NP, hop, pad),
              (p, o, B, pad, T, n_fft, NP, hop, pad), (p, o, B, pad - 1, T, n_fft, NP, hop, pad),          # L <= pad
              (p, o, B, L, T, n_fft, n_fft - 1, hop, pad)):                                               # NP < n_fft
        calls.append(('frames_fwd', Lh.msmc_stft_frames_fwd(*(a + (st,)))))
        calls.append(('frames_bwd', Lh.msmc_stft_frames_bwd(*(a + (st,)))))
        if a[0] is not None and a[1] is not None:
            for kind in (0, 1):
                calls.append(('multi %d' % kind, _multi([_op(kind, z, out, B=a[2], L=a[3], T=a[4], n_fft=a[5], NP=a[6], hop=a[7],
                                                             pad=a[8])], z)))
    # magnitude: (R, F, CP, FP)
    for r_, f_, cp_, fp_ in ((R, F, 2 * F - 1, FP), (R, F, CP, F - 1)):                                    # CP < 2F, FP < F
        calls.append(('mag_fwd', Lh.msmc_spec_mag_fwd(p, o, r_, f_, cp_, fp_, 1e-7, 1, st)))
        calls.append(('mag_bwd', Lh.msmc_spec_mag_bwd(p, p, p, o, r_, f_, cp_, fp_, 1e-7, 1, st)))
        calls.append(('multi 2', _multi([_op(2, z, out, R=r_, F=f_, CP=cp_, FP=fp_, lo=1e-7, clamp_mode=1)], z)))
        calls.append(('multi 3', _multi([_op(3, z, out, b=z, c=z, R=r_, F=f_, CP=cp_, FP=fp_, lo=1e-7, clamp_mode=1)], z)))
    calls.append(('mag_fwd null', Lh.msmc_spec_mag_fwd(None, o, R, F, CP, FP, 1e-7, 1, st)))
    calls.append(('mag_fwd null', Lh.msmc_spec_mag_fwd(p, None, R, F, CP, FP, 1e-7, 1, st)))
    for k in range(4):
        a = [p, p, p, o]
        a[k] = None
        calls.append(('mag_bwd null', Lh.msmc_spec_mag_bwd(*(a + [R, F, CP, FP, 1e-7, 1, st]))))
    # image: FP < F, dtype outside 0 / 1, null pointers
    for fp_, dt in ((iF - 1, 0), (iFP, 2), (iFP, -1)):
        calls.append(('image_fwd', Lh.msmc_mrd_image_fwd_dt(p, o, iB, iT, iF, fp_, dt, st)))
        calls.append(('image_bwd', Lh.msmc_mrd_image_bwd_dt(p, p, o, iB, iT, iF, fp_, dt, st)))
        calls.append(('multi 4', _multi([_op(4, z, out, dtype=dt, B=iB, T=iT, F=iF, FP=fp_)], z)))
        calls.append(('multi 5', _multi([_op(5, z, out, b=z, dtype=dt, B=iB, T=iT, F=iF, FP=fp_)], z)))
    calls.append(('image_fwd null', Lh.msmc_mrd_image_fwd_dt(None, o, iB, iT, iF, iFP, 0, st)))
    calls.append(('image_fwd null', Lh.msmc_mrd_image_fwd_dt(p, None, iB, iT, iF, iFP, 1, st)))
    calls.append(('image_bwd null', Lh.msmc_mrd_image_bwd_dt(None, p, o, iB, iT, iF, iFP, 0, st)))
    calls.append(('image_bwd null', Lh.msmc_mrd_image_bwd_dt(p, None, o16, iB, iT, iF, iFP, 1, st)))
    calls.append(('image_bwd null', Lh.msmc_mrd_image_bwd_dt(p, p, None, iB, iT, iF, iFP, 0, st)))
    # log-clamp: n <= 0, null pointers
    for n_ in (0, -5):
        calls.append(('log_fwd', Lh.msmc_log_clamp_fwd(p, o, n_, 1e-5, st)))
        calls.append(('log_bwd', Lh.msmc_log_clamp_bwd(p, p, o, n_, 1e-5, st)))
        calls.append(('multi 6', _multi([_op(6, z, out, R=n_, lo=1e-5)], z)))
        calls.append(('multi 7', _multi([_op(7, z, out, b=z, R=n_, lo=1e-5)], z)))
    calls.append(('log_fwd null', Lh.msmc_log_clamp_fwd(None, o, n, 1e-5, st)))
    calls.append(('log_fwd null', Lh.msmc_log_clamp_fwd(p, None, n, 1e-5, st)))
    calls.append(('log_bwd null', Lh.msmc_log_clamp_bwd(None, p, o, n, 1e-5, st)))
    calls.append(('log_bwd null', Lh.msmc_log_clamp_bwd(p, None, o, n, 1e-5, st)))
    calls.append(('log_bwd null', Lh.msmc_log_clamp_bwd(p, p, None, n, 1e-5, st)))
    calls.append(('multi null', _multi([_op(6, None, out, R=n, lo=1e-5)], z)))
    calls.append(('multi null', _multi([_op(6, z, None, R=n, lo=1e-5)], z)))
    calls.append(('multi null', _multi([_op(7, z, out, R=n, lo=1e-5)], z)))
    assert len(calls) > 60
    wrong = [(name, rc) for name, rc in calls if rc != E_SHAPE]
    assert not wrong, wrong
    assert bool(torch.isnan(out.cpu()).all()) and bool(torch.isnan(out16.float().cpu()).all()), 'a refused call launched'
