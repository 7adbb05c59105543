"""Shared cases of the waveform preparation: csrc/resample.hip (msmc_resample, msmc_peak_scale), its host side
(msmctts_amd/hip/resample.py ``Resampler`` / ``prepare_waveforms``), ``read_wav_channels``, tools/prepare_wavs.py and the
``--resample`` path of tools/extract_features.py.  tests/test_resample_emu.py runs them on the kernel interpreter,
tests/test_gpu_resample.py on the GPU.

Reference.  ``restated`` is the definition of csrc/resample.hip in float64 numpy, written from the prototype filter and not from
the polyphase bank: g = gcd, up = rate_out / g, down = rate_in / g, mx = max(up, down), half = ceil(zeros mx / rolloff),
fc = rolloff / mx, h[k] = up fc sinc(fc k) I0(beta sqrt(1 - (k / half)^2)) / I0(beta) for |k| <= half;
xbar = the mean of the channels (int16 / 32768); y[n] = sum_i xbar[i] h[n down - i up] over 0 <= i < L, |n down - i up| <= half,
for n < ceil(L up / down).  ``check_restatement_is_resample_poly`` holds it against scipy.signal.resample_poly(x, up, down,
window=h / up) before it judges anything.

Bound on y (every element, none left out).  u = 2^-24.  The kernel's documented order is acc = fl(acc + fl(bank[p][j] x[.])) for
j = 0 .. P - 1 from +0.  A term carries the rounding of its tap to fp32 (bank built in float64, rounded once), of its product and
of at most P additions: a factor (1 + d)^(P + 2), |d| <= u, and (1 + u)^(P + 2) - 1 <= (P + 3) u while (P + 2)(P + 3) u <= 1
(P <= 1024 gives 0.07).  The taps the kernel adds as products with +0 change nothing.  The downmix of C > 1 channels is C - 1
additions and one division, (1 + u)^C - 1 <= C u (1 + 2^-10) of mean_c |x_c|; C == 1 and the int16 scaling are exact.  So
    bound[n] = u ((P + 3) sum_k |h_k| |xbar_k| + [C > 1] C sum_k |h_k| mean_c |x_c,k|) (1 + 2^-10) + P 2^-126
(the factor covers the second-order cross terms, the last term products that underflow).  Nothing in it is fitted to an observed
error; the kernel's share of it is printed.

Everything else -- int16 against fp32, the pure downmix, ragged batches with poisoned padding against solo runs, repeats, a wider
Lmax_in, the normalisation given the kernel's own y -- is compared BIT FOR BIT."""
import math
import os
import wave
from fractions import Fraction

import numpy as np
import torch

from _featurecases import _raises, same_bits
import _featurecases as fcases

E_SHAPE = -2
ROOT = fcases.ROOT
U = 2.0 ** -24
SMALL = dict(zeros=4, rolloff=0.9, beta=6.0)
BEST = dict(zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492)
TARGET = np.float32(10.0 ** (-7.0 / 20.0))


def resampler(dev, rate_in, rate_out, **kw):
    from msmctts_amd.hip.resample import Resampler
    return Resampler(rate_in, rate_out, device=dev, **kw)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def design(up, down, zeros, rolloff, beta):
    """(h float64 [2 half + 1], half, P)"""
    mx = max(up, down)
    half = int(math.ceil(zeros * mx / rolloff))
    fc = rolloff / mx
    k = np.arange(-half, half + 1, dtype=np.float64)
    win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (k / half) ** 2))) / np.i0(beta)
    return up * fc * np.sinc(fc * k) * win, half, -(-(2 * half + 1) // up)


def as_float64(x):
    """[L] or [L, C], fp32 or int16 -> float64 [L, C]"""
    x = np.asarray(x)
    scale = 1.0 / 32768.0 if x.dtype == np.int16 else 1.0
    return (x.astype(np.float64) * scale).reshape(len(x), -1)


_REF = {}


def restated(x, up, down, conf):
    """float64: (y [L_out], S1 = sum |h| |xbar| [L_out], S2 = sum |h| mean_c |x_c| [L_out], P), computed once per input"""
    x = np.asarray(x)
    key = (x.tobytes(), x.dtype.str, x.shape, up, down, tuple(sorted(conf.items())))
    if key not in _REF:
        h, half, P = design(up, down, **conf)
        xc = as_float64(x)
        xbar, xabs = xc.mean(axis=1), np.abs(xc).mean(axis=1)
        L = len(xbar)
        Lo = -(-L * up // down)
        y, s1, s2 = np.zeros(Lo), np.zeros(Lo), np.zeros(Lo)
        for n in range(Lo):
            lo = max(0, -((half - n * down) // up))                  # ceil((n down - half) / up)
            hi = min(L - 1, (n * down + half) // up)
            if hi < lo:
                continue
            i = np.arange(lo, hi + 1)
            taps = h[n * down - i * up + half]
            y[n] = np.dot(taps, xbar[i])
            s1[n] = np.dot(np.abs(taps), np.abs(xbar[i]))
            s2[n] = np.dot(np.abs(taps), xabs[i])
        _REF[key] = (y, s1, s2, P)
    return _REF[key]


def bound(x, up, down, conf):
    y, s1, s2, P = restated(x, up, down, conf)
    C = as_float64(x).shape[1]
    return U * ((P + 3) * s1 + (C if C > 1 else 0) * s2) * (1 + 2.0 ** -10) + P * 2.0 ** -126


def noise(n, seed, channels=1, dtype=np.float32):
    """N(0, 0.3^2), fp32 [n] or [n, channels]; int16: the same times 30000, clipped and rounded"""
    x = 0.3 * np.random.default_rng(9100 + seed).standard_normal((n, channels))
    x = x if channels > 1 else x[:, 0]
    if dtype == np.int16:
        return np.clip(np.round(x * 30000.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


# ---- CPU only: the restatement itself -------------------------------------------------------------------------------------------------
def check_restatement_is_resample_poly():
    from scipy.signal import resample_poly
    for up, down in ((1, 2), (3, 2), (80, 147), (160, 441)):
        for L in (1, 37, 500):
            x = np.random.default_rng(L + up).standard_normal(L)
            h, half, P = design(up, down, **BEST)
            y, s1, _, _ = restated(x.astype(np.float64), up, down, BEST)
            ref = resample_poly(x, up, down, window=h / up)
            assert ref.shape == y.shape == (-(-L * up // down),), (up, down, L, ref.shape, y.shape)
            diff = np.abs(ref - y)
            print('%d / %d, L = %d: restatement against resample_poly within %.3g' % (up, down, L, diff.max()))
            assert (diff <= 1e-12 * s1 + 1e-300).all(), (up, down, L, diff.max())


def restated_f64(x, up, down, conf):
    return restated(np.asarray(x, dtype=np.float64), up, down, conf)[0]


def check_sines():
    """44.1 -> 24 kHz with the default preset: 1 kHz passes within 0.12 % (the 0.01 dB passband), 15 kHz (1.25 of the new
    Nyquist) stays below 1e-5 of its amplitude, both away from the first and last half / up outputs"""
    up, down = 80, 147
    half = design(up, down, **BEST)[1]
    edge = -(-half // up)
    t = np.arange(4410, dtype=np.float64) / 44100.0
    y = restated_f64(np.sin(2 * np.pi * 1000.0 * t), up, down, BEST)
    n = np.arange(len(y))
    inner = slice(edge, len(y) - edge)
    assert len(y) == 2400 and len(y) - 2 * edge > 1000
    err = np.abs(y - np.sin(2 * np.pi * 1000.0 * n / 24000.0))[inner].max()
    print('1 kHz: worst difference from the analytic sine %.3g' % err)
    assert err <= 0.0012
    leak = np.abs(restated_f64(np.sin(2 * np.pi * 15000.0 * t), up, down, BEST))[inner].max()
    print('15 kHz: worst output %.3g' % leak)
    assert leak <= 1e-5


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------
def _solo(rs, x, **kw):
    y, ln = rs.resample(torch.from_numpy(np.asarray(x)[None]), **kw)
    assert y.dtype == torch.float32 and ln.dtype == torch.int64 and ln.tolist() == [rs.out_length(len(x))]
    assert y.shape == (1, max(ln.tolist()[0], 1))
    return y[0].cpu().numpy()[:ln.tolist()[0]]


def _check(tag, got, x, up, down, conf):
    ref = restated(x, up, down, conf)[0]
    lim = bound(x, up, down, conf)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    diff = np.abs(got.astype(np.float64) - ref)
    share = (diff[lim > 0] / lim[lim > 0]).max() if (lim > 0).any() else 0.0
    print('%s: %d outputs, worst difference %.3g, worst share of its bound %.3g' % (tag, len(ref), diff.max() if len(ref) else 0.0, share))
    assert np.isfinite(got).all() and (diff <= lim).all(), '%s: %d of %d beyond their bound, worst %.3g of it' % (
        tag, int((diff > lim).sum()), diff.size, share)


RATIOS = {'1/2': (2, 1, 700), '1/3': (3, 1, 700), '3/2': (2, 3, 700), '147/160': (160, 147, 700), '80/147': (147, 80, 700)}


def check_ratio(dev, name):
    rate_in, rate_out, L = RATIOS[name]
    rs = resampler(dev, rate_in, rate_out, **SMALL)
    assert (rs.up, rs.down) == (rate_out, rate_in)
    x = noise(L, seed=rate_in)
    _check(name, _solo(rs, x), x, rs.up, rs.down, SMALL)


def check_bank_beyond_lds(dev):
    """44.1 -> 16 kHz with the default preset: 160 phases of 373 taps, 233 KB, served in slabs"""
    rs = resampler(dev, 44100, 16000)
    assert (rs.up, rs.down, rs.taps) == (160, 441, 373) and rs.bank().nbytes > 160 * 1024
    x = noise(2000, seed=5)
    _check('160/441 kaiser_best', _solo(rs, x), x, 160, 441, BEST)


def check_default_preset(dev):
    rs = resampler(dev, 44100, 24000)
    assert (rs.up, rs.down, rs.taps, rs.preset) == (80, 147, 249, 'kaiser_best')
    x = noise(4410, seed=6)
    _check('80/147 kaiser_best', _solo(rs, x), x, 80, 147, BEST)
    fast = resampler(dev, 44100, 24000, preset='kaiser_fast')
    assert (fast.zeros, fast.rolloff, fast.beta) == (16, 0.85, 8.555504641634386)


def _length_for(rs, target):
    """the shortest L with out_length(L) == target"""
    L = target * rs.down // rs.up
    while rs.out_length(L) < target:
        L += 1
    assert rs.out_length(L) == target, (target, L)
    return L


def length_cases():
    """name -> (rate_in, rate_out, what): what is a length, or ('out', k): L_out = tile border + k, the tile from the tile query"""
    inv = pow(80, -1, 147)
    return {
        'L1': (2, 3, 1), 'L5 under one phase': (2, 3, 5), 'L1 down': (147, 80, 1), 'L7 down': (3, 1, 7),
        'mod 0': (147, 80, 2 * 147), 'mod 1': (147, 80, 147 + inv), 'mod down-1': (147, 80, 147 + (146 * inv) % 147),
        'tile-1 1/2': (2, 1, ('out', -1)), 'tile 1/2': (2, 1, ('out', 0)), 'tile+1 1/2': (2, 1, ('out', 1)),
        'tile-1 80/147': (147, 80, ('out', -1)), 'tile 80/147': (147, 80, ('out', 0)), 'tile+1 80/147': (147, 80, ('out', 1)),
    }


def check_length(dev, name):
    from msmctts_amd.hip import lib
    rate_in, rate_out, what = length_cases()[name]
    rs = resampler(dev, rate_in, rate_out, **SMALL)
    if isinstance(what, tuple):
        qt = lib.get().msmc_resample_tile(1, rs.up, rs.down, rs.taps)
        assert qt >= 1
        L = _length_for(rs, qt * rs.up + what[1])
    else:
        L = what
        if name.startswith('mod'):
            assert (L * rs.up) % rs.down == {'mod 0': 0, 'mod 1': 1, 'mod down-1': rs.down - 1}[name]
    x = noise(L, seed=L % 1000)
    _check(name, _solo(rs, x), x, rs.up, rs.down, SMALL)


def check_empty_in_batch(dev):
    rs = resampler(dev, 2, 3, **SMALL)
    xs = [noise(300, seed=11), noise(150, seed=12)]
    wide = np.full((3, 300), 7.5, dtype=np.float32)
    wide[0], wide[2, :150] = xs[0], xs[1]
    y, ln = rs.resample(torch.from_numpy(wide), lengths=[300, 0, 150])
    assert ln.tolist() == [450, 0, 225] and y.shape == (3, 450)
    y = y.cpu().numpy()
    assert same_bits(y[1], np.zeros(450, dtype=np.float32)) and same_bits(y[2, 225:], np.zeros(225, dtype=np.float32))
    assert same_bits(y[0], _solo(rs, xs[0])) and same_bits(y[2, :225], _solo(rs, xs[1]))
    # normalised: the empty row stays zero
    z, _ = rs.resample(torch.from_numpy(wide), lengths=[300, 0, 150], norm_db=-7.0)
    assert same_bits(z.cpu().numpy()[1], np.zeros(450, dtype=np.float32))


# ---- channels and types ---------------------------------------------------------------------------------------------------------------
def check_channels(dev, C):
    rs = resampler(dev, 2, 3, **SMALL)
    x = noise(401, seed=20 + C, channels=C)
    got = _solo(rs, x)
    _check('C = %d' % C, got, x, 3, 2, SMALL)
    if C == 1:
        assert same_bits(got, _solo(rs, x.reshape(-1, 1)))                    # [B, L] and [B, L, 1] are the same input


def check_int16(dev):
    rs = resampler(dev, 2, 3, **SMALL)
    for C in (1, 2):
        q = noise(401, seed=30 + C, channels=C, dtype=np.int16)
        f = q.astype(np.float32) / np.float32(32768.0)
        a, b = _solo(rs, q), _solo(rs, f)
        assert same_bits(a, b), C
        _check('int16 C = %d' % C, a, q, 3, 2, SMALL)
    _raises(TypeError, lambda: rs.resample(np.zeros(40, dtype=np.int32)))


def check_same_rate_is_downmix(dev):
    rs = resampler(dev, 16000, 16000)
    assert (rs.up, rs.down, rs.taps, rs.half) == (1, 1, 1, 0)
    x = noise(333, seed=40, channels=2)
    want = (x[:, 0] + x[:, 1]) / np.float32(2.0)
    assert want.dtype == np.float32 and same_bits(_solo(rs, x), want)
    q = noise(333, seed=41, channels=2, dtype=np.int16)
    f = q.astype(np.float32) / np.float32(32768.0)
    assert same_bits(_solo(rs, q), (f[:, 0] + f[:, 1]) / np.float32(2.0))
    mono = noise(50, seed=42)
    assert same_bits(_solo(rs, mono), mono)


# ---- independence -------------------------------------------------------------------------------------------------------------------------
RAGGED = (700, 431, 77)


def _ragged(C=2):
    return [noise(n, seed=50 + i, channels=C) for i, n in enumerate(RAGGED)]


def check_ragged(dev):
    rs = resampler(dev, 147, 80, **SMALL)
    xs = _ragged()
    outs = [rs.out_length(n) for n in RAGGED]
    y, ln = rs.resample(xs)
    assert ln.tolist() == outs and y.shape == (3, max(outs))
    y = y.cpu().numpy()
    solo = [_solo(rs, x) for x in xs]
    for i in range(3):
        assert same_bits(y[i, :outs[i]], solo[i]), i
        assert same_bits(y[i, outs[i]:], np.zeros(max(outs) - outs[i], dtype=np.float32)), i
    # the padding poisoned, in a wider batch: nothing behind an utterance's own length is read
    for poison in (np.nan, 1e30, -1e30):
        wide = np.full((3, max(RAGGED) + 211, 2), poison, dtype=np.float32)
        for i, x in enumerate(xs):
            wide[i, :len(x)] = x
        z, zl = rs.resample(torch.from_numpy(wide), lengths=list(RAGGED))
        z = z.cpu().numpy()
        assert zl.tolist() == outs and z.shape == y.shape and same_bits(z, y), poison
        zn, _ = rs.resample(torch.from_numpy(wide), lengths=list(RAGGED), norm_db=-7.0)
        yn, _ = rs.resample(xs, norm_db=-7.0)
        assert same_bits(zn.cpu().numpy(), yn.cpu().numpy()), poison


def check_repeat(dev):
    rs = resampler(dev, 147, 80, **SMALL)
    xs = _ragged()
    a, b = rs.resample(xs, norm_db=-7.0), rs.resample(xs, norm_db=-7.0)
    assert all(same_bits(p.cpu().numpy(), q.cpu().numpy()) for p, q in zip(a, b))


def check_wider_row(dev):
    rs = resampler(dev, 2, 3, **SMALL)
    x = noise(300, seed=60)
    solo = _solo(rs, x)
    for extra in (1, 57, 1200):
        wide = np.zeros((1, 300 + extra), dtype=np.float32)
        wide[0, :300] = x
        wide[0, 300:] = 3.0
        y, ln = rs.resample(torch.from_numpy(wide), lengths=[300])
        assert ln.tolist() == [450] and same_bits(y[0].cpu().numpy(), solo), extra


# ---- normalisation ------------------------------------------------------------------------------------------------------------------------
def check_normalisation(dev):
    from msmctts_amd.hip import lib
    from msmctts_amd.hip.resample import prepare_waveforms
    rs = resampler(dev, 147, 80, **SMALL)
    xs = _ragged()
    outs = [rs.out_length(n) for n in RAGGED]
    y = rs.resample(xs)[0].cpu().numpy()
    z, pk, ln = rs.resample(xs, norm_db=-7.0, peak=True)
    z, pk = z.cpu().numpy(), pk.cpu().numpy()
    assert float(TARGET) == float(np.float32(0.44668359215096315))
    for i in range(3):
        peak = np.abs(y[i, :outs[i]]).max()
        gain = TARGET / peak
        assert peak.dtype == gain.dtype == np.float32
        assert same_bits(pk[i], peak) and same_bits(z[i, :outs[i]], y[i, :outs[i]] * gain), i
        assert same_bits(z[i, outs[i]:], np.zeros(max(outs) - outs[i], dtype=np.float32))
        got = np.abs(z[i]).max()
        print('utterance %d: peak %.9g -> %.9g, %.3g ulp from the target' % (i, peak, got, (float(got) - float(TARGET)) / np.spacing(TARGET)))
        assert abs(float(got) - float(TARGET)) <= float(np.spacing(TARGET)), (i, got)
    # another level; prepare_waveforms is resample + normalise at -7 by default
    z3 = rs.resample(xs, norm_db=-3.0)[0].cpu().numpy()
    t3 = np.float32(10.0 ** (-3.0 / 20.0))
    assert same_bits(z3[0], y[0] * (t3 / np.abs(y[0]).max()))
    p, pl = prepare_waveforms(xs, None, 147, 80, device=dev, **SMALL)
    assert pl.tolist() == outs and same_bits(p.cpu().numpy(), z)
    p2, _ = prepare_waveforms(xs, None, 147, 80, resampler=rs)
    assert same_bits(p2.cpu().numpy(), z)
    _raises(ValueError, lambda: prepare_waveforms(xs, None, 2, 3, resampler=rs))
    # norm_db=None: y untouched, one launch; with a level: two
    h = lib.get()
    for norm, launches in ((None, 1), (-7.0, 2)):
        h.msmc_prof_enable(1)
        try:
            q = prepare_waveforms(xs, None, 147, 80, norm_db=norm, resampler=rs)[0]
            if dev != 'cpu':
                torch.cuda.synchronize()
            assert h.msmc_prof_count() == launches
        finally:
            h.msmc_prof_enable(0)
        assert same_bits(q.cpu().numpy(), y if norm is None else z)
    # silence stays zero, and finite
    quiet = [np.zeros(200, dtype=np.float32), xs[2][:, 0].copy()]
    s, sp, _ = rs.resample(quiet, norm_db=-7.0, peak=True)
    s = s.cpu().numpy()
    assert same_bits(s[0], np.zeros_like(s[0])) and sp.cpu().numpy()[0] == 0.0 and np.isfinite(s).all() and np.abs(s[1]).max() > 0.4


def check_chain(dev):
    """what prepare_waveforms returns is what the extractors take"""
    from msmctts_amd.hip.resample import prepare_waveforms
    xs = [noise(2400, seed=70, channels=2, dtype=np.int16), noise(1500, seed=71, channels=2, dtype=np.int16)]
    y, ln = prepare_waveforms(xs, None, 48000, 16000, device=dev, **SMALL)
    assert ln.tolist() == [800, 500]
    fex = fcases.extractor(dev, **fcases.SMALL)
    mel, en, fl = fex.extract(y, lengths=ln)
    assert fl.tolist() == [33, 21] and mel.shape == (2, 33, 20)
    solo = fex.extract(y[1, :500].cpu().numpy())[0].cpu().numpy()
    assert same_bits(mel[1, :21].cpu().numpy(), solo[0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw(dev, up=3, down=2, half=14, P=None, L=100, Lout=None, C=1, B=1, dtype=0, null=None):
    """msmc_resample on sentinel-filled outputs -> (rc, outputs untouched?, launches logged)"""
    from msmctts_amd.hip import lib
    h = lib.get()
    P = -(-(2 * half + 1) // max(up, 1)) if P is None else P
    Lout = -(-L * max(up, 1) // max(down, 1)) if Lout is None else Lout
    nb = max(B, 1) if B < 1000 else 1
    x = torch.zeros((nb, max(L, 1), max(C, 1)), dtype=torch.int16 if dtype == 1 else torch.float32).to(dev)
    ln = torch.full((nb,), max(L, 0), dtype=torch.int32).to(dev)
    bank = torch.zeros((min(max(up, 1), 2048), min(max(P, 1), 8192)), dtype=torch.float32).to(dev)
    y = torch.full((nb, max(Lout, 1) + 64), -7.25, dtype=torch.float32).to(dev)
    part = torch.full((nb, 4096), -7.25, dtype=torch.float32).to(dev)
    arg = {'x': x, 'length': ln, 'bank': bank, 'y': y, 'partials': part}
    p = {k: (None if null == k else lib.ptr(t)) for k, t in arg.items()}
    h.msmc_prof_enable(1)
    try:
        rc = h.msmc_resample(p['x'], dtype, p['length'], p['bank'], p['y'], p['partials'], B, L, C, Lout, up, down, P, half,
                             lib.stream(x))
        if dev != 'cpu':
            torch.cuda.synchronize()
        launches = h.msmc_prof_count()
    finally:
        h.msmc_prof_enable(0)
    return rc, bool((y == -7.25).all() and (part == -7.25).all()), launches


def _raw_scale(dev, B=1, Lout=100, nparts=3, target=0.5, null=None):
    from msmctts_amd.hip import lib
    h = lib.get()
    y = torch.full((max(B, 1), max(Lout, 1)), -7.25, dtype=torch.float32).to(dev)
    part = torch.full((max(B, 1), max(nparts, 1)), 2.0, dtype=torch.float32).to(dev)
    lo = torch.full((max(B, 1),), Lout, dtype=torch.int32).to(dev)
    pk = torch.full((max(B, 1),), -7.25, dtype=torch.float32).to(dev)
    p = {k: (None if null == k else lib.ptr(t)) for k, t in {'y': y, 'partials': part, 'length': lo, 'peak': pk}.items()}
    h.msmc_prof_enable(1)
    try:
        rc = h.msmc_peak_scale(p['y'], p['partials'], p['length'], p['peak'], B, Lout, nparts, target, lib.stream(y))
        if dev != 'cpu':
            torch.cuda.synchronize()
        launches = h.msmc_prof_count()
    finally:
        h.msmc_prof_enable(0)
    return rc, bool((y == -7.25).all() and (pk == -7.25).all()), launches, y


def check_refusals(dev):
    from msmctts_amd.hip import lib
    assert _raw(dev) == (0, False, 1)                                          # the accepted call launches once and writes
    assert _raw(dev, dtype=1, C=8) == (0, False, 1)
    assert _raw(dev, up=1024, down=1023, half=0)[0] == 0 and _raw(dev, up=1, down=1024, half=511)[0] == 0      # at the bounds
    for kw in (dict(null='x'), dict(null='length'), dict(null='bank'), dict(null='y'), dict(null='partials'),
               dict(C=0), dict(C=9), dict(B=0), dict(B=65536), dict(dtype=2), dict(dtype=-1),
               dict(up=2, down=4, half=20), dict(up=6, down=4, half=20), dict(up=0), dict(down=0), dict(up=-3),
               dict(up=1025, down=1, half=0), dict(up=1, down=1025, half=100), dict(up=1, down=2, half=512),    # P = 1025
               dict(P=9), dict(P=11), dict(half=-1, P=1), dict(L=0),
               dict(L=100, Lout=149), dict(L=100, Lout=0), dict(L=101, Lout=151)):
        assert _raw(dev, **kw) == (E_SHAPE, True, 0), kw
    rc, untouched, launches, y = _raw_scale(dev)
    assert (rc, untouched, launches) == (0, False, 1) and same_bits(y.cpu().numpy(), np.full((1, 100), -7.25 * 0.25, dtype=np.float32))
    assert _raw_scale(dev, null='peak')[0] == 0
    for kw in (dict(null='y'), dict(null='partials'), dict(null='length'), dict(B=0), dict(B=65536), dict(Lout=0), dict(nparts=0),
               dict(target=0.0), dict(target=-0.5), dict(target=float('nan'))):
        assert _raw_scale(dev, **kw)[:3] == (E_SHAPE, True, 0), kw
    # the tile query refuses what the launcher refuses
    h = lib.get()
    assert h.msmc_resample_tile(0, 1025, 1, 1) == 0 and h.msmc_resample_tile(1, 1, 2, 1025) == 0
    assert h.msmc_resample_parts(100, 1025, 1, 1) == 0 and h.msmc_resample_parts(0, 3, 2, 10) == 0
    # the host layer: ValueError with the offending value, before any launch
    h.msmc_prof_enable(1)
    try:
        assert '1025' in str(_raises(ValueError, lambda: resampler(dev, 1025, 1024)))
        assert '44101' in str(_raises(ValueError, lambda: resampler(dev, 44101, 16000)))         # coprime rates: far beyond the bounds
        assert 'kaiser_worst' in str(_raises(ValueError, lambda: resampler(dev, 2, 3, preset='kaiser_worst')))
        rs = resampler(dev, 2, 3, **SMALL)
        assert '9 channels' in str(_raises(ValueError, lambda: rs.resample(np.zeros((1, 40, 9), dtype=np.float32))))
        _raises(ValueError, lambda: rs.resample(torch.zeros(2, 400), lengths=[400]))
        _raises(ValueError, lambda: rs.resample(torch.zeros(1, 400), lengths=[401]))
        _raises(ValueError, lambda: rs.resample([np.zeros(40, dtype=np.float32), np.zeros((40, 2), dtype=np.float32)]))
        _raises(ValueError, lambda: rs.resample([]))
        assert h.msmc_prof_count() == 0
    finally:
        h.msmc_prof_enable(0)


# ---- host -----------------------------------------------------------------------------------------------------------------------------
def check_out_length():
    from msmctts_amd.hip.resample import Resampler, polyphase_bank
    rs = Resampler(44100, 24000)
    L = 2 ** 31 - 1
    want = math.ceil(Fraction(L * 80, 147))
    assert rs.out_length(L) == want == 1168698584 and isinstance(rs.out_length(L), int)
    assert [rs.out_length(n) for n in (0, 1, 2, 147, 148)] == [0, 1, 2, 80, 81]
    # the bank is the prototype filter, row p holding output phase p
    for up, down in ((3, 2), (80, 147), (1, 3)):
        bank, half = polyphase_bank(up, down, **SMALL)
        h, half_, P = design(up, down, **SMALL)
        assert half == half_ and bank.shape == (up, P) and bank.dtype == np.float32
        padded = np.zeros(up * P)
        padded[:2 * half + 1] = h
        for p in range(up):
            assert same_bits(bank[p], padded[(p * down + half) % up::up].astype(np.float32)), (up, down, p)


def check_host_tensors_need_the_interpreter():
    from msmctts_amd.hip import lib
    saved = lib._host_pointers_ok
    lib._host_pointers_ok = False
    try:
        err = _raises(RuntimeError, lambda: resampler('cpu', 2, 3, **SMALL).resample(noise(100, seed=1)))
        assert 'GPU only' in str(err)
    finally:
        lib._host_pointers_ok = saved


def write_wav(path, pcm, rate):
    """int16 [L] or [L, C] -> 16-bit PCM"""
    pcm = np.asarray(pcm, dtype='<i2')
    with wave.open(path, 'wb') as w:
        w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def check_read_wav_channels(tmp_path):
    from msmctts_amd.datasets import readers
    q = noise(500, seed=80, channels=2, dtype=np.int16)
    path = str(tmp_path / 'stereo.wav')
    write_wav(path, q, 48000)
    x, rate = readers.read_wav_channels(path)
    assert rate == 48000 and x.dtype == np.int16 and same_bits(x, q)
    first, rate = readers.read_wav(path)
    assert rate == 48000 and same_bits(first, (q[:, :1].astype(np.float32) / 32768.0))
    from scipy.io import wavfile
    f = noise(300, seed=81, channels=2)
    wavfile.write(str(tmp_path / 'float.wav'), 22050, f)
    x, rate = readers.read_wav_channels(str(tmp_path / 'float.wav'))
    assert rate == 22050 and x.dtype == np.float32 and same_bits(x, f)


# ---- the tools -----------------------------------------------------------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _corpus(tmp_path):
    src = str(tmp_path / 'wav')
    os.makedirs(src)
    pcm = {'a_stereo48': (noise(2400, seed=90, channels=2, dtype=np.int16), 48000), 'b_mono441': (noise(2205, seed=91, dtype=np.int16), 44100)}
    for uid, (q, rate) in pcm.items():
        write_wav(os.path.join(src, uid + '.wav'), q, rate)
    return src, pcm


def check_prepare_tool(dev, tmp_path):
    import io
    from msmctts_amd.datasets import readers
    tool = _tool('prepare_wavs')
    src, pcm = _corpus(tmp_path)
    dst, log = str(tmp_path / 'out'), io.StringIO()
    assert tool.prepare_dir(src, dst, 24000, device=dev, out=log)[0] == 2 and 'audio-seconds/s' in log.getvalue()
    assert sorted(os.listdir(dst)) == ['a_stereo48.wav', 'b_mono441.wav']
    want = int(round(32768 * 10.0 ** (-7.0 / 20.0)))
    for uid, (q, rate) in pcm.items():
        x, r = readers.read_wav_channels(os.path.join(dst, uid + '.wav'))
        assert r == 24000 and x.dtype == np.int16 and x.shape == (1200, 1), (uid, x.shape)
        assert abs(int(np.abs(x.astype(np.int32)).max()) - want) <= 1, (uid, np.abs(x.astype(np.int32)).max(), want)
        y = resampler(dev, rate, 24000).resample([q], norm_db=-7.0)[0][0].cpu().numpy()
        assert same_bits(x[:, 0], tool.to_pcm16(y).astype(np.int16)), uid
    assert same_bits(tool.to_pcm16([0.5 / 32768, 1.5 / 32768, -2.5 / 32768, 1.0, -1.5]), np.array([0, 2, -2, 32767, -32768], dtype='<i2'))
    # --float and --no-norm
    flt = str(tmp_path / 'float')
    tool.prepare_dir(src, flt, 24000, norm_db=None, as_float=True, device=dev, out=log)
    x, r = readers.read_wav_channels(os.path.join(flt, 'a_stereo48.wav'))
    y = resampler(dev, 48000, 24000).resample([pcm['a_stereo48'][0]])[0][0].cpu().numpy()
    assert r == 24000 and x.dtype == np.float32 and same_bits(x[:, 0], y)


def check_extract_tool(dev, tmp_path):
    import io
    from msmctts_amd.hip.resample import prepare_waveforms
    tool = _tool('extract_features')
    src, pcm = _corpus(tmp_path)
    os.remove(os.path.join(src, 'b_mono441.wav'))
    fex = fcases.extractor(dev, **fcases.SMALL)
    assert fex.sample_rate == 16000
    log = io.StringIO()
    err = _raises(ValueError, lambda: tool.extract_dir(fex, src, str(tmp_path / 'refused'), out=log))
    assert 'sample rate 48000, the features are defined at 16000 (resample it first)' in str(err)
    assert not os.path.exists(str(tmp_path / 'refused'))
    dst = str(tmp_path / 'out')
    assert tool.extract_dir(fex, src, dst, energy=True, out=log, resample=True)[0] == 1
    y, ln = prepare_waveforms([pcm['a_stereo48'][0]], None, 48000, 16000, device=dev)
    assert ln.tolist() == [800]
    mel, en, _ = fex.extract(y, lengths=ln)
    assert same_bits(np.load(os.path.join(dst, 'mel', 'a_stereo48.npy')), mel[0].cpu().numpy())
    assert same_bits(np.load(os.path.join(dst, 'energy', 'a_stereo48.npy')), en[0].cpu().numpy())
    other = str(tmp_path / 'other')
    tool.extract_dir(fex, src, other, out=log, resample=True, norm_db=None)
    y, ln = prepare_waveforms([pcm['a_stereo48'][0]], None, 48000, 16000, norm_db=None, device=dev)
    assert same_bits(np.load(os.path.join(other, 'mel', 'a_stereo48.npy')), fex.extract(y, lengths=ln)[0][0].cpu().numpy())


# ---- presence ---------------------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    for name in ('msmc_resample', 'msmc_peak_scale', 'msmc_resample_tile', 'msmc_resample_parts'):
        assert name in lib.exported_symbols() and hasattr(lib.get(), name), name
    from msmctts_amd.hip.resample import Resampler, prepare_waveforms, PRESETS
    from msmctts_amd.networks.vqgantts import msmc_vqgan_emb
    assert msmc_vqgan_emb.Resampler is Resampler and msmc_vqgan_emb.prepare_waveforms is prepare_waveforms
    assert hasattr(msmc_vqgan_emb, 'FeatureExtractor') and hasattr(msmc_vqgan_emb, 'PitchExtractor')
    assert PRESETS['kaiser_best'] == BEST and PRESETS['kaiser_fast'] == dict(zeros=16, rolloff=0.85, beta=8.555504641634386)
    from msmctts_amd.datasets import readers
    assert hasattr(readers, 'read_wav_channels')
    # the pairs that must work with the default preset
    h = lib.get()
    for up, down in ((1, 2), (1, 3), (3, 2), (80, 147), (160, 441), (160, 147), (147, 160)):
        rs = Resampler(down, up)
        assert (rs.up, rs.down) == (up, down)
        assert h.msmc_resample_tile(0, up, down, rs.taps) >= 1 and h.msmc_resample_tile(1, up, down, rs.taps) >= 1, (up, down)
        assert h.msmc_resample_parts(240000, up, down, rs.taps) >= 1
