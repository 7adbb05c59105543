"""Shared cases of the F0 tracker: csrc/pitch.hip (msmc_pitch_yin), its host side (msmctts_amd/hip/pitch.py ``PitchExtractor``) and
the ``--pitch`` path of tools/extract_features.py.  tests/test_pitch_emu.py runs them on the kernel interpreter,
tests/test_gpu_pitch.py on the GPU.

Reference.  ``restated`` is YIN steps 1-5 as csrc/pitch.hip defines them, in float64 numpy: frames of span = W + tau_max + 1
samples starting at t hop - span // 2, reflected at 0 and at the utterance's length; d(tau) = sum_{j < W} (x[j] - x[j + tau])^2;
d'(tau) = d(tau) tau / S(tau), S the running sum of d (1 at tau = 0 and where S = 0); the first lag of [tau_min, tau_max] under the
threshold, walked up while d' falls; the parabola through d'(lag - 1 .. lag + 1); ln(sr / (lag + delta)).  ``decide`` holds steps
3-5 for any dtype: in float64 for the reference, in fp32 in the kernel's operation order for test 2.

Bound on d' (test 1; every element, none left out).  With u = 2^-24: a term (x[j] - x[j + tau])^2 is a rounded difference squared
and rounded, a relative error of about 3 u of a non-negative term, and the W terms are summed in sequence into partial sums
bounded by d itself, so the error of d has the scale u sqrt(W) d (the random-walk growth of W roundings; the 3 u of the terms are
below it for W >= 9).  S(tau) inherits the errors of its d(k), which add up to u sqrt(W) S at most, and adds tau roundings of
partial sums bounded by S: u (sqrt(W) + sqrt(tau)) S.  Through the quotient d tau / S, with one rounding for the product and one
for the division:
    unit(tau) = 2^-24 d'(tau) (2 sqrt(W) + sqrt(tau) + 2)
It is relative, because every sum here is over non-negative terms: where d is exactly 0 (the period of a periodic frame) the
kernel has to return exactly 0, and where S = 0 (silence) exactly 1.  The bound is C_DP unit with C_DP MEASURED, never on the
kernel: ``fp32_chain`` evaluates d, S and d' in fp32 numpy in the kernel's documented order (``cumsum`` is sequential) and
``measured_c`` takes 8 x the worst ratio of its difference from ``restated`` to the unit over ALL inputs of the kernel tests
(``all_inputs``).  Observed where this was written: worst ratio 0.4988 (the real geometry; 0.31 .. 0.43 on the small one) ->
C_DP = 3.99 (the table: profiles/pitch.md).  The kernel sums in the order of the fp32 chain, so it used 0.125 of the bound on the
interpreter; the GPU's figure is in the profile.

Decision (test 3).  A frame is compared when every comparison the float64 decision makes is clear of the bound: each
d'(tau) against the threshold, from tau_min up to the crossing (up to tau_max on an unvoiced frame), by more than C_DP unit(tau),
and each step of the walk, the failing one included, d'(tau + 1) against d'(tau) by more than C_DP (unit(tau) + unit(tau + 1)).
On such a frame no admissible error changes the lag or the voicing.  The others are left out, at most 2 % of the frames of
``all_inputs`` together (asserted).

Bound on ln f0 on compared frames.  With errors ea, eb, ec <= C_DP unit on a, b, c = d'(lag - 1), d'(lag), d'(lag + 1) and
E = ea + 2 eb + ec: the numerator a - c moves by at most ea + ec <= E, the denominator D = a - 2 b + c by at most E, so for D > E
    |delta' - delta| <= (E / 2 + |delta| E) / (D - E) = E (1/2 + |delta|) / (D - E),
and 2 at most in any case (delta is clipped to [-1, 1]; the clip does not expand).  The fp32 evaluation of delta adds four
roundings (a - c, the two of D, the division; the halving is exact): 4 u (1/2 + |delta|) D / (D - E) at most, taken as
8 u (1/2 + |delta|).  Then ln f0 = ln sr - ln(lag + delta) moves by at most dd / (lag + delta - dd), plus the roundings of the sum,
the division (2 u, relative to f0, so absolute on its logarithm) and logf (2 ulp of ln f0, each at most 2^-23 |ln f0|): together
below 2^-21 max(1, |ln f0|), which is what ``lnf0_bound`` adds.  Observed: the kernel's track within 3.1e-7 of float64 on the
interpreter and 6.2e-7 on an MI355X (the device's logf), a quarter of its bound at most.
Silence, zero rows, the ragged batch against solo runs, the repeat and the decision on the kernel's own d' are compared BIT FOR BIT.
"""
import os

import numpy as np
import torch

import _featurecases as fcases
from _featurecases import _raises, _write_wav, same_bits

E_SHAPE = -2
ROOT = fcases.ROOT
U = 2.0 ** -24
FRAME_TILE = 32

DEFAULTS = dict(sample_rate=16000, frame_length_ms=50, frame_shift_ms=12.5, fmin=60, fmax=500, threshold=0.15)
# the small geometry: tau 8 .. 40 (one lag block of 64, partly filled), W = 64, span = 105 (odd), hop = 25
SMALL = dict(DEFAULTS, sample_rate=2000, win_length=64, hop_length=25, fmin=50, fmax=250)


def extractor(dev, **kw):
    from msmctts_amd.hip.pitch import PitchExtractor
    return PitchExtractor(device=dev, **kw)


def geometry(conf):
    """(sr, W, hop, tau_min, tau_max, span)"""
    sr = conf['sample_rate']
    W = conf.get('win_length') or int(conf['frame_length_ms'] / 1000 * sr)
    hop = conf.get('hop_length') or int(conf['frame_shift_ms'] / 1000 * sr)
    tau_min, tau_max = int(sr // conf['fmax']), int(sr // conf['fmin'])
    return sr, W, hop, tau_min, tau_max, W + tau_max + 1


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def frames(y, conf):
    """[T, span] in y's dtype: x_t[j] = y[reflect(t hop - span // 2 + j)]"""
    sr, W, hop, tau_min, tau_max, span = geometry(conf)
    y = np.asarray(y)
    L = len(y)
    assert L > span // 2
    idx = hop * np.arange(1 + L // hop)[:, None] - span // 2 + np.arange(span)[None, :]
    period = 2 * (L - 1)
    idx = np.abs(idx) % period                           # numpy's 'reflect', whatever the number of reflections
    idx = np.where(idx >= L, period - idx, idx)
    return y[idx]


def cmnd_of(y, conf, dt):
    """(d', unit-free) [T, tau_max + 2] in ``dt``: sequential sums (``cumsum``), (d * tau) / S"""
    sr, W, hop, tau_min, tau_max, span = geometry(conf)
    x = frames(np.asarray(y, dtype=np.float32), conf).astype(dt)
    d = np.zeros((x.shape[0], tau_max + 2), dtype=dt)
    for tau in range(1, tau_max + 2):
        df = x[:, :W] - x[:, tau:tau + W]
        d[:, tau] = np.cumsum(df * df, axis=1, dtype=dt)[:, -1]
    S = np.cumsum(d[:, 1:], axis=1, dtype=dt)
    tau = np.arange(1, tau_max + 2).astype(dt)[None, :]
    dp = np.ones_like(d)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = (d[:, 1:] * tau) / S
    dp[:, 1:] = np.where(S > 0, q, dt(1))
    assert dp.dtype == dt
    return dp


def decide(dp, conf, dt, log=True):
    """steps 3-5 on d' rows [T, tau_max + 2], every operation in ``dt`` and in the order of csrc/pitch.hip ->
    (lag [T] int, 0 = unvoiced; aperiodicity [T]; pitch [T]; delta [T]; D [T], the parabola's denominator)"""
    sr, W, hop, tau_min, tau_max, span = geometry(conf)
    dp = np.asarray(dp, dtype=dt)
    T = dp.shape[0]
    thr = dt(np.float32(conf['threshold']))              # the launcher takes the threshold as fp32
    lag, ap, f0 = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=dt), np.zeros(T, dtype=dt)
    delta, den = np.zeros(T, dtype=dt), np.zeros(T, dtype=dt)
    for t in range(T):
        r = dp[t]
        under = np.nonzero(r[tau_min:tau_max + 1] < thr)[0]
        if under.size == 0:
            ap[t] = r[tau_min:tau_max + 1].min()
            continue
        k = tau_min + int(under[0])
        while k + 1 <= tau_max and r[k + 1] < r[k]:
            k += 1
        a, b, c = r[k - 1], r[k], r[k + 1]
        num = a - c
        D = (a - (b + b)) + c
        dl = dt(0)
        if D > 0:
            dl = dt(0.5) * (num / D)
            dl = min(max(dl, dt(-1)), dt(1))
        f = dt(sr) / (dt(k) + dl)
        lag[t], ap[t], delta[t], den[t] = k, b, dl, D
        f0[t] = np.log(f) if log else f
    assert ap.dtype == dt and f0.dtype == dt
    return lag, ap, f0, delta, den


_REF = {}


def restated(y, conf):
    """float64: {'dp': d' [T, tau_max + 2], 'lag', 'aper', 'pitch', 'delta', 'den'} (computed once per input)"""
    key = (np.asarray(y, dtype=np.float32).tobytes(), tuple(sorted(conf.items())))
    if key not in _REF:
        dp = cmnd_of(y, conf, np.float64)
        lag, ap, f0, delta, den = decide(dp, conf, np.float64)
        _REF[key] = {'dp': dp, 'lag': lag, 'aper': ap, 'pitch': f0, 'delta': delta, 'den': den}
    return _REF[key]


def unit(dp, conf):
    """the bound on d' at C_DP = 1, [T, tau_max + 2] (0 at tau = 0, which is the constant 1)"""
    sr, W, hop, tau_min, tau_max, span = geometry(conf)
    tau = np.arange(tau_max + 2, dtype=np.float64)[None, :]
    un = U * np.abs(dp) * (2 * np.sqrt(W) + np.sqrt(tau) + 2)
    un[:, 0] = 0.0
    return un


def clear_frames(ref, conf, c):
    """[T] bool: every comparison of the float64 decision clears the bound c * unit"""
    sr, W, hop, tau_min, tau_max, span = geometry(conf)
    dp, bound = ref['dp'], c * unit(ref['dp'], conf)
    thr = float(np.float32(conf['threshold']))
    ok = np.ones(dp.shape[0], dtype=bool)
    for t in range(dp.shape[0]):
        k = int(ref['lag'][t])
        first = tau_max
        if k:
            first = tau_min + int(np.nonzero(dp[t, tau_min:tau_max + 1] < thr)[0][0])
        sl = slice(tau_min, first + 1)
        ok[t] = (np.abs(dp[t, sl] - thr) > bound[t, sl]).all()
        if k:
            for q in range(first, min(k, tau_max - 1) + 1):          # the steps q -> q + 1 the walk compared (the last one fails)
                ok[t] &= abs(dp[t, q + 1] - dp[t, q]) > bound[t, q] + bound[t, q + 1]
    return ok


def lnf0_bound(ref, conf, c):
    """[T]: the bound on |ln f0 - float64| on voiced frames whose lag is the reference's (derivation: the module docstring)"""
    bound = c * unit(ref['dp'], conf)
    out = np.zeros(len(ref['lag']))
    for t, k in enumerate(ref['lag']):
        if not k:
            continue
        E = bound[t, k - 1] + 2 * bound[t, k] + bound[t, k + 1]
        D, dl = ref['den'][t], abs(ref['delta'][t])
        dd = min(2.0, E * (0.5 + dl) / (D - E)) if D > E else 2.0
        dd += 8 * U * (0.5 + dl)
        out[t] = dd / (k + ref['delta'][t] - dd) + 2.0 ** -21 * max(1.0, abs(ref['pitch'][t]))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def tone(n, sr, f0, seed, noise=0.002, gap=None, gap_noise=0.3):
    """three harmonics (1, 1/2, 1/3) of f0 (a number, or the instantaneous frequency per sample) plus N(0, noise^2); ``gap`` =
    (first, last): that stretch is N(0, gap_noise^2) alone.  fp32"""
    rng = np.random.default_rng(7300 + seed)
    ph = 2.0 * np.pi * np.cumsum(np.broadcast_to(np.asarray(f0, dtype=np.float64), (n,))) / sr
    y = 0.3 * (np.sin(ph) + np.sin(2 * ph) / 2 + np.sin(3 * ph) / 3) + noise * rng.standard_normal(n)
    if gap is not None:
        y[gap[0]:gap[1]] = gap_noise * rng.standard_normal(gap[1] - gap[0])
    return y.astype(np.float32)


# name: (samples, F0).  span // 2 + 1 = 53 is the shortest accepted length (every frame reflects at both ends); 106 / 107: both
# reflections inside one frame; 431: a last tile of ... frames; 790: T = 32, exactly one tile; 825: T = 34, two tiles
LENGTHS = {
    'shortest L53': (53, 200.0),
    'L106': (106, 87.0),
    'L107': (107, 123.4),
    'L400': (400, 200.0),
    'L431': (431, 87.0),
    'T32 one tile L790': (790, 123.4),
    'T34 two tiles L825': (825, 87.0),
}
GAP = (825, 123.4, (300, 520))                           # tone, pure noise, tone
RAGGED = (825, 431, 106)


def small_wave(name):
    n, f0 = LENGTHS[name]
    return tone(n, 2000, f0, seed=n)


def gap_wave():
    return tone(GAP[0], 2000, GAP[1], seed=1, gap=GAP[2])


def ragged_waves():
    return [small_wave('T34 two tiles L825'), small_wave('L431'), small_wave('L106')]


def real_wave():
    """one second at 16 kHz: harmonics of 180 Hz with 20 % vibrato at 2.5 Hz, noise alone from 0.4 s to 0.6 s -> (y, f0 per sample)"""
    n = 16000
    f0 = 180.0 * (1.0 + 0.2 * np.sin(2.0 * np.pi * 2.5 * np.arange(n) / 16000.0))
    return tone(n, 16000, f0, seed=2, gap=(6400, 9600)), f0


def square_wave(n=400):
    return np.where((np.arange(n) % 16) < 8, 0.25, -0.25).astype(np.float32)


def int16_wave():
    return np.round(small_wave('L431') * 30000.0).astype(np.int16)


def all_inputs():
    """every (name, waveform, configuration) a toleranced kernel test of this file uses: what ``measured_c`` and the 2 % cap cover"""
    out = [(name, small_wave(name), SMALL) for name in LENGTHS]
    out += [('noise in the middle', gap_wave(), SMALL), ('int16', int16_wave().astype(np.float32) / np.float32(32768.0), SMALL)]
    out += [('real geometry', real_wave()[0], DEFAULTS)]
    return out


_C = {}


def measured_c(verbose=True):
    """C_DP = 8 x the worst ratio of |fp32 numpy chain - float64 restatement| of d' to ``unit`` over ``all_inputs``"""
    if not _C:
        worst = 0.0
        for name, y, conf in all_inputs():
            ref = restated(y, conf)
            d32 = cmnd_of(y, conf, np.float32)
            un = unit(ref['dp'], conf)
            diff = np.abs(d32.astype(np.float64) - ref['dp'])
            assert (diff[un == 0] == 0).all()
            ratio = (diff[un > 0] / un[un > 0]).max()
            lag32 = decide(d32, conf, np.float32)[0]
            if verbose:
                print('%-20s fp32 numpy chain against float64: d\' within %.3g, worst ratio to the unit %.4g; %d of %d frames '
                      'change lag or voicing' % (name, diff.max(), ratio, int((lag32 != ref['lag']).sum()), len(lag32)))
            worst = max(worst, ratio)
        _C['c'] = 8 * worst
        if verbose:
            print('worst ratio %.4g -> C_DP = %.4g' % (worst, 8 * worst))
    return _C['c']


# ---- the float64 tracker itself (no kernel) -----------------------------------------------------------------------------------------------
def check_restatement_tracks_f0():
    """facts about the definition: within 1.5 % of the F0 of the steady tones and 2.4 % under vibrato on the frames that lie
    inside the signal, the noise stretches unvoiced, and an fp32 evaluation changes no lag"""
    for name in LENGTHS:
        n, f0 = LENGTHS[name]
        ref = restated(small_wave(name), SMALL)
        inside = [t for t in range(1 + n // 25) if t * 25 - 52 >= 0 and t * 25 + 53 <= n]
        for t in inside:
            assert ref['lag'][t] and abs(np.exp(ref['pitch'][t]) / f0 - 1) < 0.015, (name, t, np.exp(ref['pitch'][t]))
    ref = restated(gap_wave(), SMALL)
    quiet = [t for t in range(34) if t * 25 - 52 >= GAP[2][0] and t * 25 + 53 <= GAP[2][1]]
    assert len(quiet) >= 4 and not ref['lag'][quiet].any() and ref['lag'][3:11].all()
    y, f0 = real_wave()
    ref = restated(y, DEFAULTS)
    for t in range(81):
        lo, hi = t * 200 - 533, t * 200 + 534
        if lo >= 6400 and hi <= 9600:
            assert not ref['lag'][t], t
        elif lo >= 0 and (hi <= 6400 or lo >= 9600) and hi <= 16000:
            # the lag is measured between the window's two ends: compare with the mean F0 over the frame's W + lag samples
            want = f0[lo:lo + 800 + int(ref['lag'][t])].mean()
            assert ref['lag'][t] and abs(np.exp(ref['pitch'][t]) / want - 1) < 0.024, (t, np.exp(ref['pitch'][t]), want)


# ---- 1: d' against float64 ------------------------------------------------------------------------------------------------------------------
def _run(ex, y, **kw):
    """solo run with every extra -> numpy (pitch [T], voiced [T], aperiodicity [T], cmnd [T, tau_max + 2])"""
    f0, vo, ap, cm, length = ex.extract(torch.from_numpy(np.asarray(y)), voiced=True, aperiodicity=True, cmnd=True, **kw)
    assert f0.shape[0] == 1 and length.tolist() == [1 + len(y) // ex.hop]
    assert f0.dtype == ap.dtype == cm.dtype == torch.float32 and vo.dtype == torch.uint8
    return f0[0].cpu().numpy(), vo[0].cpu().numpy(), ap[0].cpu().numpy(), cm[0].cpu().numpy()


def _within_ulp(a, b, n):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b)))).all()


def _check(tag, out, y, conf, stats=None):
    """tests 1, 2 and 3 on one run"""
    f0, vo, ap, cm = out
    sr, W, hop, tau_min, tau_max, span = geometry(conf)
    ref = restated(y, conf)
    c = measured_c()
    T = ref['dp'].shape[0]
    assert cm.shape == (T, tau_max + 2) and f0.shape == vo.shape == ap.shape == (T,), (tag, cm.shape)
    # 1: every d' within its bound; exact where the bound is zero
    bound = c * unit(ref['dp'], conf)
    diff = np.abs(cm.astype(np.float64) - ref['dp'])
    share = (diff[bound > 0] / bound[bound > 0]).max()
    print('%s: d\' worst difference %.3g, worst share of its bound %.3g' % (tag, diff.max(), share))
    assert np.isfinite(cm).all() and (cm[:, 0] == 1.0).all(), tag
    assert (diff <= bound).all(), '%s: %d of %d d\' beyond their bound, worst %.3g of it' % (tag, int((diff > bound).sum()), diff.size, share)
    # 2: the decision on the kernel's own d', in fp32 in the kernel's order: bit for bit, the pitch within 2 ulp
    lag32, ap32, f032, _, _ = decide(cm, conf, np.float32)
    assert same_bits(vo, (lag32 > 0).astype(np.uint8)), tag
    assert same_bits(ap, ap32), (tag, np.nonzero(ap != ap32)[0])
    assert ((f0 == 0) == (lag32 == 0)).all() and same_bits(f0[lag32 == 0], np.zeros_like(f0[lag32 == 0])), tag
    assert _within_ulp(f0, f032, 2), (tag, np.abs(f0 - f032).max())
    # the chosen lag, from the pitch: sr / exp(pitch) lies within (lag - 1, lag + 1), and aperiodicity names d'(lag)
    v = lag32 > 0
    assert (np.abs(sr / np.exp(f0[v].astype(np.float64)) - lag32[v]) <= 1 + 1e-5).all(), tag
    assert same_bits(ap[v], cm[np.nonzero(v)[0], lag32[v]]), tag
    # 3: against the float64 tracker on the frames whose decision clears the bound
    ok = clear_frames(ref, conf, c)
    assert (lag32[ok] == ref['lag'][ok]).all(), (tag, np.nonzero(ok & (lag32 != ref['lag']))[0])
    both = ok & (ref['lag'] > 0)
    dl = np.abs(f0.astype(np.float64) - ref['pitch'])
    lim = lnf0_bound(ref, conf, c)
    if both.any():
        print('%s: %d of %d frames compared, %d voiced; ln f0 worst difference %.3g, worst share of its bound %.3g'
              % (tag, int(ok.sum()), T, int(both.sum()), dl[both].max(), (dl[both] / lim[both]).max()))
    assert (dl[both] <= lim[both]).all(), (tag, np.nonzero(both & (dl > lim))[0])
    if stats is not None:
        stats.append((int(ok.sum()), T))


def check_left_out_cap():
    """the condition of test 3: at most 2 % of the frames of all inputs fall inside the margin (a fact of the float64 side)"""
    c = measured_c()
    out = total = 0
    for name, y, conf in all_inputs():
        ok = clear_frames(restated(y, conf), conf, c)
        out, total = out + int((~ok).sum()), total + ok.size
        assert (~ok).sum() <= 0.02 * ok.size or ok.size < 50, (name, int((~ok).sum()), ok.size)
    print('%d of %d frames inside the margin' % (out, total))
    assert out <= 0.02 * total, (out, total)


def check_length(dev, name):
    y = small_wave(name)
    ex = extractor(dev, **SMALL)
    assert (ex.win, ex.hop, ex.tau_min, ex.tau_max, ex.span) == (64, 25, 8, 40, 105)
    _check(name, _run(ex, y), y, SMALL)


def check_gap(dev):
    y = gap_wave()
    out = _run(extractor(dev, **SMALL), y)
    _check('noise in the middle', out, y, SMALL)
    quiet = [t for t in range(34) if t * 25 - 52 >= GAP[2][0] and t * 25 + 53 <= GAP[2][1]]
    assert not out[1][quiet].any() and not out[0][quiet].any() and out[1][3:11].all()


def check_real_geometry(dev):
    y, _ = real_wave()
    ex = extractor(dev, **DEFAULTS)
    assert (ex.win, ex.hop, ex.tau_min, ex.tau_max) == (800, 200, 32, 266)
    out = _run(ex, y)
    assert out[0].shape == (81,)
    _check('real geometry', out, y, DEFAULTS)


def check_periodic_is_exact(dev):
    """a frame of an exactly periodic signal of small integers (times 2^-2) has d'(period) == 0.0: the direct difference form"""
    y = square_wave()
    f0, vo, ap, cm = _run(extractor(dev, **SMALL), y)
    inside = [t for t in range(17) if t * 25 - 52 >= 0 and t * 25 + 53 <= 400]
    assert len(inside) >= 8
    for t in inside:
        assert cm[t, 16] == 0.0 and cm[t, 32] == 0.0 and cm[t, 8] > 1.0, (t, cm[t, 16])
        # (d'(15) and d'(17) differ -- the normalisation grows with the lag -- so the parabola's vertex is close to 16, not on it)
        assert vo[t] == 1 and ap[t] == 0.0 and abs(np.exp(f0[t]) / 125.0 - 1) < 0.01, (t, f0[t])
    _check('square wave', (f0, vo, ap, cm), y, SMALL)


# ---- 4: structure ----------------------------------------------------------------------------------------------------------------------------
def check_ragged(dev):
    ex = extractor(dev, **SMALL)
    wavs = ragged_waves()
    f0, vo, ap, cm, length = ex.extract(wavs, voiced=True, aperiodicity=True, cmnd=True)
    T = [1 + n // 25 for n in RAGGED]
    assert length.dtype == torch.int64 and length.tolist() == T and f0.shape == vo.shape == ap.shape == (3, max(T))
    assert cm.shape == (3, max(T), 42)
    got = [t.cpu().numpy() for t in (f0, vo, ap, cm)]
    # a wider batch whose padding is NaN: nothing behind an utterance's own length is read
    wide = np.full((3, max(RAGGED) + 211), np.nan, dtype=np.float32)
    for i, w in enumerate(wavs):
        wide[i, :len(w)] = w
    again = ex.extract(torch.from_numpy(wide), lengths=list(RAGGED), voiced=True, aperiodicity=True, cmnd=True)
    assert again[-1].tolist() == T and all(same_bits(a.cpu().numpy(), g) for a, g in zip(again[:4], got))
    for i, w in enumerate(wavs):
        solo = _run(ex, w)
        for g, s in zip(got, solo):
            assert same_bits(g[i, :T[i]], s), i
            assert same_bits(g[i, T[i]:], np.zeros_like(g[i, T[i]:])), i                 # rows past T_b are zero
    # the extras are optional and ordered; pitch_track is the layout of a batch's ``pitch`` entry
    only = ex.extract(wavs)
    assert len(only) == 2 and same_bits(only[0].cpu().numpy(), got[0]) and only[1].tolist() == T
    f0a, apa, _ = ex.extract(wavs, aperiodicity=True)
    assert same_bits(f0a.cpu().numpy(), got[0]) and same_bits(apa.cpu().numpy(), got[2])
    track = ex.extract(wavs, pitch_track=True)[0]
    assert track.shape == (3, max(T), 1) and same_bits(track[..., 0].cpu().numpy(), got[0])
    from msmctts_amd.hip import pitch
    assert pitch.pitch_track(torch.from_numpy(got[0])).shape == (3, max(T), 1)
    # the same frame count as the mel and the energy
    fex = fcases.extractor(dev, **fcases.SMALL)
    assert [ex.feat_length(n) for n in RAGGED + (53, 790, 799, 800)] == [fex.feat_length(n) for n in RAGGED + (53, 790, 799, 800)]


def check_repeat(dev):
    ex = extractor(dev, **SMALL)
    wavs = ragged_waves()
    a = ex.extract(wavs, voiced=True, aperiodicity=True, cmnd=True)
    b = ex.extract(wavs, voiced=True, aperiodicity=True, cmnd=True)
    assert all(same_bits(p.cpu().numpy(), q.cpu().numpy()) for p, q in zip(a, b))


def check_silence(dev):
    y = np.zeros(431, dtype=np.float32)
    f0, vo, ap, cm = _run(extractor(dev, **SMALL), y)
    assert same_bits(f0, np.zeros_like(f0)) and not vo.any() and same_bits(ap, np.ones_like(ap)) and same_bits(cm, np.ones_like(cm))


def check_int16(dev):
    q = int16_wave()
    y = q.astype(np.float32) / np.float32(32768.0)
    ex = extractor(dev, **SMALL)
    a, b, c = _run(ex, q), _run(ex, y), _run(ex, y.astype(np.float64))
    assert all(same_bits(u, v) and same_bits(u, w) for u, v, w in zip(a, b, c))
    _check('int16', a, y, SMALL)


def check_hz(dev):
    """``log=False``: the Hz track and the log track name the same F0 -- ln(Hz) within 2 ulp of the log track (an ulp of the Hz
    value itself is out of reach of any logf: half an ulp of ln f0 = 5 is 4 ulp of f0) --, 0 stays 0, the rest has the same bits"""
    y = gap_wave()
    a = _run(extractor(dev, **SMALL), y)
    b = _run(extractor(dev, log=False, **SMALL), y)
    assert all(same_bits(u, v) for u, v in zip(a[1:], b[1:]))
    v = a[1] > 0
    assert v.any() and not v.all() and same_bits(b[0][~v], np.zeros_like(b[0][~v])) and (b[0][v] > 0).all()
    assert _within_ulp(np.log(b[0][v].astype(np.float64)).astype(np.float32), a[0][v], 2)
    lag32, _, hz32, _, _ = decide(b[3], SMALL, np.float32, log=False)
    assert _within_ulp(b[0], hz32, 2)


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw(dev, L, W=64, hop=25, tau_min=8, tau_max=40, B=1, sr=2000, thr=0.15, null=None):
    """msmc_pitch_yin on sentinel-filled outputs -> (rc, outputs untouched?, launches logged)"""
    from msmctts_amd.hip import lib
    h = lib.get()
    T = 1 + max(L, 0) // max(hop, 1)
    wav = torch.zeros((B, max(L, 1)), dtype=torch.float32).to(dev)
    ln = torch.full((B,), L, dtype=torch.int32).to(dev)
    f0 = torch.full((B, T), -7.25, dtype=torch.float32).to(dev)
    ap = torch.full((B, T), -7.25, dtype=torch.float32).to(dev)
    vo = torch.full((B, T), 7, dtype=torch.uint8).to(dev)
    cm = torch.full((B, T, max(tau_max, 0) + 2), -7.25, dtype=torch.float32).to(dev)
    arg = {'wav': wav, 'length': ln, 'pitch': f0, 'voiced': vo, 'aper': ap, 'cmnd': cm}
    p = {k: (None if null == k else lib.ptr(t)) for k, t in arg.items()}
    h.msmc_prof_enable(1)
    try:
        rc = h.msmc_pitch_yin(p['wav'], p['length'], p['pitch'], p['voiced'], p['aper'], p['cmnd'], B, L, T, W, hop, tau_min,
                              tau_max, sr, thr, 1, lib.stream(wav))
        if dev != 'cpu':
            torch.cuda.synchronize()
        launches = h.msmc_prof_count()
    finally:
        h.msmc_prof_enable(0)
    return rc, bool((f0 == -7.25).all() and (ap == -7.25).all() and (vo == 7).all() and (cm == -7.25).all()), launches


def check_refusals(dev):
    assert _raw(dev, 300) == (0, False, 1)                                     # the accepted call launches once and writes
    rc, untouched, launches = _raw(dev, 300, null='voiced')                    # an optional output may be NULL
    assert (rc, launches) == (0, 1)
    assert _raw(dev, 53)[0] == 0
    for kw in (dict(L=52), dict(L=0), dict(L=300, tau_min=1), dict(L=300, tau_min=8, tau_max=8), dict(L=300, tau_min=9, tau_max=8),
               dict(L=300, W=0), dict(L=300, hop=0), dict(L=300, B=0), dict(L=60, B=65536), dict(L=300, thr=0.0),
               dict(L=300, thr=-0.15), dict(L=300, sr=0), dict(L=300, null='wav'), dict(L=300, null='length'),
               dict(L=300, null='pitch'),                  # (the last two: a sample span beyond LDS, by the hop and by the window)
               dict(L=300, hop=2000), dict(L=30000, W=41000)):
        assert _raw(dev, **kw) == (E_SHAPE, True, 0), kw
    # the host layer: ValueError with the offending value, before any launch
    from msmctts_amd.hip import lib
    ex = extractor(dev, **SMALL)
    h = lib.get()
    h.msmc_prof_enable(1)
    try:
        assert '52' in str(_raises(ValueError, lambda: ex.extract(np.zeros(52, dtype=np.float32))))
        assert '47' in str(_raises(ValueError, lambda: ex.extract([small_wave('L400'), np.zeros(47, dtype=np.float32)])))
        assert h.msmc_prof_count() == 0
    finally:
        h.msmc_prof_enable(0)
    assert '260' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, fmin=260))))            # fmin >= fmax
    assert '250' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, fmin=250))))
    assert '1200' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, fmax=1200))))          # tau_min = 1
    assert '-0.5' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, threshold=-0.5))))
    assert 'threshold = 0' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, threshold=0.0))))
    _raises(TypeError, lambda: ex.extract(np.zeros(400, dtype=np.int32)))
    _raises(ValueError, lambda: ex.extract(torch.zeros(2, 400), lengths=[400]))


def check_host_tensors_need_the_interpreter():
    """without the interpreter build bound a host tensor raises as for every other operator"""
    from msmctts_amd.hip import lib
    saved = lib._host_pointers_ok
    lib._host_pointers_ok = False
    try:
        err = _raises(RuntimeError, lambda: extractor('cpu', **SMALL).extract(small_wave('L400')))
        assert 'GPU only' in str(err)
    finally:
        lib._host_pointers_ok = saved


# ---- 6: the tool ---------------------------------------------------------------------------------------------------------------------------
def check_tool(dev, tmp_path):
    import importlib.util
    import io
    spec = importlib.util.spec_from_file_location('extract_features_tool', os.path.join(ROOT, 'tools', 'extract_features.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, plain, full = str(tmp_path / 'wav'), str(tmp_path / 'plain'), str(tmp_path / 'full')
    os.makedirs(src)
    # the small-geometry signals, written as 16 kHz files: the features' small geometry is defined there (lags 8 .. 40 again)
    pcm = {'b_long': np.round(small_wave('T34 two tiles L825') * 30000.0).astype(np.int16), 'a_short': int16_wave()}
    for uid, q in pcm.items():
        _write_wav(os.path.join(src, uid + '.wav'), q, 16000)
    fex = fcases.extractor(dev, **fcases.SMALL)
    pex = extractor(dev, **dict(SMALL, sample_rate=16000, fmin=400, fmax=2000))
    assert (pex.tau_min, pex.tau_max, pex.hop) == (8, 40, fex.hop)
    log = io.StringIO()
    assert tool.extract_dir(fex, src, plain, energy=True, jobs=2, out=log)[0] == 2
    assert sorted(os.listdir(plain)) == ['energy', 'mel']                      # without --pitch the directory does not appear
    assert tool.extract_dir(fex, src, full, energy=True, jobs=2, out=log, pitch=pex)[0] == 2
    assert sorted(os.listdir(full)) == ['energy', 'mel', 'pitch']
    from msmctts_amd.datasets import readers
    for uid, q in pcm.items():
        got = np.load(os.path.join(full, 'pitch', uid + '.npy'))
        assert got.shape == (1 + len(q) // 25,) and got.dtype == np.float32 and (got > 0).any()
        assert same_bits(got, pex.extract(q)[0][0].cpu().numpy()), uid
        assert readers.read_npy(os.path.join(full, 'pitch', uid + '.npy'), shape_only=True) == (1 + len(q) // 25,)
        for kind in ('mel', 'energy'):                                         # and the other files have the bits they had
            assert same_bits(np.load(os.path.join(full, kind, uid + '.npy')), np.load(os.path.join(plain, kind, uid + '.npy')))
    # a pitch extractor on another frame grid is refused before anything is written
    other = str(tmp_path / 'other')
    err = _raises(ValueError, lambda: tool.extract_dir(fex, src, other, jobs=2, out=log, pitch=extractor(dev, **SMALL)))
    assert '2000' in str(err) and not os.path.exists(other)


def check_config():
    from msmctts_amd.hip.pitch import PitchExtractor
    for conf in ({'fmin': 80, 'threshold': 0.1, 'num_mels': 40}, {'hparams': {'fmin': 80, 'threshold': 0.1, 'num_mels': 40}}):
        ex = PitchExtractor.from_config(conf)
        assert (ex.win, ex.hop, ex.tau_min, ex.tau_max, ex.threshold) == (800, 200, 32, 200, 0.1)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    assert 'msmc_pitch_yin' in lib.exported_symbols() and hasattr(lib.get(), 'msmc_pitch_yin')
    from msmctts_amd.hip.pitch import PitchExtractor
    from msmctts_amd.networks.vqgantts import msmc_vqgan_emb
    assert msmc_vqgan_emb.PitchExtractor is PitchExtractor and hasattr(msmc_vqgan_emb, 'FeatureExtractor')
    ex = PitchExtractor()
    assert (ex.win, ex.hop, ex.tau_min, ex.tau_max) == (800, 200, 32, 266) and ex.log and ex.threshold == 0.15
    assert lib.get().msmc_pitch_yin_tile(0) == FRAME_TILE
