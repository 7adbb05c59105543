"""Shared cases of the spectrogram and the Griffin-Lim inverses: csrc/griffin_lim.hip (msmc_stft, msmc_istft, msmc_deemphasis),
their host side (msmctts_amd/hip/griffin_lim.py ``GriffinLim``) and tools/invert_features.py / tools/extract_features.py
--spectrogram.  tests/test_griffin_lim_emu.py runs them on the kernel interpreter, tests/test_gpu_griffin_lim.py on the GPU.

References.  ``stft64`` / ``istft64`` restate librosa.stft / librosa.istft with their defaults in float64 numpy (reflect padding,
periodic Hann centred in n_fft, rfft / irfft, overlap-add, division by the summed squared windows above the smallest normal
fp32, n_fft / 2 trimmed); ``restated_*`` put the reference's audio.py around them.  ``check_restatement`` pins them against
tests/golden/griffin_lim.npz -- the reference's own code around restated transforms (tests/golden/make_golden_griffin_lim.py) -- to
1e-9 relative to the largest value of each output.

Tolerances against float64 (every element, none left out).  With u = 2^-24:
  stft (complex): a bin is a sum of ``win`` products frame[n] basis[n][f], |basis| <= w[n] <= 1, so the unit of the bound is
      U_st[t] = u sqrt(win) |windowed frame t|_2                        for re and im of every frequency of frame t.
  db: an error d on |z| moves the normalised value by K d / max(|z|, 1e-5), K as in tests/_featurecases.py: unit K U_st / max(..).
  istft: a tap is a sum of K = 2 F products spec[t][k] ibasis[k][n], |ibasis| <= 2 w[n] / n_fft; sample j adds the taps of the
      frames that cover it and divides by env[j] = sum w^2 (where that exceeds the smallest normal fp32):
      U_ist[j] = u sqrt(2 F) sum_t |spec[t]|_2 (2 w[n_t] / n_fft) / env[j].
  round trip: istft is linear, so an error of c_st U_st[t] on each of the 2 F numbers of frame t moves sample j by at most
      c_st sum_t U_st[t] (2 (2 F) / n_fft) w[n_t] / env[j]; added to c_ist U_ist[j] of the kernel's own spectrum.
  de-emphasis: U_de = u max|x| / (1 - a), the gain of the recurrence on the roundings of its states.
The constants c are MEASURED, never on the kernel: the same chains in fp32 numpy on the kernel's own fp32 constants against
float64, the worst ratio to the unit over the inputs of the tests, times 8 for the MFMA's sequential fmaf chain (``measured_c``;
it prints them; profiles/griffin_lim.md has the values and the share of each bound the kernels used on an MI355X).
  project: given the kernel's own z, t1 = mag z / |z| within 4 u mag per component (three roundings of the normalised
      components, their squares' sum and root, two quotients and a product: 3 u by the first-order count, 4 asserted);
      with prev: out = t1 + alpha (t1 - t0) within 4 u mag (1 + alpha) + 2 u (|t1 - t0| + |out|) (fp32 alpha, three roundings).
Whole Griffin-Lim runs are NOT compared per element (rounding moves the phase of near-zero bins): their spectral convergence
sc = || |STFT(y)| - S || / || S ||, evaluated in float64 on the host, must lie within half the spread (max - min) of the
reference's sc over the fixture's 8 draws of the reference's sc from the same phases.  The first inverse of every run,
istft(S angles), IS checked per element.  Ragged batches against solo runs, repeats, silence and padding are compared BIT FOR BIT.
"""
import os

import numpy as np
import torch
from scipy.signal import lfilter

import _featurecases as fc
from _featurecases import SMALL, _raises, same_bits

E_SHAPE = -2
ROOT = fc.ROOT
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'griffin_lim.npz')
U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
SMALL8 = dict(SMALL, griffin_lim_iters=8)
# hop > win (gaps: the envelope rule), hop == win, win == n_fft (halo of 10 frames, 22 positions per workgroup)
GEOMETRIES = {
    'hop > win': dict(SMALL, win_length=64, hop_length=80),
    'hop == win': dict(SMALL, win_length=64, hop_length=64),
    'win == n_fft': dict(SMALL, win_length=256, hop_length=25),
}
# frames: the shortest accepted (25 * 6 = 150 > 128), the workgroup's own edge at this geometry (32 - 4 = 28 positions), 32 / 33,
# three workgroups
ISTFT_FRAMES = (7, 28, 29, 32, 33, 70)
RAGGED_FRAMES = (70, 33, 7)
DEEMPH_LENGTHS = (1, 255, 256, 257, 1000)


def griffin_lim(dev, **kw):
    from msmctts_amd.hip.griffin_lim import GriffinLim
    return GriffinLim(device=dev, **kw)


def geom(conf):
    return fc.geometry(conf)


def window(conf, full=True):
    n_fft, hop, win = geom(conf)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    left = (n_fft - win) // 2
    return np.pad(w, (left, n_fft - win - left)) if full else w


def stft64(y, conf):
    """[T, F] complex128"""
    n_fft, hop, win = geom(conf)
    p = np.pad(np.asarray(y, dtype=np.float64), n_fft // 2, mode='reflect')
    idx = hop * np.arange(1 + len(y) // hop)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(p[idx] * window(conf)[None, :], axis=1)


def _overlap_add(frames, conf, dt=np.float64):
    """windowed frames [T, n_fft] -> (trimmed sum, trimmed envelope, untrimmed length)"""
    n_fft, hop, win = geom(conf)
    T = frames.shape[0]
    y, env = np.zeros(n_fft + hop * (T - 1), dtype=dt), np.zeros(n_fft + hop * (T - 1), dtype=dt)
    w2 = (window(conf) ** 2).astype(dt)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += frames[t]
        env[t * hop:t * hop + n_fft] += w2
    keep = slice(n_fft // 2, n_fft // 2 + hop * (T - 1))
    return y[keep], env[keep]


def istft64(D, conf):
    """D [T, F] complex -> [hop (T - 1)] float64"""
    n_fft = geom(conf)[0]
    fr = np.fft.irfft(np.asarray(D, dtype=np.complex128), n_fft, axis=1) * window(conf)[None, :]
    y, env = _overlap_add(fr, conf)
    ok = env > TINY
    y[ok] /= env[ok]
    return y


def preemph64(y, a):
    return lfilter([1.0, -a], [1.0], np.asarray(y, dtype=np.float64))


def normalise64(S, conf):
    return fc._normalise(S, conf)


def spectrogram64(y, conf):
    D = stft64(preemph64(y, conf['preemphasis']), conf)
    return normalise64(20 * np.log10(np.maximum(1e-5, np.abs(D))) - conf['ref_level_db'], conf)


def amplitudes64(x, conf, power=1.5, inv_mel=None):
    """``_db_to_amp(_denormalize(x) + ref)`` (then ``_mel_to_linear``) ``** power`` of a normalised [T, F] / [T, M]"""
    lo, top = conf['min_level_db'], conf['max_abs_value']
    x = np.asarray(x, dtype=np.float64)
    if conf['symmetric_specs']:
        D = (np.clip(x, -top, top) + top) * -lo / (2 * top) + lo
    else:
        D = np.clip(x, 0, top) * -lo / top + lo
    A = np.power(10.0, (D + conf['ref_level_db']) * 0.05)
    if inv_mel is not None:
        A = np.maximum(1e-10, A @ np.asarray(inv_mel, dtype=np.float64).T)
    return A ** power


def griffin_lim64(S, phase, conf, iters, fast=False):
    """``_griffin_lim`` / ``_fast_griffin_lim`` on S [T, F], phases in turns [T, F] -> y before ``inv_preemphasis``"""
    t0 = c = S * np.exp(2j * np.pi * phase)
    y = istft64(c, conf)
    for _ in range(iters):
        t1 = S * np.exp(1j * np.angle(stft64(y, conf)))
        c = t1 + 0.99 * (t1 - t0) if fast else t1
        t0 = t1
        y = istft64(c, conf)
    return y


def spectral_convergence(y, S, conf):
    return float(np.linalg.norm(np.abs(stft64(y, conf)) - S) / np.linalg.norm(S))


def fixture():
    z = np.load(GOLDEN)
    conf = dict(SMALL)
    for k in fc.DEFAULTS:
        conf[k] = z['hparam.' + k].item()
    for k in ('num_mels', 'num_freq', 'sample_rate'):
        conf[k] = int(conf[k])
    conf['symmetric_specs'] = bool(conf['symmetric_specs'])
    del conf['win_length'], conf['hop_length']
    return conf, z


def small_conf():
    """the fixture's hparams: the small geometry through the millisecond values, as the reference's ``_stft_parameters`` has it"""
    conf, z = fixture()
    assert geom(conf) == (256, 25, 101) and conf['num_mels'] == 20 and int(z['hparam.griffin_lim_iters'].item()) == 8
    return conf


# ---- the fp32 numpy chains and the measured constants ---------------------------------------------------------------------------
def _wframes(y, conf, pre, dt):
    """windowed frames' norm needs float64; the fp32 chain needs the unwindowed frames in fp32"""
    return fc._frames(y, dict(conf, preemphasis=pre), dt)


def stft_unit(y, conf, pre=0.0):
    """U_st [T]"""
    win = geom(conf)[2]
    fr = _wframes(y, conf, pre, np.float64) * window(conf, full=False)[None, :]
    return U * np.sqrt(win) * np.linalg.norm(fr, axis=1)


def stft32(y, conf, pre=0.0):
    from msmctts_amd.hip.features import windowed_dft_basis
    n_fft, hop, win = geom(conf)
    F = n_fft // 2 + 1
    b = windowed_dft_basis(n_fft, win, F, 1)[0]
    fr = _wframes(np.asarray(y, dtype=np.float32), conf, np.float32(pre), np.float32)
    return fr @ b[:, :F], fr @ b[:, F:]


def _ibasis(conf):
    from msmctts_amd.hip.griffin_lim import inverse_dft_basis
    n_fft, hop, win = geom(conf)
    return inverse_dft_basis(n_fft, win, win, 1)[0][:n_fft + 2]              # [2 F, win] fp32


def _cover(conf, T):
    """for the trimmed samples: (w[n_t] summed over covering frames weighted by ``per_frame`` -> function, envelope)"""
    n_fft, hop, win = geom(conf)

    def spread(per_frame):
        fr = np.asarray(per_frame, dtype=np.float64)[:, None] * window(conf)[None, :]
        return _overlap_add(fr, conf)[0]
    env = _overlap_add(np.zeros((T, n_fft)), conf)[1]
    return spread, env


def istft_unit(D, conf):
    """U_ist [hop (T - 1)] for the spectrum D [T, F]"""
    n_fft = geom(conf)[0]
    spread, env = _cover(conf, D.shape[0])
    nrm = np.sqrt((np.abs(D) ** 2).sum(axis=1))
    s = spread(nrm * 2.0 / n_fft)
    return U * np.sqrt(n_fft + 2) * np.where(env > TINY, s / np.where(env > TINY, env, 1.0), s)


def istft32(D, conf):
    """the chain of the kernel in fp32 numpy: [T, 2 F] @ [2 F, win], overlap-add, division"""
    n_fft, hop, win = geom(conf)
    A = np.concatenate([D.real, D.imag], axis=1).astype(np.float32)
    fr = np.zeros((D.shape[0], n_fft), dtype=np.float32)
    off = (n_fft - win) // 2
    fr[:, off:off + win] = A @ _ibasis(conf)
    y, _ = _overlap_add(fr, conf, np.float32)
    env = _overlap_add(np.zeros((D.shape[0], n_fft), dtype=np.float32), conf, np.float32)[1]
    ok = env > np.float32(TINY)
    y[ok] /= env[ok]
    return y


def deemph32(x, a):
    y, a, prev = np.empty_like(x), np.float32(a), np.float32(0)
    for n in range(len(x)):
        prev = y[n] = x[n] + a * prev
    return y


def deemph_input(n, seed=0):
    return fc.small_wave(max(n, 8), 20 + seed)[:n]


def wave(T, seed=0, conf=SMALL):
    """a waveform of exactly T frames at the geometry of ``conf``"""
    return fc.small_wave((T - 1) * geom(conf)[1] + 3, seed)


def spectrum(T, seed=0, conf=SMALL):
    """a complex64-exact spectrum of T frames: the float64 STFT of ``wave`` rounded to fp32"""
    return stft64(wave(T, seed, conf), conf).astype(np.complex64).astype(np.complex128)


def transform_inputs():
    out = [(wave(T), SMALL) for T in ISTFT_FRAMES] + [(wave(T, 1 + i), SMALL) for i, T in enumerate(RAGGED_FRAMES)]
    return out + [(wave(40, 3, c), c) for c in GEOMETRIES.values()] + [(np.load(GOLDEN)['wav'], SMALL)]


_C = {}


def measured_c(verbose=True):
    """{'stft', 'db', 'istft', 'deemph'}: 8 x the worst ratio of |fp32 numpy chain - float64| to the unit over the tests' inputs"""
    if not _C:
        worst = dict(stft=0.0, db=0.0, istft=0.0, deemph=0.0)
        for y, conf in transform_inputs():
            Z = stft64(y, conf)
            re, im = stft32(y, conf)
            unit = stft_unit(y, conf)[:, None]
            worst['stft'] = max(worst['stft'], (np.abs(re - Z.real) / unit).max(), (np.abs(im - Z.imag) / unit).max())
            D = Z.astype(np.complex64).astype(np.complex128)
            d, unit = np.abs(istft32(D, conf) - istft64(D, conf)), istft_unit(D, conf)
            assert not d[unit == 0].any()                                      # (samples no window covers: +0 in every chain)
            worst['istft'] = max(worst['istft'], (d[unit > 0] / unit[unit > 0]).max())
        for (y, conf) in db_inputs():
            ref, unit = spectrogram64(y, conf), db_unit(y, conf)
            worst['db'] = max(worst['db'], (np.abs(db32(y, conf) - ref) / unit).max())
        for n in DEEMPH_LENGTHS:
            x = deemph_input(n)
            ref = lfilter([1.0], [1.0, -0.97], x.astype(np.float64))
            worst['deemph'] = max(worst['deemph'], (np.abs(deemph32(x, 0.97) - ref) / (U * np.abs(x).max() / 0.03)).max())
        _C.update({k: 8 * v for k, v in worst.items()})
        if verbose:
            print('fp32 numpy chains against float64, worst ratio to the unit -> c = 8 x: '
                  + ', '.join('%s %.4g -> %.4g' % (k, v, 8 * v) for k, v in worst.items()))
    return _C


def real_conf():
    return fc.fixture()[0]


def db_inputs():
    return [(np.load(GOLDEN)['wav'], small_conf()), (fc.fixture()[1][0], real_conf())]


def db_unit(y, conf):
    K = (2 if conf['symmetric_specs'] else 1) * conf['max_abs_value'] * 20 / (np.log(10) * abs(conf['min_level_db']))
    mag = np.abs(stft64(preemph64(y, conf['preemphasis']), conf))
    # the pre-emphasis runs in fp32 inside the kernel: its rounding is part of the summed operand's, one more unit of it
    return K * stft_unit(y, conf, conf['preemphasis'])[:, None] / np.maximum(mag, 1e-5)


def db32(y, conf):
    f32 = np.float32
    re, im = stft32(y, conf, conf['preemphasis'])
    S = f32(20) * np.log10(np.maximum(f32(1e-5), np.sqrt(re * re + im * im))) - f32(conf['ref_level_db'])
    return normalise64(S, dict(conf, min_level_db=f32(conf['min_level_db']), max_abs_value=f32(conf['max_abs_value'])))


def _within(tag, got, ref, bound):
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    live = np.broadcast_to(bound, d.shape) > 0
    share = (d[live] / np.broadcast_to(bound, d.shape)[live]).max() if live.any() else 0.0
    print('%s: worst difference %.3g, worst share of its bound %.3g' % (tag, d.max() if d.size else 0.0, share))
    assert np.isfinite(np.asarray(got)).all(), tag
    assert (d <= bound).all(), '%s: %d of %d elements beyond their bound, worst %.3g of it' % (tag, int((d > bound).sum()), d.size, share)


# ---- 1: the restatement against the reference fixture ----------------------------------------------------------------------------
def check_restatement():
    conf, z = fixture()
    assert geom(conf) == (256, 25, 101) and z['phase.0'].shape == (129, 61)
    a, iters, power = conf['preemphasis'], int(z['hparam.griffin_lim_iters'].item()), float(z['hparam.power'].item())
    y = z['wav'].astype(np.float64)

    def rel(got, want):
        return np.abs(got - want).max() / np.abs(want).max()
    errs = {'spectrogram': rel(spectrogram64(y, conf).T, z['spectrogram'])}
    rc, wavs = real_conf(), fc.fixture()[1]
    errs['real spectrogram'] = rel(spectrogram64(wavs[0], rc).T, z['real.spectrogram'])
    assert same_bits(np.random.RandomState(0).rand(129, 61), z['phase.0'])
    S = amplitudes64(z['spectrogram'].T, conf, power)
    ph = z['phase.0'].T
    de = lambda v: lfilter([1.0], [1.0, -a], v)                                # noqa: E731
    errs['inv_spectrogram'] = rel(de(griffin_lim64(S, ph, conf, iters)), z['inv_spectrogram'])
    errs['fast_inv_spectrogram'] = rel(de(griffin_lim64(S, ph, conf, iters, fast=True)), z['fast_inv_spectrogram'])
    # the reference's pseudo-inverse ran in fp32 LAPACK: followed with its matrix; this project's float64 one agrees to fp32 rounding
    Sm = amplitudes64(z['mel'].T, conf, power, inv_mel=z['inv_mel_basis'])
    errs['inv_mel_spectrogram'] = rel(de(griffin_lim64(Sm, ph, conf, iters)), z['inv_mel_spectrogram'])
    for k in range(8):
        errs['draw %d' % k] = rel(de(griffin_lim64(S, np.random.RandomState(k).rand(129, 61).T, conf, iters)), z['draw.%d' % k])
    print('restatement against the reference fixture, relative to the largest value: '
          + ', '.join('%s %.3g' % kv for kv in errs.items()))
    assert max(errs.values()) <= 1e-9, errs
    own = griffin_lim('cpu', **conf).inv_mel_basis()
    assert own.dtype == np.float64 and rel(own, z['inv_mel_basis'].astype(np.float64)) <= 1e-4


# ---- 2: stft, complex and db --------------------------------------------------------------------------------------------------
def _complex_of(gl, y, lengths=None):
    z, fl = gl.stft(y, lengths)
    return z.cpu().numpy().astype(np.complex128), fl


def check_stft_complex(dev):
    gl = griffin_lim(dev, **SMALL8)
    c = measured_c()['stft']
    for T in (7, 32, 33, 70):
        y = wave(T)
        z, fl = _complex_of(gl, y)
        Z = stft64(y, SMALL)
        assert fl.tolist() == [T] and z.shape == (1, T, 129)
        bound = c * stft_unit(y, SMALL)[:, None]
        _within('stft re, T = %d' % T, z[0].real, Z.real, bound)
        _within('stft im, T = %d' % T, z[0].imag, Z.imag, bound)
    # a ragged batch with poisoned padding: the bits of the solo runs, +0 rows behind
    ys = [wave(T, 1 + i) for i, T in enumerate(RAGGED_FRAMES)]
    wide = np.full((3, max(len(v) for v in ys) + 77), np.nan, dtype=np.float32)
    for i, v in enumerate(ys):
        wide[i, :len(v)] = v
    zb = gl.stft(torch.from_numpy(wide), [len(v) for v in ys], planar=True)[0].cpu().numpy()
    for i, (v, T) in enumerate(zip(ys, RAGGED_FRAMES)):
        solo = gl.stft(v, planar=True)[0].cpu().numpy()
        assert same_bits(zb[i, :T], solo[0]) and same_bits(zb[i, T:], np.zeros_like(zb[i, T:])), i


def check_db(dev):
    """``spectrogram`` against the fixture's, at the small and at the real geometry (21 frames)"""
    conf, z = fixture()
    c = measured_c()['db']
    for tag, (y, cf), want in zip(('small', 'real'), db_inputs(), (z['spectrogram'], z['real.spectrogram'])):
        sp, fl = griffin_lim(dev, **cf).spectrogram(y)
        assert sp.shape == (1,) + want.T.shape and sp.dtype == torch.float32 and fl.tolist() == [want.shape[1]]
        _within('spectrogram, %s geometry' % tag, sp[0].cpu().numpy(), want.T, c * db_unit(y, cf))


# ---- 3: istft -----------------------------------------------------------------------------------------------------------------
def _istft(gl, D, feat_length=None):
    y, ln = gl.istft(torch.from_numpy(np.asarray(D).astype(np.complex64)), feat_length)
    return y.cpu().numpy(), ln.tolist()


def check_istft_length(dev, T):
    gl = griffin_lim(dev, **SMALL8)
    D = spectrum(T)
    y, ln = _istft(gl, D[None])
    assert y.shape == (1, 25 * (T - 1)) and ln == [25 * (T - 1)] and y.dtype == np.float32
    _within('istft, T = %d' % T, y[0], istft64(D, SMALL), measured_c()['istft'] * istft_unit(D, SMALL))


def check_istft_geometry(dev, name):
    conf = GEOMETRIES[name]
    gl = griffin_lim(dev, **conf)
    D = spectrum(40, 3, conf)
    y, _ = _istft(gl, D[None])
    ref = istft64(D, conf)
    _within('istft, ' + name, y[0], ref, measured_c()['istft'] * istft_unit(D, conf))
    if name == 'hop > win':                                                    # the samples between two windows stay +0
        env = _cover(conf, 40)[1]
        assert (env <= TINY).sum() >= 38 * 15 and same_bits(y[0][env <= TINY], np.zeros(int((env <= TINY).sum()), dtype=np.float32))


def check_istft_ragged(dev):
    gl = griffin_lim(dev, **SMALL8)
    Ds = [spectrum(T, 1 + i) for i, T in enumerate(RAGGED_FRAMES)]
    batch = np.full((3, 70, 129), np.nan + 1j * np.nan, dtype=np.complex64)
    for i, D in enumerate(Ds):
        batch[i, :len(D)] = D
    y, ln = _istft(gl, batch, list(RAGGED_FRAMES))
    assert ln == [25 * (T - 1) for T in RAGGED_FRAMES]
    for i, D in enumerate(Ds):
        solo, _ = _istft(gl, D[None])
        assert same_bits(y[i, :ln[i]], solo[0]) and same_bits(y[i, ln[i]:], np.zeros_like(y[i, ln[i]:])), i


def check_round_trip(dev):
    gl = griffin_lim(dev, **SMALL8)
    c = measured_c()
    n_fft = 256
    for T in (33, 70):
        x = wave(T)
        planar, fl = gl.stft(x, planar=True)
        y, ln = gl.istft(planar, fl)
        z = planar.cpu().numpy().astype(np.float64)
        D = z[0, :, 0] + 1j * z[0, :, 1]
        spread, env = _cover(SMALL, T)
        moved = spread(c['stft'] * stft_unit(x, SMALL) * 2.0 * (n_fft + 2) / n_fft) / env
        _within('round trip, T = %d' % T, y[0].cpu().numpy(), x[:25 * (T - 1)].astype(np.float64),
                c['istft'] * istft_unit(D, SMALL) + moved)


# ---- 4: the projection --------------------------------------------------------------------------------------------------------
def _raw_stft(gl, y, mode, out, mag=None, prev=None, alpha=0.0):
    x = torch.from_numpy(np.ascontiguousarray(y[None])).to(out.device)
    ln = torch.tensor([len(y)], dtype=torch.int32).to(out.device)
    gl._stft(x, ln, out.shape[1], mode, out, mag=mag, prev=prev, alpha=alpha)
    return out


def check_project(dev):
    """``complex``, then ``project`` on the same waveform: the output against mag z / |z| in float64 from the kernel's own z"""
    gl = griffin_lim(dev, **SMALL8)
    T, F = 40, 129
    y = wave(T, 7)
    y[400:] = 0.0                                                              # frames 22 .. : all-zero spans, z == 0 exactly
    z = _raw_stft(gl, y, 0, torch.empty((1, T, 2, F), dtype=torch.float32).to(dev)).cpu().numpy().astype(np.float64)[0]
    rng = np.random.default_rng(5)
    mag = (rng.random((1, T, F)) ** 4 * 30).astype(np.float32)
    mag[0, 3] = 0.0
    mg = torch.from_numpy(mag).to(dev)
    out = _raw_stft(gl, y, 1, torch.full((1, T, 2, F), np.nan, dtype=torch.float32).to(dev), mag=mg).cpu().numpy()[0]
    zc = z[:, 0] + 1j * z[:, 1]
    zero = zc == 0
    assert zero[22:].all() and not zero[:16].any()
    S = mag[0].astype(np.float64)
    t1 = np.where(zero, S, S * zc / np.where(zero, 1.0, np.abs(zc)))
    _within('project re', out[:, 0], t1.real, 4 * U * S + 1e-300)
    _within('project im', out[:, 1], t1.imag, 4 * U * S + 1e-300)
    assert same_bits(out[:, 0][zero], mag[0][zero]) and same_bits(out[:, 1][zero], np.zeros(int(zero.sum()), dtype=np.float32))
    # the momentum form, given z and t0
    t0 = (rng.standard_normal((1, T, 2, F)) * 3).astype(np.float32)
    prev = torch.from_numpy(t0.copy()).to(dev)
    a32 = float(np.float32(0.99))
    out2 = _raw_stft(gl, y, 1, torch.full((1, T, 2, F), np.nan, dtype=torch.float32).to(dev), mag=mg, prev=prev, alpha=0.99)
    out2, prev = out2.cpu().numpy()[0], prev.cpu().numpy()[0]
    assert same_bits(prev, out)                                                # prev holds t1: the bits of the plain projection
    for part, want in ((0, t1.real), (1, t1.imag)):
        d = want - t0[0, :, part].astype(np.float64)
        ref = want + a32 * d
        _within('project with momentum, part %d' % part, out2[:, part], ref, 4 * U * S * 1.99 + 2 * U * (np.abs(d) + np.abs(ref)) + 1e-300)


# ---- 5: Griffin-Lim runs ------------------------------------------------------------------------------------------------------
def _planar_start(S, phase):
    """the fp32 spectrum the loop starts from, as the host prepares it: float64, rounded once -> complex128 of those bits"""
    c = S * np.exp(2j * np.pi * phase)
    return c.real.astype(np.float32).astype(np.float64) + 1j * c.imag.astype(np.float32).astype(np.float64)


def check_first_inverse(dev):
    """iters = 0, no de-emphasis: istft(S angles) per element, for the three entry points' magnitudes"""
    conf, z = fixture()
    gl = griffin_lim(dev, griffin_lim_iters=8, **conf)
    ph = z['phase.0'].T
    for tag, x, mel in (('spectrogram', z['spectrogram'].T, False), ('mel', z['mel'].T, True)):
        x = x.astype(np.float32)                                               # (the features as the device takes them)
        S = amplitudes64(x, conf, 1.5, inv_mel=gl.inv_mel_basis() if mel else None)
        xs, lens = gl._features_in(torch.from_numpy(x), x.shape[1], None)
        Sd = gl.amplitudes(xs, mel=mel)
        assert np.abs(Sd[0].cpu().numpy() - S).max() <= 1e-12 * S.max()
        y, ln = gl.griffin_lim(Sd, lens, phase=ph[None], iters=0, deemphasis=False)
        D = _planar_start(Sd[0].cpu().numpy(), ph)
        _within('first inverse, ' + tag, y[0].cpu().numpy(), istft64(D, conf), measured_c()['istft'] * istft_unit(D, conf))


def _emph(y, a):
    return preemph64(np.asarray(y, dtype=np.float64), a)


def check_runs_converge(dev):
    """the three entry points from the fixture's phases, 8 iterations: sc within half the spread of the reference's 8 draws"""
    conf, z = fixture()
    a = conf['preemphasis']
    gl = griffin_lim(dev, griffin_lim_iters=8, **conf)
    S = amplitudes64(z['spectrogram'].T, conf)
    sc_draws = [spectral_convergence(_emph(z['draw.%d' % k], a), S, conf) for k in range(8)]
    margin = 0.5 * (max(sc_draws) - min(sc_draws))
    print('reference sc over 8 draws: %.4f .. %.4f, margin %.4f' % (min(sc_draws), max(sc_draws), margin))
    assert 0.2 < min(sc_draws) and max(sc_draws) < 0.32 and margin > 0.01
    ph = torch.from_numpy(z['phase.0'].T[None].copy())
    spec = torch.from_numpy(z['spectrogram'].T[None].astype(np.float32))
    mel = torch.from_numpy(z['mel'].T[None].astype(np.float32))
    Sm = amplitudes64(z['mel'].T, conf, inv_mel=gl.inv_mel_basis())
    runs = (('inv_spectrogram', gl.inv_spectrogram(spec, phase=ph), S),
            ('fast_inv_spectrogram', gl.fast_inv_spectrogram(spec, phase=ph), S),
            ('inv_mel_spectrogram', gl.inv_mel_spectrogram(mel, phase=ph), Sm))
    for name, (y, ln), mag in runs:
        assert y.shape == (1, 1500) and y.dtype == torch.float32 and ln.tolist() == [1500]
        y = y[0].cpu().numpy()
        assert np.isfinite(y).all()
        got, want = spectral_convergence(_emph(y, a), mag, conf), spectral_convergence(_emph(z[name], a), mag, conf)
        print('%s: sc %.5f, the reference from the same phases %.5f; waveform within %.3g of the reference'
              % (name, got, want, np.abs(y - z[name]).max()))
        assert abs(got - want) <= margin, (name, got, want, margin)


def check_sixty_iterations(dev):
    """the default 60 iterations at the small geometry, against the float64 restatement from the same phases"""
    conf, z = fixture()
    gl = griffin_lim(dev, **conf)
    assert gl.griffin_lim_iters == 60
    S = amplitudes64(z['spectrogram'].T, conf)
    sc = [spectral_convergence(griffin_lim64(S, np.random.RandomState(k).rand(129, 61).T, conf, 60), S, conf) for k in range(8)]
    margin = 0.5 * (max(sc) - min(sc))
    y, _ = gl.inv_spectrogram(torch.from_numpy(z['spectrogram'].T[None].astype(np.float32)), seed=0)
    got = spectral_convergence(_emph(y[0].cpu().numpy(), conf['preemphasis']), S, conf)
    print('60 iterations: sc %.5f, float64 from the same phases %.5f, 8 draws %.4f .. %.4f' % (got, sc[0], min(sc), max(sc)))
    assert abs(got - sc[0]) <= margin and got < 0.2


def check_real_geometry(dev):
    """21 frames at 2048 / 800 / 200, 2 iterations: the first inverse per element, the run by its sc against float64's 4 draws"""
    conf, z = fixture()
    rc = real_conf()
    gl = griffin_lim(dev, griffin_lim_iters=2, **rc)
    x = z['real.spectrogram'].T
    S = amplitudes64(x, rc)
    xs, lens = gl._features_in(torch.from_numpy(x.astype(np.float32)), 1025, None)
    phases = [np.random.RandomState(k).rand(1025, 21).T for k in range(4)]
    y0, _ = gl.griffin_lim(gl.amplitudes(xs), lens, seed=0, iters=0, deemphasis=False)
    D = _planar_start(gl.amplitudes(xs)[0].cpu().numpy(), phases[0])
    _within('first inverse, real geometry', y0[0].cpu().numpy(), istft64(D, rc), measured_c()['istft'] * istft_unit(D, rc))
    sc = [spectral_convergence(griffin_lim64(S, p, rc, 2), S, rc) for p in phases]
    y, ln = gl.inv_spectrogram(xs, seed=0)
    assert y.shape == (1, 4000) and ln.tolist() == [4000]
    got = spectral_convergence(_emph(y[0].cpu().numpy(), rc['preemphasis']), S, rc)
    print('real geometry, 2 iterations: sc %.5f, float64 %.5f, 4 draws %.4f .. %.4f' % (got, sc[0], min(sc), max(sc)))
    assert abs(got - sc[0]) <= 0.5 * (max(sc) - min(sc))


def check_ragged_run(dev):
    """a ragged batch with poisoned padding through 2 iterations of both loops: the bits of the solo runs, +0 behind"""
    gl = griffin_lim(dev, **dict(SMALL8, griffin_lim_iters=2))
    rng = np.random.default_rng(9)
    specs = [rng.uniform(-4, 4, (T, 129)).astype(np.float32) for T in RAGGED_FRAMES]
    batch = np.full((3, 70, 129), np.nan, dtype=np.float32)
    for i, s in enumerate(specs):
        batch[i, :len(s)] = s
    for fast in (False, True):
        y, ln = gl.inv_spectrogram(torch.from_numpy(batch), list(RAGGED_FRAMES), seed=4, fast=fast)
        y = y.cpu().numpy()
        assert ln.tolist() == [25 * (T - 1) for T in RAGGED_FRAMES]
        for i, s in enumerate(specs):
            solo = gl.inv_spectrogram(torch.from_numpy(s), seed=4 + i, fast=fast)[0].cpu().numpy()
            n = int(ln[i])
            assert np.isfinite(solo).all() and same_bits(y[i, :n], solo[0]) and same_bits(y[i, n:], np.zeros_like(y[i, n:])), (fast, i)


# ---- 6: de-emphasis -----------------------------------------------------------------------------------------------------------
def check_deemphasis(dev):
    gl = griffin_lim(dev, **SMALL8)
    c = measured_c()['deemph']
    for n in DEEMPH_LENGTHS:
        x = deemph_input(n)
        pad = np.full((2, n + 300), -7.25, dtype=np.float32)
        pad[0, :n], pad[1, :max(n // 2, 1)] = x, x[:max(n // 2, 1)]
        for in_place in (True, False):
            src = torch.from_numpy(pad.copy()).to(dev)
            dst = src if in_place else torch.full(pad.shape, 3.5, dtype=torch.float32).to(dev)
            out = gl.deemphasis(src, [n, max(n // 2, 1)], out=None if in_place else dst).cpu().numpy()
            ref = lfilter([1.0], [1.0, -0.97], x.astype(np.float64))
            _within('de-emphasis, %d samples%s' % (n, '' if in_place else ', out of place'), out[0, :n], ref,
                    c * U * np.abs(x).max() / 0.03)
            assert same_bits(out[1, :max(n // 2, 1)], out[0, :max(n // 2, 1)])      # the same samples, whatever the row
            fill = np.float32(-7.25 if in_place else 3.5)
            assert (out[0, n:] == fill).all() and (out[1, max(n // 2, 1):] == fill).all()
            if not in_place:
                assert same_bits(src.cpu().numpy(), pad)


# ---- 7: repeat, silence, refusals ---------------------------------------------------------------------------------------------
def check_repeat(dev):
    gl = griffin_lim(dev, **dict(SMALL8, griffin_lim_iters=3))
    spec = torch.from_numpy(np.random.default_rng(2).uniform(-4, 4, (2, 40, 129)).astype(np.float32))
    a, b = gl.fast_inv_spectrogram(spec, seed=1), gl.fast_inv_spectrogram(spec, seed=1)
    assert same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and len(gl._consts) == 1 and len(gl.features._consts) == 1


def check_silence(dev):
    gl = griffin_lim(dev, **dict(SMALL8, griffin_lim_iters=2))
    y = np.zeros(777, dtype=np.float32)
    z = gl.stft(y, planar=True)[0].cpu().numpy()
    assert same_bits(z, np.zeros((1, 32, 2, 129), dtype=np.float32))
    sp = gl.spectrogram(y)[0].cpu().numpy()
    assert same_bits(sp, np.full((1, 32, 129), -4.0, dtype=np.float32))
    w, ln = gl.istft(torch.zeros((1, 32, 2, 129)))
    assert same_bits(w.cpu().numpy(), np.zeros((1, 775), dtype=np.float32))
    dev_ = w.device
    w, ln = gl.griffin_lim(torch.zeros((1, 32, 129), dtype=torch.float64).to(dev_), [32], seed=0)
    assert same_bits(w.cpu().numpy(), np.zeros((1, 775), dtype=np.float32))


def _count(fn):
    from msmctts_amd.hip import lib
    h = lib.get()
    h.msmc_prof_enable(1)
    try:
        rc = fn()
        if torch.cuda.is_available() and lib.backend() != 'emu':
            torch.cuda.synchronize()
        return rc, h.msmc_prof_count()
    finally:
        h.msmc_prof_enable(0)


def check_refusals(dev):
    from msmctts_amd.hip import lib
    h = lib.get()
    t = lambda *s: torch.full(s, -7.25, dtype=torch.float32).to(dev)          # noqa: E731
    wav, out, mag, basis = t(1, 300), t(1, 13, 2, 129), t(1, 13, 129), torch.zeros((2, 112, 256)).to(dev)
    ln, fr = torch.tensor([300], dtype=torch.int32).to(dev), torch.tensor([13], dtype=torch.int32).to(dev)
    p, s = lib.ptr, lib.stream(wav)

    def stft(mode=0, L=300, n_fft=256, win=101, hop=25, B=1, mg=None, pv=None, w=wav, min_db=-100.0):
        return _count(lambda: h.msmc_stft(p(w), p(ln), p(basis), mode, p(out), p(mg), p(pv), 0.0, B, L, 13, n_fft, win, hop, 0.0,
                                          20.0, min_db, 4.0, 1, s))
    assert stft() == (0, 1) and not (out == -7.25).any()
    out.fill_(-7.25)
    for kw in (dict(mode=3), dict(mode=-1), dict(mode=1), dict(mode=0, mg=mag), dict(mode=2, pv=out), dict(L=128), dict(win=257),
               dict(win=0), dict(hop=0), dict(n_fft=255), dict(B=0), dict(w=None), dict(mode=2, min_db=0.0),
               dict(L=20000, n_fft=2048, win=2048, hop=2048)):           # (the last: a sample span beyond LDS)
        assert stft(**kw) == (E_SHAPE, 0), kw
    assert (out == -7.25).all()
    ib, wsq, y = torch.zeros((1, 272, 128)).to(dev), torch.zeros(101).to(dev), t(1, 300)

    def istft(T=13, n_fft=256, win=101, hop=25, B=1, sp=out):
        return _count(lambda: h.msmc_istft(p(sp), p(fr), p(ib), p(wsq), p(y), B, T, n_fft, win, hop, s))
    out.zero_()
    assert istft() == (0, 1) and not (y == -7.25).any()
    y.fill_(-7.25)
    # (a halo of 32 frames and more; a window beyond LDS)
    for kw in (dict(T=1), dict(win=257), dict(hop=0), dict(n_fft=255), dict(B=0), dict(sp=None), dict(win=101, hop=3),
               dict(n_fft=2048, win=1200, hop=300)):
        assert istft(**kw) == (E_SHAPE, 0), kw
    assert (y == -7.25).all()
    assert h.msmc_istft_tile(256, 101, 25) == 28 and h.msmc_istft_tile(2048, 800, 200) == 29 and h.msmc_istft_tile(256, 101, 3) == 0
    for kw in (dict(B=0), dict(L=0), dict(x=None)):
        a = dict(dict(B=1, L=300, x=y), **kw)
        assert _count(lambda: h.msmc_deemphasis(p(a['x']), p(y), p(ln), a['B'], a['L'], 0.97, s)) == (E_SHAPE, 0), kw
    assert (y == -7.25).all()
    # the host layer: ValueError with the offending value, before any launch
    gl = griffin_lim(dev, **SMALL8)

    def host():
        assert '125' in str(_raises(ValueError, lambda: gl.inv_spectrogram(torch.zeros(6, 129))))
        assert '125' in str(_raises(ValueError, lambda: gl.inv_mel_spectrogram(torch.zeros(2, 9, 20), [9, 6])))
        assert '128' in str(_raises(ValueError, lambda: gl.spectrogram(np.zeros(128, dtype=np.float32))))
        _raises(ValueError, lambda: gl.inv_spectrogram(torch.zeros(9, 20)))
        _raises(ValueError, lambda: gl.inv_spectrogram(torch.zeros(1, 9, 129), phase=torch.zeros(1, 9, 128)))
        _raises(ValueError, lambda: gl.istft(torch.zeros(1, 9, 129, dtype=torch.complex64), [10]))
        return 0
    assert _count(host) == (0, 0)
    assert '1200' in str(_raises(ValueError, lambda: griffin_lim(dev, **dict(fc.DEFAULTS, win_length=1200)).consts(dev)))
    gl7 = gl.inv_spectrogram(torch.zeros(7, 129), iters=1)                      # the shortest accepted: 150 samples
    assert gl7[0].shape == (1, 150)


def check_host_tensors_need_the_interpreter():
    from msmctts_amd.hip import lib
    saved = lib._host_pointers_ok
    lib._host_pointers_ok = False
    try:
        gl = griffin_lim('cpu', **SMALL8)
        for fn in (lambda: gl.spectrogram(fc.small_wave(400)), lambda: gl.inv_spectrogram(torch.zeros(9, 129)),
                   lambda: gl.istft(torch.zeros(1, 9, 2, 129)), lambda: gl.deemphasis(torch.zeros(1, 9), [9])):
            assert 'GPU only' in str(_raises(RuntimeError, fn))
    finally:
        lib._host_pointers_ok = saved


# ---- 8: the tools -------------------------------------------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def check_tools(dev, tmp_path):
    """extract_features --spectrogram, then invert_features --linear --seed: the wav file of the direct call"""
    import io
    import wave as wavfile
    from msmctts_amd.hip.griffin_lim import save_wav_pcm
    extract, invert = _tool('extract_features'), _tool('invert_features')
    src, feats, wavs = str(tmp_path / 'wav'), str(tmp_path / 'feats'), str(tmp_path / 'inv')
    os.makedirs(src)
    pcm = {'b_long': fc.int16_wave(), 'a_short': fc.int16_wave()[:431]}
    for uid, q in pcm.items():
        fc._write_wav(os.path.join(src, uid + '.wav'), q, 16000)
    gl = griffin_lim(dev, **dict(SMALL8, griffin_lim_iters=3))
    log = io.StringIO()
    extract.extract_dir(gl.features, src, feats, energy=False, jobs=2, out=log, spectrogram=gl)
    assert sorted(os.listdir(feats)) == ['mel', 'spec']
    assert invert.invert_dir(gl, feats, wavs, linear=True, seed=5, jobs=2, out=log)[0] == 2
    assert '2 files' in log.getvalue()
    for uid, q in pcm.items():
        sp = gl.spectrogram(q)[0][0].cpu().numpy()
        got = np.load(os.path.join(feats, 'spec', uid + '.npy'))
        assert got.dtype == np.float32 and same_bits(got, sp), uid
        y = gl.inv_spectrogram(torch.from_numpy(sp), seed=5)[0][0].cpu().numpy()
        with wavfile.open(os.path.join(wavs, uid + '.wav'), 'rb') as f:
            assert (f.getframerate(), f.getnchannels(), f.getsampwidth()) == (16000, 1, 2)
            data = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2')
        assert same_bits(data, save_wav_pcm(y)) and np.abs(data).max() >= 32766, uid
    # from the mel files, the fast loop, fewer iterations: files of the same lengths
    wavs2 = str(tmp_path / 'inv2')
    invert.invert_dir(gl, feats, wavs2, linear=False, fast=True, iters=1, seed=0, jobs=1, out=log)
    assert sorted(os.listdir(wavs2)) == ['a_short.wav', 'b_long.wav']
    # without the flag the outputs of extract_features are what they were
    feats2 = str(tmp_path / 'feats2')
    extract.extract_dir(gl.features, src, feats2, energy=False, jobs=2, out=log)
    assert sorted(os.listdir(feats2)) == ['mel']
    assert same_bits(np.load(os.path.join(feats2, 'mel', 'b_long.npy')), np.load(os.path.join(feats, 'mel', 'b_long.npy')))
    save = save_wav_pcm(np.array([0.001, -0.002]))
    assert save.tolist() == [int(0.001 * 32767 / 0.01), int(-0.002 * 32767 / 0.01)]


def check_config(tmp_path):
    import yaml
    from msmctts_amd.hip.griffin_lim import GriffinLim
    for conf in ({'num_mels': 40, 'griffin_lim_iters': 30, 'power': 1.2}, {'hparams': {'num_mels': 40, 'griffin_lim_iters': 30, 'power': 1.2}}):
        path = str(tmp_path / 'h.yaml')
        with open(path, 'w') as f:
            yaml.safe_dump(conf, f)
        gl = GriffinLim.from_config(yaml.safe_load(open(path)))
        assert (gl.features.num_mels, gl.griffin_lim_iters, gl.power, gl.n_fft, gl.win, gl.hop) == (40, 30, 1.2, 2048, 800, 200)
    gl = GriffinLim()
    assert (gl.griffin_lim_iters, gl.power) == (60, 1.5)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    for name in ('msmc_stft', 'msmc_istft', 'msmc_deemphasis', 'msmc_stft_tile', 'msmc_istft_tile'):
        assert name in lib.exported_symbols() and hasattr(lib.get(), name), name
    from msmctts_amd.hip.griffin_lim import GriffinLim
    from msmctts_amd.networks.vqgantts import msmc_vqgan_emb
    assert msmc_vqgan_emb.GriffinLim is GriffinLim and hasattr(msmc_vqgan_emb, 'FeatureExtractor')
    h = lib.get()
    assert [h.msmc_stft_tile(i) for i in range(4)] == [32, 128, 16, 256]
