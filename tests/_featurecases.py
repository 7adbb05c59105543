"""Shared cases of the acoustic features: csrc/features.hip (msmc_mel_features), its host side (msmctts_amd/hip/features.py
``FeatureExtractor``) and tools/extract_features.py.  tests/test_features_emu.py runs them on the kernel interpreter,
tests/test_gpu_features.py on the GPU.

References.  ``restated`` is the chain of the reference's audio.py (``melspectrogram`` / ``energy``) in float64 numpy: pre-emphasis,
reflect padding by n_fft / 2, frames, periodic Hann centred in n_fft, ``rfft``, magnitude, the Slaney basis (``mel_filterbank``:
the fp32 values ``MelLoss`` uses, as float64), dB, normalise and clip.  ``check_restatement`` pins it against
tests/golden/features.npz -- the reference's own code around a restated ``librosa.stft`` (tests/golden/make_golden_features.py) --
to 1e-9 absolute on the normalised mel and 1e-9 relative on the energy.

Tolerance of the kernel against ``restated`` (every element, none left out).  An absolute error d on a mel amplitude whose
float64 value is m moves 20 log10(max(1e-5, m)) by at most 20 / ln 10 * d / max(m, 1e-5) to first order, and the normalised
value by that times max_abs / |min_level_db|, doubled for symmetric specs: K d / max(m, 1e-5), K = 0.695 at the defaults.  For d:
a bin of the spectrum is a sum of ``win`` products frame[n] basis[n][f] with |basis| <= 1, so sequential fp32 summation leaves an
error whose scale is 2^-24 sqrt(win) |frame|_2 (the random-walk growth of ``win`` roundings of partial sums bounded by the frame's
l2 norm), the magnitude inherits it, and mel bin j adds these over its frequencies with the weights basis[j][f] >= 0:
    d_mel[t][j] = c 2^-24 sqrt(win) |windowed frame t|_2 sum_f basis[j][f]
    d_energy[t] = c 2^-24 sqrt(win) sqrt(F) |windowed frame t|_2            (an l2 norm over F bins of that error each)
c is MEASURED, never on the kernel: ``fp32_chain`` evaluates the same chain in fp32 numpy (the kernel's own fp32 constants, BLAS
products, fp32 epilogue) and ``measured_c`` takes the worst ratio of its difference from ``restated`` to the unit of the bound
(c = 1) over ALL inputs of the kernel tests of this file (the fixture's three waveforms at the real geometry, every
small-geometry length, the ragged batch, the variants), separately for the mel and the energy, and multiplies it by 8: an fp32
MFMA is one sequential fmaf chain over the taps, whose error grows like sqrt(n), where the blocked sums of a BLAS product grow
more slowly.  It is measured where the tests run (a BLAS differs from build to build).  Observed on the machine this was written
on (the table per input: profiles/features.md): worst mel ratio 5.404 (``preemphasis=0``; 1.97 / 2.58 / 0.61 on the fixture's
three waveforms) -> c_mel = 43.2; worst energy ratio 0.2434 -> c_energy = 1.95; in normalised units the fp32 chain was within
3.8e-6 of float64 on noise + tone and 4.0e-5 on the pure tone's leakage bins.  The mel ratios above 1 sit on bins far above the
floor, where the unit is tiny and the fp32 epilogue (log10 and the affine map, about 1e-6 normalised) is what differs.  The
kernel on an MI355X used at most 0.121 of its mel bound and 0.148 of its energy bound.
Silence, zero rows, the ragged batch against solo runs and the repeat are compared BIT FOR BIT.
"""
import os
import wave

import numpy as np
import torch

E_SHAPE = -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'features.npz')

DEFAULTS = dict(sample_rate=16000, num_mels=80, num_freq=1025, frame_length_ms=50, frame_shift_ms=12.5, preemphasis=0.97,
                min_level_db=-100, ref_level_db=20, max_abs_value=4.0, symmetric_specs=True)
# the small geometry: n_fft = 256 (F = 129: no multiple of a frequency tile), win = 101 (odd, no multiple of a tap slice), hop = 25
SMALL = dict(DEFAULTS, num_freq=129, num_mels=20, win_length=101, hop_length=25)
FRAME_TILE = 32


def _raises(exc, fn):
    """the exception ``fn()`` raises, which must be an ``exc``"""
    try:
        fn()
    except exc as err:
        return err
    raise AssertionError('%s was not raised' % exc.__name__)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def extractor(dev, **kw):
    from msmctts_amd.hip.features import FeatureExtractor
    return FeatureExtractor(device=dev, **kw)


def geometry(conf):
    """(n_fft, hop, win) by the reference's ``_stft_parameters``, with the tests' overrides"""
    n_fft = (conf['num_freq'] - 1) * 2
    hop = conf.get('hop_length') or int(conf['frame_shift_ms'] / 1000 * conf['sample_rate'])
    win = conf.get('win_length') or int(conf['frame_length_ms'] / 1000 * conf['sample_rate'])
    return n_fft, hop, win


def mel_basis(conf):
    from msmctts_amd.trainers.criterions.stft_loss import mel_filterbank
    return mel_filterbank(conf['sample_rate'], (conf['num_freq'] - 1) * 2, conf['num_mels'], 0, conf['sample_rate'] / 2.0)


def _normalise(S, conf):
    lo, top = conf['min_level_db'], conf['max_abs_value']
    if conf['symmetric_specs']:
        return np.clip((2 * top) * ((S - lo) / (-lo)) - top, -top, top)
    return np.clip(top * ((S - lo) / (-lo)), 0, top)


def _frames(y, conf, dt):
    """the windowed frames [T, win] of the pre-emphasised, reflect-padded waveform, in ``dt``"""
    n_fft, hop, win = geometry(conf)
    y = np.asarray(y).astype(dt)
    p = y.copy()
    p[1:] = y[1:] - dt(conf['preemphasis']) * y[:-1]
    padded = np.pad(p, n_fft // 2, mode='reflect')
    off = (n_fft - win) // 2
    idx = hop * np.arange(1 + len(y) // hop)[:, None] + off + np.arange(win)[None, :]
    return padded[idx]


def restated(y, conf):
    """float64: {'mel': normalised [T, M], 'energy': [T], 'amp': mel amplitudes [T, M], 'norm': |windowed frame|_2 [T]}"""
    n_fft, hop, win = geometry(conf)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    fr = _frames(y, conf, np.float64) * w[None, :]
    off = (n_fft - win) // 2
    full = np.zeros((fr.shape[0], n_fft))
    full[:, off:off + win] = fr
    mag = np.abs(np.fft.rfft(full, axis=1))
    amp = mag @ mel_basis(conf).astype(np.float64).T
    S = 20 * np.log10(np.maximum(1e-5, amp)) - conf['ref_level_db']
    return {'mel': _normalise(S, conf), 'energy': np.linalg.norm(mag, ord=2, axis=1), 'amp': amp,
            'norm': np.linalg.norm(fr, axis=1)}


def fp32_chain(y, conf):
    """the same chain in fp32 numpy, on the kernel's fp32 constants (window folded into the basis): (mel [T, M], energy [T])"""
    from msmctts_amd.hip.features import windowed_dft_basis
    n_fft, hop, win = geometry(conf)
    F = n_fft // 2 + 1
    b = windowed_dft_basis(n_fft, win, F, 1)[0]                                # one tile of F columns: [win, 2 F]
    fr = _frames(np.asarray(y, dtype=np.float32), conf, np.float32)
    re, im = fr @ b[:, :F], fr @ b[:, F:]
    mag = np.sqrt(re * re + im * im)
    amp = mag @ mel_basis(conf).T
    f32 = np.float32
    S = f32(20) * np.log10(np.maximum(f32(1e-5), amp)) - f32(conf['ref_level_db'])
    c32 = dict(conf, min_level_db=f32(conf['min_level_db']), max_abs_value=f32(conf['max_abs_value']))
    mel = _normalise(S, c32)
    assert mel.dtype == np.float32 and mag.dtype == np.float32
    return mel, np.sqrt(np.sum(mag * mag, axis=1, dtype=np.float32))


def bound_units(ref, conf):
    """the bounds at c = 1: (normalised mel [T, M], energy [T])"""
    n_fft, hop, win = geometry(conf)
    K = (2 if conf['symmetric_specs'] else 1) * conf['max_abs_value'] * 20 / (np.log(10) * abs(conf['min_level_db']))
    d = 2.0 ** -24 * np.sqrt(win) * ref['norm'][:, None] * mel_basis(conf).astype(np.float64).sum(axis=1)[None, :]
    return K * d / np.maximum(ref['amp'], 1e-5), 2.0 ** -24 * np.sqrt(win) * np.sqrt(n_fft // 2 + 1) * ref['norm']


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def fixture():
    z = np.load(GOLDEN)
    conf = {k: z['hparam.' + k].item() for k in DEFAULTS}
    for k in ('num_mels', 'num_freq', 'sample_rate'):
        conf[k] = int(conf[k])
    conf['symmetric_specs'] = bool(conf['symmetric_specs'])
    return conf, [z['wav.%d' % i] for i in range(3)], [(z['mel.%d' % i], z['energy.%d' % i]) for i in range(3)]


def small_wave(n, seed=0):
    """noise + a tone + a quiet stretch, fp32"""
    rng = np.random.default_rng(4100 + 7 * n + seed)
    t = np.arange(n, dtype=np.float64)
    y = 0.08 * rng.standard_normal(n) + 0.25 * np.sin(2.0 * np.pi * (300.0 + 40 * seed) / 16000.0 * t)
    y[n // 3:n // 3 + n // 8] *= 1e-3
    return y.astype(np.float32)


def _len_for(frames, rest):
    return (frames - 1) * 25 + rest


# name: samples.  T = 1 + L // 25 around the frame tile of 32, the shortest utterance (L = n_fft / 2 + 1 = 129: every frame
# touches both reflected edges), L % hop != 0 and == 0, three frame tiles
LENGTHS = {
    'T31 tile-1': _len_for(FRAME_TILE - 1, 7),
    'T32 tile': _len_for(FRAME_TILE, 0),
    'T33 tile+1': _len_for(FRAME_TILE + 1, 13),
    'shortest L129': 129,
    'T70 three tiles': _len_for(70, 24),
}
RAGGED = (757, 129, 1313)
VARIANTS = {
    'no preemphasis': dict(SMALL, preemphasis=0.0),
    'asymmetric': dict(SMALL, symmetric_specs=False),
    'mels80': dict(SMALL, num_mels=80),
}
VARIANT_LEN = 1013


def _conf_only(conf):
    return {k: v for k, v in conf.items() if k not in ('win_length', 'hop_length')}


def all_inputs():
    """every (waveform, configuration) a toleranced kernel test of this file uses: what ``measured_c`` covers"""
    conf, wavs, _ = fixture()
    out = [(w, conf) for w in wavs]
    out += [(small_wave(n), SMALL) for n in LENGTHS.values()]
    out += [(small_wave(n, 1 + i), SMALL) for i, n in enumerate(RAGGED)]
    out += [(small_wave(VARIANT_LEN, 5), c) for c in VARIANTS.values()]
    out += [(int16_wave().astype(np.float32) / np.float32(32768.0), SMALL)]
    return out


def int16_wave():
    return np.round(small_wave(VARIANT_LEN, 9) * 32767.0 / np.abs(small_wave(VARIANT_LEN, 9)).max() * 0.5).astype(np.int16)


_C = {}


def measured_c(verbose=True):
    """(c_mel, c_energy) = 8 x the worst ratio of |fp32 numpy chain - float64 restatement| to the bound's unit over ``all_inputs``"""
    if not _C:
        worst_m = worst_e = 0.0
        for y, conf in all_inputs():
            ref = restated(y, conf)
            mel32, en32 = fp32_chain(y, conf)
            um, ue = bound_units(ref, conf)
            rm, re_ = np.abs(mel32 - ref['mel']) / um, np.abs(en32 - ref['energy']) / ue
            worst_m, worst_e = max(worst_m, rm.max()), max(worst_e, re_.max())
        _C['c'] = (8 * worst_m, 8 * worst_e)
        if verbose:
            print('fp32 numpy chain against float64: worst mel ratio %.4g -> c_mel %.4g; worst energy ratio %.4g -> c_energy %.4g'
                  % (worst_m, 8 * worst_m, worst_e, 8 * worst_e))
    return _C['c']


# ---- 1: the restatement against the reference fixture -------------------------------------------------------------------------------------
def check_restatement():
    conf, wavs, outs = fixture()
    assert {k: conf[k] for k in DEFAULTS} == DEFAULTS and geometry(conf) == (2048, 200, 800)
    assert [len(w) for w in wavs] == [4000, 3000, 1025]
    for w, (mel, en) in zip(wavs, outs):
        ref = restated(w, conf)
        assert ref['mel'].shape == mel.T.shape and mel.dtype == np.float64
        dm, de = np.abs(ref['mel'] - mel.T).max(), (np.abs(ref['energy'] - en) / en).max()
        print('restatement against the reference fixture: mel %.3g absolute, energy %.3g relative' % (dm, de))
        assert dm <= 1e-9 and de <= 1e-9, (dm, de)


# ---- 2, 3, 7: the kernel against the restatement ----------------------------------------------------------------------------------------
def _compare(tag, mel, en, y, conf):
    ref = restated(y, conf)
    c_mel, c_en = measured_c()
    um, ue = bound_units(ref, conf)
    T = ref['mel'].shape[0]
    assert mel.shape == ref['mel'].shape and en.shape == (T,) and mel.dtype == en.dtype == np.float32, (tag, mel.shape, en.shape)
    dm, de = np.abs(mel.astype(np.float64) - ref['mel']), np.abs(en.astype(np.float64) - ref['energy'])
    print('%s: mel worst difference %.3g, worst share of its bound %.3g; energy %.3g, share %.3g'
          % (tag, dm.max(), (dm / (c_mel * um)).max(), de.max(), (de / (c_en * ue)).max()))
    assert np.isfinite(mel).all() and np.isfinite(en).all(), tag
    assert (dm <= c_mel * um).all(), '%s: %d of %d mel elements beyond their bound, worst %.3g of it' % (
        tag, int((dm > c_mel * um).sum()), dm.size, (dm / (c_mel * um)).max())
    assert (de <= c_en * ue).all(), '%s: %d of %d energies beyond their bound, worst %.3g of it' % (
        tag, int((de > c_en * ue).sum()), de.size, (de / (c_en * ue)).max())


def _solo(ex, y, **kw):
    mel, en, length = ex.extract(torch.from_numpy(np.asarray(y)), **kw)
    assert mel.shape[0] == 1 and length.tolist() == [1 + len(y) // ex.hop]
    return mel[0].cpu().numpy(), en[0].cpu().numpy()


def check_real_geometry(dev):
    """the fixture's three waveforms at 2048 / 800 / 200, M = 80, in one ragged batch"""
    conf, wavs, _ = fixture()
    ex = extractor(dev, **conf)
    assert (ex.n_fft, ex.win, ex.hop) == (2048, 800, 200)
    mel, en, length = ex.extract(wavs)
    assert length.tolist() == [21, 16, 6] and mel.shape == (3, 21, 80)
    mel, en = mel.cpu().numpy(), en.cpu().numpy()
    for i, w in enumerate(wavs):
        T = 1 + len(w) // 200
        _compare('real geometry, waveform %d' % i, mel[i, :T], en[i, :T], w, conf)
        assert not mel[i, T:].any() and not en[i, T:].any()


def check_length(dev, name):
    n = LENGTHS[name]
    ex = extractor(dev, **SMALL)
    assert (ex.n_fft, ex.win, ex.hop) == (256, 101, 25)
    y = small_wave(n)
    mel, en = _solo(ex, y)
    _compare(name, mel, en, y, SMALL)


def check_variant(dev, name):
    conf = VARIANTS[name]
    y = small_wave(VARIANT_LEN, 5)
    mel, en = _solo(extractor(dev, **conf), y)
    _compare(name, mel, en, y, conf)
    if name == 'asymmetric':
        assert mel.min() >= 0.0 and mel.max() <= 4.0
    if name == 'mels80':
        assert mel.shape[1] == 80


def check_int16(dev):
    """int16 PCM is scaled by 1 / 32768 on the host: the bits of the run on those fp32 values, within the bound of their restatement"""
    q = int16_wave()
    y = q.astype(np.float32) / np.float32(32768.0)
    ex = extractor(dev, **SMALL)
    mel, en = _solo(ex, q)
    mel_f, en_f = _solo(ex, y)
    assert same_bits(mel, mel_f) and same_bits(en, en_f)
    mel_d, _ = _solo(ex, y.astype(np.float64))
    assert same_bits(mel, mel_d)
    _compare('int16', mel, en, y, SMALL)


# ---- 4, 5: ragged batch, repeatability -------------------------------------------------------------------------------------------------
def check_ragged(dev):
    ex = extractor(dev, **SMALL)
    wavs = [small_wave(n, 1 + i) for i, n in enumerate(RAGGED)]
    mel, en, length = ex.extract(wavs)
    T = [1 + n // 25 for n in RAGGED]
    assert length.dtype == torch.int64 and length.tolist() == T and mel.shape == (3, max(T), 20) and en.shape == (3, max(T))
    mel, en = mel.cpu().numpy(), en.cpu().numpy()
    # a wider batch whose padding is NaN: nothing behind an utterance's own length is read
    wide = np.full((3, max(RAGGED) + 517), np.nan, dtype=np.float32)
    for i, w in enumerate(wavs):
        wide[i, :len(w)] = w
    mel_w, en_w, length_w = ex.extract(torch.from_numpy(wide), lengths=list(RAGGED))
    assert length_w.tolist() == T and same_bits(mel_w.cpu().numpy(), mel) and same_bits(en_w.cpu().numpy(), en)
    for i, w in enumerate(wavs):
        solo_mel, solo_en = _solo(ex, w)
        assert same_bits(mel[i, :T[i]], solo_mel) and same_bits(en[i, :T[i]], solo_en), i
        assert same_bits(mel[i, T[i]:], np.zeros_like(mel[i, T[i]:])) and same_bits(en[i, T[i]:], np.zeros_like(en[i, T[i]:])), i
        _compare('ragged %d' % i, mel[i, :T[i]], en[i, :T[i]], w, SMALL)
    track = ex.extract(wavs, energy_track=True)[1]
    assert track.shape == (3, max(T), 1) and same_bits(track[..., 0].cpu().numpy(), en)
    from msmctts_amd.hip import features
    assert features.energy_track(torch.from_numpy(en)).shape == (3, max(T), 1)
    assert ex.extract(wavs, energy=False)[1] is None and same_bits(ex.extract(wavs, energy=False)[0].cpu().numpy(), mel)


def check_repeat(dev):
    ex = extractor(dev, **SMALL)
    wavs = [small_wave(n, 1 + i) for i, n in enumerate(RAGGED)]
    a, b = ex.extract(wavs), ex.extract(wavs)
    assert same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())
    assert len(ex._consts) == 1                     # the constants were built once


# ---- 6: silence ----------------------------------------------------------------------------------------------------------------------------
def check_silence(dev):
    y = np.zeros(777, dtype=np.float32)
    for conf, level in ((SMALL, -4.0), (VARIANTS['asymmetric'], 0.0)):
        mel, en = _solo(extractor(dev, **conf), y)
        assert mel.shape == (32, 20) and same_bits(mel, np.full_like(mel, level)) and same_bits(en, np.zeros_like(en))


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------------
def _raw(dev, L, n_fft=256, win=101, hop=25, M=20, B=1, min_db=-100.0, top=4.0, null=None):
    """msmc_mel_features on sentinel-filled outputs -> (rc, outputs untouched?, launches logged)"""
    from msmctts_amd.hip import lib
    h = lib.get()
    fq, ks = h.msmc_mel_features_tile(1), h.msmc_mel_features_tile(2)
    F = n_fft // 2 + 1
    T = 1 + max(L, 0) // max(hop, 1)
    wav = torch.zeros((B, max(L, 1)), dtype=torch.float32).to(dev)
    ln = torch.full((B,), L, dtype=torch.int32).to(dev)
    basis = torch.zeros((-(-F // fq), -(-max(win, 1) // ks) * ks, 2 * fq), dtype=torch.float32).to(dev)
    melT = torch.zeros((-(-F // fq) * fq, 160), dtype=torch.float32).to(dev)
    mel = torch.full((B, T, max(M, 1)), -7.25, dtype=torch.float32).to(dev)
    en = torch.full((B, T), -7.25, dtype=torch.float32).to(dev)
    h.msmc_prof_enable(1)
    try:
        rc = h.msmc_mel_features(lib.ptr(wav) if null != 'wav' else None, lib.ptr(ln), lib.ptr(basis), lib.ptr(melT), lib.ptr(mel),
                                 lib.ptr(en), B, L, T, n_fft, win, hop, M, 0.97, 20.0, min_db, top, 1, lib.stream(wav))
        if dev != 'cpu':
            torch.cuda.synchronize()
        launches = h.msmc_prof_count()
    finally:
        h.msmc_prof_enable(0)
    return rc, bool((mel == -7.25).all() and (en == -7.25).all()), launches


def check_refusals(dev):
    assert _raw(dev, 300) == (0, False, 1)                                     # the accepted call launches once and writes
    for kw in (dict(L=128), dict(L=0), dict(L=300, M=129), dict(L=300, M=0), dict(L=300, win=257), dict(L=300, win=0),
               dict(L=300, hop=0), dict(L=300, n_fft=255, win=101), dict(L=300, B=0), dict(L=300, min_db=0.0),
               dict(L=300, top=0.0), dict(L=300, null='wav'),      # (the last: a sample span beyond LDS)
               dict(L=20000, n_fft=1024, win=1024, hop=1024)):
        assert _raw(dev, **kw) == (E_SHAPE, True, 0), kw
    # the host layer: ValueError with the offending value, before any launch
    from msmctts_amd.hip import lib
    ex = extractor(dev, **SMALL)
    h = lib.get()
    h.msmc_prof_enable(1)
    try:
        err = _raises(ValueError, lambda: ex.extract(np.zeros(128, dtype=np.float32)))
        assert '128' in str(err)
        err = _raises(ValueError, lambda: ex.extract([small_wave(400), np.zeros(77, dtype=np.float32)]))
        assert '77' in str(err)
        assert h.msmc_prof_count() == 0
    finally:
        h.msmc_prof_enable(0)
    assert '129' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, num_mels=129))))
    assert '257' in str(_raises(ValueError, lambda: extractor(dev, **dict(SMALL, win_length=257))))
    assert '1000' in str(_raises(ValueError, lambda: extractor(dev, **dict(DEFAULTS, num_freq=401, frame_length_ms=62.5))))
    _raises(TypeError, lambda: ex.extract(np.zeros(400, dtype=np.int32)))
    _raises(ValueError, lambda: ex.extract(torch.zeros(2, 400), lengths=[400]))


def check_host_tensors_need_the_interpreter():
    """without the interpreter build bound a host tensor raises as for every other operator"""
    from msmctts_amd.hip import lib
    saved = lib._host_pointers_ok
    lib._host_pointers_ok = False
    try:
        err = _raises(RuntimeError, lambda: extractor('cpu', **SMALL).extract(small_wave(400)))
        assert 'GPU only' in str(err)
    finally:
        lib._host_pointers_ok = saved


# ---- 9: the tool -------------------------------------------------------------------------------------------------------------------------
def _write_wav(path, pcm, rate):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype='<i2').tobytes())


def check_tool(dev, tmp_path):
    import importlib.util
    import io
    spec = importlib.util.spec_from_file_location('extract_features_tool', os.path.join(ROOT, 'tools', 'extract_features.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, dst = str(tmp_path / 'wav'), str(tmp_path / 'out')
    os.makedirs(src)
    pcm = {'b_long': int16_wave(), 'a_short': int16_wave()[:431]}
    for uid, q in pcm.items():
        _write_wav(os.path.join(src, uid + '.wav'), q, 16000)
    ex = extractor(dev, **SMALL)
    log = io.StringIO()
    assert tool.extract_dir(ex, src, dst, energy=True, jobs=2, out=log)[0] == 2
    assert '2 files' in log.getvalue() and 'audio-seconds/s' in log.getvalue()
    for uid, q in pcm.items():
        mel, en = _solo(ex, q)
        got_mel, got_en = np.load(os.path.join(dst, 'mel', uid + '.npy')), np.load(os.path.join(dst, 'energy', uid + '.npy'))
        assert got_mel.shape == (1 + len(q) // 25, 20) and got_en.shape == (1 + len(q) // 25,)
        assert same_bits(got_mel, mel) and same_bits(got_en, en), uid
    # the files are what the datasets' reader takes
    from msmctts_amd.datasets import readers
    assert readers.read_npy(os.path.join(dst, 'mel', 'a_short.npy'), shape_only=True) == (18, 20)
    # a file at another rate is refused by name, and nothing is written for the directory
    _write_wav(os.path.join(src, 'c_wrong_rate.wav'), pcm['a_short'], 22050)
    dst2 = str(tmp_path / 'out2')
    err = _raises(ValueError, lambda: tool.extract_dir(ex, src, dst2, energy=True, jobs=2, out=log))
    assert 'c_wrong_rate.wav' in str(err) and '22050' in str(err) and not os.path.exists(dst2)
    # without --energy no energy directory
    os.remove(os.path.join(src, 'c_wrong_rate.wav'))
    tool.extract_dir(ex, src, dst2, energy=False, jobs=1, out=log)
    assert sorted(os.listdir(dst2)) == ['mel'] and same_bits(np.load(os.path.join(dst2, 'mel', 'b_long.npy')),
                                                             np.load(os.path.join(dst, 'mel', 'b_long.npy')))


def check_tool_config(tmp_path):
    """--config: a yaml file naming some hparams, flat or under ``hparams``"""
    import yaml
    from msmctts_amd.hip.features import FeatureExtractor
    for conf in ({'num_mels': 40, 'symmetric_specs': False}, {'hparams': {'num_mels': 40, 'symmetric_specs': False}}):
        path = str(tmp_path / 'h.yaml')
        with open(path, 'w') as f:
            yaml.safe_dump(conf, f)
        ex = FeatureExtractor.from_config(yaml.safe_load(open(path)))
        assert (ex.num_mels, ex.symmetric_specs, ex.n_fft, ex.win, ex.hop) == (40, False, 2048, 800, 200)


# ---- 10 ----------------------------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    assert 'msmc_mel_features' in lib.exported_symbols() and hasattr(lib.get(), 'msmc_mel_features')
    from msmctts_amd.hip.features import FeatureExtractor
    from msmctts_amd.networks.vqgantts import msmc_vqgan_emb
    assert msmc_vqgan_emb.FeatureExtractor is FeatureExtractor and hasattr(msmc_vqgan_emb, 'fit_kmeans')
    ex = FeatureExtractor()
    assert (ex.n_fft, ex.win, ex.hop, ex.num_mels) == (2048, 800, 200, 80)
    h = lib.get()
    assert [h.msmc_mel_features_tile(i) for i in range(3)] == [FRAME_TILE, 128, 16]
