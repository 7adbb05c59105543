#!/usr/bin/env python
"""Golden fixture for the spectrogram and the Griffin-Lim inverses (csrc/griffin_lim.hip, msmctts_amd/hip/griffin_lim.py),
generated from the reference itself.

    python tests/golden/make_golden_griffin_lim.py        # writes tests/golden/griffin_lim.npz

The unmodified reference ``examples/csmsc/scripts/audio/audio.py`` with its ``hparams.py`` is imported behind the shims of
``_ref_shims.install()`` (``librosa.filters.mel``: the Slaney restatement of oracle/audio.py) plus TWO stubs of this script's own,
``librosa.stft`` and ``librosa.istft``, which are not installed where this project is built.  Both are float64 numpy restatements
of what librosa computes with its defaults as the reference calls them: ``stft`` as in make_golden_features.py; ``istft(D,
hop_length, win_length)`` -- n_fft = 2 (rows - 1), ``irfft`` of every frame times the periodic Hann window of ``win_length``
samples zero-padded on both sides to n_fft, overlap-add at t hop, division by the summed squared windows where they exceed
``tiny`` (the smallest normal float32), n_fft // 2 trimmed at both ends.  So, as with the mel basis, THE TRANSFORMS THEMSELVES ARE
PINNED ONLY AGAINST RESTATEMENTS, not against librosa's code; everything around them -- pre-emphasis and its inverse
(``scipy.signal.lfilter``), ``_stft_parameters``, ``_amp_to_db`` / ``_db_to_amp``, ``_normalize`` / ``_denormalize``,
``_mel_to_linear`` with its ``np.linalg.pinv``, ``** power``, the loops of ``_griffin_lim`` and ``_fast_griffin_lim`` -- is the
reference's own code running.  ``np.complex`` (gone from numpy) is shimmed to ``complex``.  ``np.random`` is seeded before each
call, so the one draw a call makes, ``rand(*S.shape)``, is ``RandomState(seed).rand(F, T)``: stored for seed 0.

The reference's ``hparams`` object is set to the small geometry of the tests (num_freq 129, frame_shift_ms 1.5625,
frame_length_ms 6.3125 at 16 kHz: n_fft 256, hop 25, win 101; num_mels 20; griffin_lim_iters 8).  Stored for a noise-plus-two-tones
waveform of 1500 samples (float32, handed to the reference as float64): ``spectrogram(y)`` [F, T], ``melspectrogram(y)`` [M, T],
the phases of seed 0, the outputs of ``inv_spectrogram``, ``fast_inv_spectrogram`` and ``inv_mel_spectrogram`` from them,
``inv_spectrogram`` from the draws of seeds 0 .. 7 (``draw.k``; the phases of 1 .. 7 are regenerated from the seed), and the
pseudo-inverse the reference computed (float32 LAPACK on the float32 basis: the tests use it to follow ``inv_mel_spectrogram`` to
rounding, and compare their own float64 one with it).  At the real geometry (the reference's defaults) only ``spectrogram`` of the
feature fixture's ``wav.0`` (21 frames).  Data only; no reference source.  The archive is written with fixed member timestamps.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402
from make_golden_features import stft, write_npz  # noqa: E402

SMALL = dict(num_freq=129, frame_shift_ms=1.5625, frame_length_ms=6.3125, num_mels=20, griffin_lim_iters=8)
DRAWS = 8


def istft(stft_matrix, hop_length=None, win_length=None):
    """float64 restatement of librosa.istft with its defaults (see the module docstring)"""
    D = np.asarray(stft_matrix, dtype=np.complex128)
    n_fft = 2 * (D.shape[0] - 1)
    win_length = n_fft if win_length is None else win_length
    hop_length = win_length // 4 if hop_length is None else hop_length
    n = np.arange(win_length, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    left = (n_fft - win_length) // 2
    window = np.pad(window, (left, n_fft - win_length - left))
    frames = np.fft.irfft(D.T, n_fft, axis=1) * window[None, :]
    T = frames.shape[0]
    y = np.zeros(n_fft + hop_length * (T - 1))
    env = np.zeros_like(y)
    for t in range(T):
        y[t * hop_length:t * hop_length + n_fft] += frames[t]
        env[t * hop_length:t * hop_length + n_fft] += window * window
    ok = env > np.finfo(np.float32).tiny
    y[ok] /= env[ok]
    return y[n_fft // 2:n_fft // 2 + hop_length * (T - 1)]


def waveform():
    rng = np.random.default_rng(20240923)
    t = np.arange(1500, dtype=np.float64)
    y = 0.04 * rng.standard_normal(1500) + 0.3 * np.sin(2.0 * np.pi * 440.0 / 16000.0 * t) \
        + 0.15 * np.sin(2.0 * np.pi * 1720.0 / 16000.0 * t + 0.7)
    return y.astype(np.float32)


def main():
    _ref_shims.install()
    sys.modules['librosa'].stft = stft
    sys.modules['librosa'].istft = istft
    if not hasattr(np, 'complex'):
        np.complex = complex
    sys.path.insert(0, os.path.join(_ref_shims.REFERENCE_ROOT, 'examples', 'csmsc', 'scripts', 'audio'))
    import audio  # noqa: E402  (the reference's; finds its own hparams.py beside it)
    from hparams import hparams

    out = {}
    # the real geometry first (the reference's defaults): spectrogram of the feature fixture's first waveform
    wav0 = np.load(os.path.join(HERE, 'features.npz'))['wav.0']
    out['real.spectrogram'] = audio.spectrogram(wav0.astype(np.float64))
    assert audio._stft_parameters() == (2048, 200, 800) and out['real.spectrogram'].shape == (1025, 21)

    for k, v in SMALL.items():
        setattr(hparams, k, v)
    assert audio._stft_parameters() == (256, 25, 101), audio._stft_parameters()
    audio._mel_basis = audio._inv_mel_basis = None
    for k in ('num_mels', 'num_freq', 'sample_rate', 'frame_length_ms', 'frame_shift_ms', 'preemphasis', 'min_level_db',
              'ref_level_db', 'max_abs_value', 'symmetric_specs', 'griffin_lim_iters', 'power'):
        out['hparam.' + k] = np.asarray(getattr(hparams, k), dtype=np.float64)
    w = waveform()
    y = w.astype(np.float64)
    spec, mel = audio.spectrogram(y), audio.melspectrogram(y)
    assert spec.shape == (129, 61) and mel.shape == (20, 61)
    out['wav'], out['spectrogram'], out['mel'] = w, spec, mel
    out['phase.0'] = np.random.RandomState(0).rand(*spec.shape)

    def seeded(fn, arg, seed):
        np.random.seed(seed)
        res = fn(arg.copy())
        assert res.dtype == np.float64 and res.shape == (25 * 60,)
        return res

    out['inv_spectrogram'] = seeded(audio.inv_spectrogram, spec, 0)
    out['fast_inv_spectrogram'] = seeded(audio.fast_inv_spectrogram, spec, 0)
    out['inv_mel_spectrogram'] = seeded(audio.inv_mel_spectrogram, mel.T, 0)
    out['inv_mel_basis'] = np.asarray(audio._inv_mel_basis)
    for k in range(DRAWS):
        out['draw.%d' % k] = seeded(audio.inv_spectrogram, spec, k)
    assert np.array_equal(out['draw.0'], out['inv_spectrogram'])
    path = os.path.join(HERE, 'griffin_lim.npz')
    write_npz(path, out)
    print('wrote griffin_lim.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
