#!/usr/bin/env python
"""Golden fixture for the acoustic features (csrc/features.hip, msmctts_amd/hip/features.py), generated from the reference itself.

    python tests/golden/make_golden_features.py        # writes tests/golden/features.npz

The unmodified reference ``examples/csmsc/scripts/audio/audio.py`` with its ``hparams.py`` is imported behind the shims of
``_ref_shims.install()`` (``librosa.filters.mel``: the Slaney restatement of oracle/audio.py) plus ONE stub of this script's own:
``librosa.stft``, which is not installed where this project is built.  The stub is a float64 numpy restatement of what
``librosa.stft(y, n_fft, hop_length, win_length)`` computes with its defaults -- ``center=True``, reflect padding by n_fft // 2,
the periodic Hann window of ``win_length`` samples zero-padded on both sides to n_fft, ``rfft`` of every frame, [1 + n_fft // 2,
1 + len(y) // hop_length] complex.  So, as with the mel basis, THE STFT ITSELF IS PINNED ONLY AGAINST A RESTATEMENT, not against
librosa's code; everything around it -- pre-emphasis (``scipy.signal.lfilter``), ``_stft_parameters``, magnitude, ``_linear_to_mel``,
``_amp_to_db``, ``_normalize``, ``energy`` -- is the reference's own code running.

``audio.melspectrogram(y)`` and ``audio.energy(y)`` on three short waveforms (stored as float32, handed to the reference as
float64): noise + tone of 4000 samples, a pure tone of 3000 samples (leakage bins far below the peak), noise of
n_fft / 2 + 1 = 1025 samples -- the shortest librosa's reflect padding takes.  Stored: the waveforms, the hparams, the outputs
in float64 as the reference returns them (mel [num_mels, T], energy [T]).  Data only; no reference source.  The archive is
written with fixed member timestamps: running the script again gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402

HPARAM_NAMES = ('num_mels', 'num_freq', 'sample_rate', 'frame_length_ms', 'frame_shift_ms', 'preemphasis', 'min_level_db',
                'ref_level_db', 'max_abs_value', 'symmetric_specs')


def stft(y, n_fft=2048, hop_length=None, win_length=None):
    """float64 restatement of librosa.stft with its defaults (see the module docstring)"""
    win_length = n_fft if win_length is None else win_length
    hop_length = win_length // 4 if hop_length is None else hop_length
    y = np.asarray(y, dtype=np.float64)
    n = np.arange(win_length, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    left = (n_fft - win_length) // 2
    window = np.pad(window, (left, n_fft - win_length - left))
    padded = np.pad(y, n_fft // 2, mode='reflect')
    frames = 1 + (len(padded) - n_fft) // hop_length
    idx = hop_length * np.arange(frames)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(padded[idx] * window[None, :], axis=1).T


def waveforms(n_fft):
    rng = np.random.default_rng(20240611)
    t = np.arange(4000, dtype=np.float64)
    a = 0.05 * rng.standard_normal(4000) + 0.3 * np.sin(2.0 * np.pi * 440.0 / 16000.0 * t)
    b = 0.5 * np.sin(2.0 * np.pi * 1000.0 / 16000.0 * t[:3000] + 0.3)
    c = 0.1 * rng.standard_normal(n_fft // 2 + 1)
    return [w.astype(np.float32) for w in (a, b, c)]


def write_npz(path, arrays):
    """an .npz with fixed member timestamps (numpy.savez stamps the members with the time of day)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    _ref_shims.install()
    sys.modules['librosa'].stft = stft
    sys.path.insert(0, os.path.join(_ref_shims.REFERENCE_ROOT, 'examples', 'csmsc', 'scripts', 'audio'))
    import audio  # noqa: E402  (the reference's; finds its own hparams.py beside it)
    from hparams import hparams

    out = {'hparam.' + k: np.asarray(getattr(hparams, k), dtype=np.float64) for k in HPARAM_NAMES}
    n_fft, hop, win = audio._stft_parameters()
    out['geometry'] = np.asarray([n_fft, hop, win], dtype=np.int64)
    for i, w in enumerate(waveforms(n_fft)):
        y = w.astype(np.float64)
        mel, en = audio.melspectrogram(y), audio.energy(y)
        assert mel.dtype == np.float64 and mel.shape == (hparams.num_mels, 1 + len(y) // hop) and en.shape == mel.shape[1:]
        out['wav.%d' % i], out['mel.%d' % i], out['energy.%d' % i] = w, mel, en
    path = os.path.join(HERE, 'features.npz')
    write_npz(path, out)
    print('wrote features.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
