#!/usr/bin/env python
"""Turns feature files back into waveforms by Griffin-Lim on the gfx950 kernels (``GriffinLim``, msmctts_amd/hip/griffin_lim.py):
what the reference does per file on librosa with ``audio.inv_mel_spectrogram`` / ``inv_spectrogram`` / ``fast_inv_spectrogram``
and ``save_wav`` -- how one listens to a mel without a trained vocoder.

    python tools/invert_features.py feat_dir -o wav_dir [--linear] [--fast] [--iters N] [--seed S] [--jobs B] [--config yaml]

Reads ``feat_dir/mel/<id>.npy`` (float32 [T, num_mels], what tools/extract_features.py writes) or, with ``--linear``,
``feat_dir/spec/<id>.npy`` (float32 [T, num_freq], ``extract_features.py --spectrogram``).  The files are sorted by length and
``--jobs B`` of them share the launches; a file's waveform does not depend on its batch: its initial phases are
``RandomState(seed).rand(num_freq, T)``, the reference's draw after ``np.random.seed(seed)``.  ``--fast``: the momentum loop of
``_fast_griffin_lim``.  ``--iters``: iterations (default: ``griffin_lim_iters`` of the config, else 60).  Writes
``wav_dir/<id>.wav``, 16-bit mono at ``sample_rate``, scaled as the reference's ``save_wav`` scales (the peak at 32767).
``--config``: the yaml file tools/extract_features.py takes, which may also name ``griffin_lim_iters`` and ``power``.  A file of
too few frames for the iteration's reflect padding (``hop (T - 1) <= n_fft / 2``) is refused by name before anything is written.
Prints the files, frames and seconds of audio per second of wall time, reading and writing included.
"""
import argparse
import os
import sys
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402


def write_wav(path, pcm, rate):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype='<i2').tobytes())


def invert_dir(gl, feat_dir, output_dir, linear=False, fast=False, iters=None, seed=0, jobs=16, out=sys.stdout):
    """-> (files, frames, samples).  ``gl``: a ``GriffinLim``."""
    import torch
    from msmctts_amd.hip.griffin_lim import save_wav_pcm
    sub, width = ('spec', gl.num_freq) if linear else ('mel', gl.features.num_mels)
    src = os.path.join(feat_dir, sub)
    names = sorted(n for n in os.listdir(src) if n.endswith('.npy')) if os.path.isdir(src) else []
    if not names:
        raise ValueError('%s holds no .npy file' % src)
    items = []
    for n in names:
        x = np.load(os.path.join(src, n))
        if x.ndim != 2 or x.shape[1] != width:
            raise ValueError('%s: expected [T, %d], got %s' % (os.path.join(src, n), width, x.shape))
        if gl.hop * (x.shape[0] - 1) <= gl.n_fft // 2:
            raise ValueError('%s: %d frames give %d samples, Griffin-Lim needs more than n_fft / 2 = %d'
                             % (os.path.join(src, n), x.shape[0], gl.hop * (x.shape[0] - 1), gl.n_fft // 2))
        items.append((n[:-4], x.astype(np.float32)))
    os.makedirs(output_dir, exist_ok=True)
    items.sort(key=lambda it: (len(it[1]), it[0]))
    start = time.time()
    frames = samples = 0
    for first in range(0, len(items), jobs):
        batch = items[first:first + jobs]
        lens = [len(x) for _, x in batch]
        feats, phase = np.zeros((len(batch), max(lens), width), dtype=np.float32), np.zeros((len(batch), max(lens), gl.num_freq))
        for b, (_, x) in enumerate(batch):
            feats[b, :lens[b]] = x
            phase[b, :lens[b]] = np.random.RandomState(seed).rand(gl.num_freq, lens[b]).T
        fn = gl.inv_spectrogram if linear else gl.inv_mel_spectrogram
        wav, length = fn(torch.from_numpy(feats), lens, phase=torch.from_numpy(phase), iters=iters, fast=fast)
        wav, length = wav.cpu().numpy(), length.cpu().tolist()
        for b, (uid, _) in enumerate(batch):
            write_wav(os.path.join(output_dir, uid + '.wav'), save_wav_pcm(wav[b, :int(length[b])]), gl.features.sample_rate)
            frames, samples = frames + lens[b], samples + int(length[b])
    took = max(time.time() - start, 1e-9)
    print('%d files, %d frames, %.1f s of audio in %.3f s: %.1f files/s, %.1f audio-seconds/s'
          % (len(items), frames, samples / gl.features.sample_rate, took, len(items) / took,
             samples / gl.features.sample_rate / took), file=out)
    return len(items), frames, samples


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('feat_dir')
    ap.add_argument('-o', '--output-dir', required=True)
    ap.add_argument('--linear', action='store_true', help='read spec/<id>.npy (linear spectrograms), not mel/<id>.npy')
    ap.add_argument('--fast', action='store_true', help='the momentum loop of _fast_griffin_lim')
    ap.add_argument('--iters', type=int, default=None, help='iterations (default: the config, else 60)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the initial phases')
    ap.add_argument('-j', '--jobs', type=int, default=16, help='utterances per launch')
    ap.add_argument('-c', '--config', default=None, help='yaml file with hparams (default: those of the reference)')
    ap.add_argument('--device', default='cuda', help='default: the current GPU')
    args = ap.parse_args(argv)
    if args.jobs < 1:
        ap.error('--jobs must be positive')
    from msmctts_amd.hip.griffin_lim import GriffinLim
    conf = {}
    if args.config is not None:
        import yaml
        with open(args.config) as f:
            conf = yaml.safe_load(f) or {}
    gl = GriffinLim.from_config(conf, device=args.device)
    return invert_dir(gl, args.feat_dir, args.output_dir, args.linear, args.fast, args.iters, args.seed, args.jobs)


if __name__ == '__main__':
    main()
