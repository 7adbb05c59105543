#!/usr/bin/env python
"""Runs ON the GPU box: ``FeatureExtractor.extract`` (msmctts_amd/hip/features.py, one launch of csrc/features.hip) on B = 16
utterances of 10 s at the default geometry (16 kHz, 2048 / 800 / 200, 80 mels), against two baselines:

  chain   this tree's loss-side spectral kernels given the same window: ``msmc_stft_frames_fwd`` (the frames written to memory),
          the constant DFT GEMM, ``spec_mag`` and the mel projection GEMM (hip/spectral.py).  It has no pre-emphasis, dB or
          normalisation step and no energy: it does LESS than ``extract``.
  cpu     the float64 numpy restatement of the chain (tests/_featurecases.py ``restated``) in a pool of 16 processes, one
          utterance per task: what the reference's process pool does, without librosa's own overheads.

    python tools/bench_features.py [--rounds 5] [--out result.json]

Device times are host clocks around windows of launches that end in a device synchronise, after a warm-up; the two device paths
alternate within every round and the window is sized to about ``--window`` seconds.  The audio is resident on the device: no
wav reading, no upload.  Prints per path the median over the rounds with the smallest and largest round, and one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd'), os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402

B, SECONDS, RATE = 16, 10, 16000


def waveforms():
    rng = np.random.default_rng(5)
    t = np.arange(SECONDS * RATE, dtype=np.float64)
    return [(0.05 * rng.standard_normal(t.size) + 0.2 * np.sin(2 * np.pi * (200.0 + 30 * i) / RATE * t)).astype(np.float32)
            for i in range(B)]


def _cpu_one(y):
    import _featurecases as cases
    r = cases.restated(y, cases.DEFAULTS)
    return r['mel'].shape[0]


def cpu_pool(wavs, rounds):
    """seconds per batch of the float64 restatement in 16 processes (started before the GPU is opened)"""
    import multiprocessing as mp
    times = []
    with mp.get_context('spawn').Pool(16) as pool:
        pool.map(_cpu_one, wavs)                       # warm-up: imports, FFT plans
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(_cpu_one, wavs)
            times.append(time.perf_counter() - t0)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.4, help='seconds of device work per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    wavs = waveforms()
    cpu = cpu_pool(wavs, args.rounds)

    import msmctts_amd  # noqa: F401
    import torch
    assert torch.cuda.is_available(), 'bench_features.py measures on the GPU'
    from msmctts_amd.hip import spectral
    from msmctts_amd.hip.features import FeatureExtractor
    from msmctts_amd.trainers.criterions.stft_loss import MelLoss
    ex = FeatureExtractor(device='cuda')
    x = torch.from_numpy(np.stack(wavs)).cuda()
    loss = MelLoss(ex.n_fft, ex.hop, ex.win, RATE, ex.num_mels)
    dft, mel = loss._consts(x.device)
    F = ex.n_fft // 2 + 1
    T = x.shape[1] // ex.hop + 1

    def run_extract():
        return ex.extract(x)

    def run_chain():
        with torch.no_grad():
            fr = spectral._Frames.apply(x, T, dft[3], spectral._pad4(dft[3]), ex.hop, ex.n_fft // 2 - dft[2])
            spec = spectral._ConstGemm.apply(fr, dft[0], dft[1], False)
            mag = spectral._SpecMag.apply(spec, F, spectral._pad4(F), 1e-9, 0)
            return spectral._ConstGemm.apply(mag, mel[0], mel[1], False)

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    paths = {'extract': run_extract, 'chain': run_chain}
    iters, rounds = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        window(fn, 3)                                  # warm-up: code objects, constants
        iters[k] = max(5, int(args.window / max(window(fn, 5), 1e-6)))
    for _ in range(args.rounds):
        for k, fn in paths.items():
            rounds[k].append(window(fn, iters[k]))
    audio = B * SECONDS
    result = {'B': B, 'seconds_each': SECONDS, 'frames': B * T, 'device': torch.cuda.get_device_name(0), 'iters': iters}
    for k, ts in list(rounds.items()) + [('cpu16', cpu)]:
        med = float(np.median(ts))
        result[k] = {'us_per_batch_median': med * 1e6, 'us_min': min(ts) * 1e6, 'us_max': max(ts) * 1e6,
                     'audio_seconds_per_second': audio / med}
        print('%-8s %10.1f us per batch (rounds %0.1f .. %0.1f), %10.0f audio-seconds/s'
              % (k, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, audio / med))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
