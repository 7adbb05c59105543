#!/usr/bin/env python
"""Runs ON the GPU box: ``PitchExtractor.extract`` (msmctts_amd/hip/pitch.py, one launch of csrc/pitch.hip) on the workload of
tools/bench_features.py -- B = 16 utterances of 10 s at the default geometry (16 kHz, window 800, hop 200, lags 32 .. 266) --
beside one baseline:

  cpu     the float64 numpy restatement of YIN (tests/_pitchcases.py ``restated``) in a pool of 16 processes, one utterance per
          task.  The reference has no F0 tracker to compare with.

    python tools/bench_pitch.py [--rounds 5] [--out result.json]

Device times are host clocks around windows of launches that end in a device synchronise, after a warm-up; the window is sized
to about ``--window`` seconds.  The audio is resident on the device: no wav reading, no upload.  Prints per path the median over
the rounds with the smallest and largest round, and one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd'), os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402

from bench_features import B, RATE, SECONDS, waveforms  # noqa: E402  (tools/ is the script's directory)


def _cpu_one(y):
    import _pitchcases as cases
    return cases.restated(y, cases.DEFAULTS)['pitch'].shape[0]


def cpu_pool(wavs, rounds):
    """seconds per batch of the float64 restatement in 16 processes (started before the GPU is opened)"""
    import multiprocessing as mp
    times = []
    with mp.get_context('spawn').Pool(16) as pool:
        pool.map(_cpu_one, wavs[:1] * 16)              # warm-up: imports
        for r in range(rounds):
            batch = [w + np.float32(1e-9 * (r + 1)) for w in wavs]             # (the restatement keeps its results per input)
            t0 = time.perf_counter()
            pool.map(_cpu_one, batch)
            times.append(time.perf_counter() - t0)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cpu-rounds', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.4, help='seconds of device work per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    wavs = waveforms()
    cpu = cpu_pool(wavs, args.cpu_rounds)

    import msmctts_amd  # noqa: F401
    import torch
    assert torch.cuda.is_available(), 'bench_pitch.py measures on the GPU'
    from msmctts_amd.hip.pitch import PitchExtractor
    ex = PitchExtractor(device='cuda')
    x = torch.from_numpy(np.stack(wavs)).cuda()
    T = x.shape[1] // ex.hop + 1

    def run_extract():
        return ex.extract(x)

    def run_all():
        return ex.extract(x, voiced=True, aperiodicity=True)

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    paths = {'extract': run_extract, 'extract_voiced_aperiodicity': run_all}
    iters, rounds = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        window(fn, 3)                                  # warm-up: code objects
        iters[k] = max(5, int(args.window / max(window(fn, 5), 1e-6)))
    for _ in range(args.rounds):
        for k, fn in paths.items():
            rounds[k].append(window(fn, iters[k]))
    voiced = float(run_all()[1].float().mean().item())
    audio = B * SECONDS
    flop = 3.0 * B * T * ex.win * (ex.tau_max + 1)
    result = {'B': B, 'seconds_each': SECONDS, 'frames': B * T, 'device': torch.cuda.get_device_name(0), 'iters': iters,
              'voiced_share': voiced, 'difference_flop': flop}
    for k, ts in list(rounds.items()) + [('cpu16', cpu)]:
        med = float(np.median(ts))
        result[k] = {'us_per_batch_median': med * 1e6, 'us_min': min(ts) * 1e6, 'us_max': max(ts) * 1e6,
                     'audio_seconds_per_second': audio / med}
        print('%-28s %12.1f us per batch (rounds %0.1f .. %0.1f), %10.0f audio-seconds/s'
              % (k, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, audio / med))
    print('difference function: %.2f GFLOP per batch (3 W (tau_max + 1) per frame), %.2f TFLOP/s in extract'
          % (flop / 1e9, flop / result['extract']['us_per_batch_median'] / 1e6))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
