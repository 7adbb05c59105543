#!/usr/bin/env python
"""Runs ON the GPU box: ``GriffinLim.inv_spectrogram`` (msmctts_amd/hip/griffin_lim.py on csrc/griffin_lim.hip) on B = 16
utterances of 10 s at the default geometry (16 kHz, 2048 / 800 / 200), 60 iterations -- the workload of the other feature
profiles -- with each kernel timed alone against its own roofline, and one baseline:

  cpu     the float64 numpy restatement of ``_griffin_lim`` (tests/_griffinlimcases.py ``griffin_lim64``) in a pool of 16
          processes, one utterance per task: what the reference does per file, without librosa's own overheads.

    python tools/bench_griffin_lim.py [--rounds 5] [--cpu-iters 60] [--out result.json]

Device times are host clocks around windows of launches that end in a device synchronise, after a warm-up; the window is sized
to about ``--window`` seconds.  The spectrograms are resident on the device.  Rooflines: the fp32 MFMA rate (157.3 TFLOP/s) on the
MFMA work a launch issues (padded tiles and halo rows included; the useful share is printed beside it) and 6.3 TB/s measured
copy bandwidth on the bytes a launch must move.  Prints per path the median over the rounds with the smallest and largest round,
and one JSON line.
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
MFMA_FLOPS, COPY_BYTES = 157.3e12, 6.3e12


def spectrograms(T, F):
    """normalised dB spectrograms of a plausible spread (the values do not change the work)"""
    rng = np.random.default_rng(5)
    return rng.uniform(-3.5, 2.5, (B, T, F)).astype(np.float32)


def _cpu_one(args):
    import _featurecases as fc
    import _griffinlimcases as cases
    x, iters, seed = args
    S = cases.amplitudes64(x, fc.DEFAULTS)
    phase = np.random.RandomState(seed).rand(S.shape[1], S.shape[0]).T
    return cases.griffin_lim64(S, phase, fc.DEFAULTS, iters).shape[0]


def cpu_pool(specs, iters):
    """seconds per batch of the float64 restatement in 16 processes (started before the GPU is opened), one timed round"""
    import multiprocessing as mp
    with mp.get_context('spawn').Pool(16) as pool:
        pool.map(_cpu_one, [(x[:40], 1, 0) for x in specs])            # warm-up: imports, FFT plans
        t0 = time.perf_counter()
        pool.map(_cpu_one, [(x, iters, b) for b, x in enumerate(specs)])
        return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device work per timed window')
    ap.add_argument('--cpu-iters', type=int, default=60, help='iterations of the CPU baseline (0: skip it)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    n_fft, win, hop = 2048, 800, 200
    F, T = n_fft // 2 + 1, 1 + SECONDS * RATE // hop
    specs = spectrograms(T, F)
    cpu = cpu_pool(list(specs), args.cpu_iters) if args.cpu_iters > 0 else None

    import msmctts_amd  # noqa: F401
    import torch
    assert torch.cuda.is_available(), 'bench_griffin_lim.py measures on the GPU'
    from msmctts_amd.hip import lib
    from msmctts_amd.hip.griffin_lim import MODE_PROJECT, GriffinLim
    gl = GriffinLim(device='cuda')
    assert (gl.n_fft, gl.win, gl.hop) == (n_fft, win, hop)
    x = torch.from_numpy(specs).cuda()
    S = gl.amplitudes(x)
    mag = S.to(torch.float32).contiguous()
    L = hop * (T - 1)
    fr = torch.full((B,), T, dtype=torch.int32).cuda()
    ln = torch.full((B,), L, dtype=torch.int32).cuda()
    y, _ = gl.griffin_lim(S, [T] * B, seed=0, iters=1, deemphasis=False)
    c = torch.empty((B, T, 2, F), dtype=torch.float32).cuda()
    prev = torch.zeros_like(c)

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def iteration():
        gl._stft(y, ln, T, MODE_PROJECT, c, mag=mag)
        gl._istft(c, fr, y)

    paths = {
        'stft_project': lambda: gl._stft(y, ln, T, MODE_PROJECT, c, mag=mag),
        'stft_project_momentum': lambda: gl._stft(y, ln, T, MODE_PROJECT, c, mag=mag, prev=prev, alpha=0.99),
        'istft': lambda: gl._istft(c, fr, y),
        'iteration': iteration,
        'deemphasis': lambda: gl.deemphasis(y.clone(), ln),
        'batch_60_iterations': lambda: gl.inv_spectrogram(x, seed=0),
    }
    iters, rounds = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        window(fn, 2)                                  # warm-up: code objects, constants
        iters[k] = max(2, int(args.window / max(window(fn, 2), 1e-6)))
    for _ in range(args.rounds):
        for k, fn in paths.items():
            rounds[k].append(window(fn, iters[k]))
    h = lib.get()
    ft, fq, ks = (h.msmc_stft_tile(i) for i in range(3))
    pt = h.msmc_istft_tile(n_fft, win, hop)
    rows = B * -(-T // ft) * ft
    issued = {'stft_project': rows * (-(-win // ks) * ks) * (-(-F // fq) * fq) * 2 * 2.0,
              'istft': B * -(-(win // 2 + L) // (pt * hop)) * ft * (-(-2 * F // ks) * ks) * (-(-win // fq) * fq) * 2.0}
    useful = B * T * win * 2 * F * 2.0
    moved = {'stft_project': 4.0 * (B * L + 3 * B * T * F), 'istft': 4.0 * (B * L + 2 * B * T * F), 'deemphasis': 8.0 * B * L}
    result = {'B': B, 'seconds_each': SECONDS, 'frames': B * T, 'device': torch.cuda.get_device_name(0), 'iters': iters,
              'istft_positions_per_workgroup': pt}
    for k, ts in rounds.items():
        med = float(np.median(ts))
        result[k] = {'us_median': med * 1e6, 'us_min': min(ts) * 1e6, 'us_max': max(ts) * 1e6}
        note = ''
        if k in issued:
            result[k].update(gflop_issued=issued[k] / 1e9, gflop_useful=useful / 1e9, mfma_roofline_us=issued[k] / MFMA_FLOPS * 1e6,
                             share_of_mfma_peak=issued[k] / MFMA_FLOPS / med)
            note = ', %.1f GFLOP issued (%.1f useful): %.1f us at the MFMA rate, %.1f %% of it reached' % (
                issued[k] / 1e9, useful / 1e9, issued[k] / MFMA_FLOPS * 1e6, 100 * issued[k] / MFMA_FLOPS / med)
        if k in moved:
            result[k].update(mbytes=moved[k] / 1e6, copy_roofline_us=moved[k] / COPY_BYTES * 1e6)
            note += ', %.1f MB to move: %.1f us at copy bandwidth' % (moved[k] / 1e6, moved[k] / COPY_BYTES * 1e6)
        print('%-22s %11.1f us (rounds %0.1f .. %0.1f)%s' % (k, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, note))
    batch = result['batch_60_iterations']['us_median'] / 1e6
    print('batch of %d x %d s, %d iterations: %.3f s, %.0f audio-seconds/s' % (B, SECONDS, gl.griffin_lim_iters, batch,
                                                                                B * SECONDS / batch))
    if cpu is not None:
        result['cpu16'] = {'s_per_batch': cpu, 'iters': args.cpu_iters}
        print('float64 numpy restatement, 16 processes, %d iterations: %.2f s per batch (%.1f x the device batch at 60)'
              % (args.cpu_iters, cpu, cpu * 60.0 / args.cpu_iters / batch))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
