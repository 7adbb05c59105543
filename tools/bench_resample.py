#!/usr/bin/env python
"""Runs ON the GPU box: ``Resampler.resample`` (msmctts_amd/hip/resample.py: msmc_resample, then msmc_peak_scale of
csrc/resample.hip) on B = 16 utterances of 10 s, stereo int16 at 44.1 kHz, resident on the device, to 24 kHz and to 16 kHz with the
default preset and -7 dBFS, beside two yardsticks:

  copy    a device-to-device copy that moves as many bytes as the two launches read and write (the input once, the output
          written once, read once and written again): what the job would cost were it bound by memory alone.
  cpu     scipy.signal.resample_poly in float64 with the same taps on the downmixed signal, then the peak scaling, in a pool of
          16 processes, one utterance per task.

    python tools/bench_resample.py [--rounds 5] [--out result.json]

Device times are host clocks around windows of calls that end in a device synchronise, after a warm-up; the window is sized to
about ``--window`` seconds.  The two launches are split out by the library's launch log (device events around each launch,
median over ``--rounds`` calls).  Prints per path the median over the rounds with the smallest and largest round, and one JSON
line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import numpy as np  # noqa: E402

B, SECONDS, RATE_IN, CHANNELS = 16, 10, 44100, 2
RATES_OUT = (24000, 16000)


def waveforms():
    """int16 [B, L, 2]: two harmonics of a voice-like tone plus noise, another level per channel"""
    rng = np.random.default_rng(4100)
    t = np.arange(SECONDS * RATE_IN) / float(RATE_IN)
    out = np.empty((B, len(t), CHANNELS), dtype=np.int16)
    for b in range(B):
        f0 = 110.0 + 9.0 * b
        y = 0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 3 * f0 * t) + 0.02 * rng.standard_normal(len(t))
        out[b, :, 0] = np.round(y * 20000.0)
        out[b, :, 1] = np.round(y * 12000.0 + 200.0 * rng.standard_normal(len(t)))
    return out


def _cpu_one(job):
    from scipy.signal import resample_poly
    from msmctts_amd.hip.resample import PRESETS, prototype_filter
    x, up, down = job
    h, _ = prototype_filter(up, down, **PRESETS['kaiser_best'])
    y = resample_poly(x.astype(np.float64).mean(axis=1) / 32768.0, up, down, window=h / up)
    return y * (10.0 ** (-7.0 / 20.0) / np.abs(y).max())


def cpu_pool(wavs, pairs, rounds):
    """rate -> seconds per batch in 16 processes (started before the GPU is opened)"""
    import multiprocessing as mp
    times = {rate: [] for rate in pairs}
    with mp.get_context('spawn').Pool(16) as pool:
        pool.map(_cpu_one, [(wavs[0][:4410], 80, 147)] * 16)                   # warm-up: imports
        for rate, (up, down) in pairs.items():
            for _ in range(rounds):
                t0 = time.perf_counter()
                pool.map(_cpu_one, [(w, up, down) for w in wavs])
                times[rate].append(time.perf_counter() - t0)
    return times


def launch_log(h, fn, rounds):
    """kernel name -> median device ms over ``rounds`` calls of fn, from the library's launch log"""
    import torch
    seen = {}
    for _ in range(rounds):
        h.msmc_prof_enable(1)
        try:
            fn()
            torch.cuda.synchronize()
            name, ms = ctypes.create_string_buffer(128), ctypes.c_float()
            for i in range(h.msmc_prof_count()):
                if h.msmc_prof_read(i, name, 128, ctypes.byref(ms)) == 0:
                    seen.setdefault(name.value.decode(), []).append(ms.value)
        finally:
            h.msmc_prof_enable(0)
    return {k: float(np.median(v)) for k, v in seen.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cpu-rounds', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.4, help='seconds of device work per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import msmctts_amd  # noqa: F401
    from msmctts_amd.hip.resample import Resampler
    wavs = waveforms()
    shapes = {rate: Resampler(RATE_IN, rate) for rate in RATES_OUT}
    cpu = cpu_pool(wavs, {rate: (rs.up, rs.down) for rate, rs in shapes.items()}, args.cpu_rounds) if args.cpu_rounds else {}

    import torch
    assert torch.cuda.is_available(), 'bench_resample.py measures on the GPU'
    from msmctts_amd.hip import lib
    x = torch.from_numpy(wavs).cuda()
    audio = B * SECONDS

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    result = {'B': B, 'seconds_each': SECONDS, 'rate_in': RATE_IN, 'channels': CHANNELS, 'device': torch.cuda.get_device_name(0)}
    for rate in RATES_OUT:
        rs = Resampler(RATE_IN, rate, device='cuda')
        Lo = rs.out_length(x.shape[1])
        moved = x.numel() * 2 + 3 * B * Lo * 4                                 # read x; write y; read and write y again
        src = torch.empty(moved // 2, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        paths = {'resample_and_normalise': lambda: rs.resample(x, norm_db=-7.0), 'resample_only': lambda: rs.resample(x),
                 'copy_of_the_same_bytes': lambda: dst.copy_(src)}
        iters, rounds = {}, {k: [] for k in paths}
        for k, fn in paths.items():
            window(fn, 3)                                                      # warm-up: code objects, the bank
            iters[k] = max(5, int(args.window / max(window(fn, 5), 1e-6)))
        for _ in range(args.rounds):
            for k, fn in paths.items():
                rounds[k].append(window(fn, iters[k]))
        launches = launch_log(lib.get(), paths['resample_and_normalise'], args.rounds)
        flop = 2.0 * B * Lo * rs.taps
        entry = {'up': rs.up, 'down': rs.down, 'taps_per_phase': rs.taps, 'bank_bytes': int(rs.bank().nbytes), 'out_samples': B * Lo,
                 'bytes_moved': moved, 'flop': flop, 'iters': iters, 'launch_ms': launches}
        print('44.1 -> %g kHz: %d / %d, %d taps per phase, bank %.0f KB, %.2f GFLOP, %.1f MB moved'
              % (rate / 1000.0, rs.up, rs.down, rs.taps, rs.bank().nbytes / 1024.0, flop / 1e9, moved / 1e6))
        for k, ts in list(rounds.items()) + ([('cpu16_resample_poly', cpu[rate])] if cpu else []):
            med = float(np.median(ts))
            entry[k] = {'us_per_batch_median': med * 1e6, 'us_min': min(ts) * 1e6, 'us_max': max(ts) * 1e6,
                        'audio_seconds_per_second': audio / med}
            print('  %-26s %12.1f us per batch (rounds %0.1f .. %0.1f), %10.0f audio-seconds/s'
                  % (k, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, audio / med))
        for name, ms in launches.items():
            print('  launch %-19s %12.1f us on the device' % (name, ms * 1e3))
        result[str(rate)] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
