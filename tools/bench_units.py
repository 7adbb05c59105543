#!/usr/bin/env python
"""Runs ON the GPU box: the labels-only wide assignment (csrc/vq_assign.inc, msmc_vq_assign_wide) against the wide search it
shares its main loop with (msmc_vq_search_wide), and the unit kernels of csrc/units.hip.

  assign    d = 768 and d = 1024, K = 100 and K = 1000, N = 6400 and N = 2^20, with the distance and (``dist = NULL``) without.
            Both entry points are called directly on preallocated buffers -- no allocation, no wrapper -- in the same process, on
            the same inputs: ``--rounds`` rounds, each timing a block of calls of every variant in turn (alternated, so that a
            drift of the clocks or a neighbour's load hits all of them), device events around each block after a warm-up.
            Reported per variant: the median and the spread (min .. max) of the rounds' per-call times, and the assignment's
            median over the search's.  The yardstick is the search in this process, never an earlier run.
            Stores per frame: 8 d (quant, diff) + 8 for the search, 12 (8 without dist) for the assignment; both read 4 d.
            The labels of the two are compared at the timed size (they must be equal).
  units     msmc_units_collapse and msmc_units_usage (K = 1000, overwrite and accumulate) at B = 64, T = 2000 on labels with
            runs of geometric length (mean 4), the same way.

    python tools/bench_units.py [--quick] [--rounds R]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
from msmctts_amd.hip import lib, vq

dev = torch.device('cuda:0')
WIDTHS, CODES, FRAMES = (768, 1024), (100, 1000), (6400, 1 << 20)


def rounds_us(fns, calls, rounds):
    """{name: [us per call of every round]}: each round times a block of ``calls`` calls of every variant in turn"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / calls * 1e3)
    return out


def line(name, us):
    return '  %-28s %9.1f us  (%.1f .. %.1f over %d rounds)' % (name, statistics.median(us), min(us), max(us), len(us))


def assign(quick, rounds):
    gen = torch.Generator().manual_seed(0)
    dgen = torch.Generator(device=dev).manual_seed(0)             # (the frames are drawn on the card: 4 GiB at the largest size)
    for d in WIDTHS:
        for K in CODES:
            et, en = vq.vq_prepare(torch.randn(1, d, K, generator=gen).to(dev), frames=0)
            for N in FRAMES[:1] if quick else FRAMES:
                x = torch.randn(N, d, generator=dgen, device=dev)
                quant, diff = torch.empty_like(x), torch.empty_like(x)
                i0 = torch.empty(N, dtype=torch.int64, device=dev)
                i1, i2, dist = torch.empty_like(i0), torch.empty_like(i0), torch.empty(N, dtype=torch.float32, device=dev)
                st = lib.stream(x)
                # the launchers take N d 4 < 2^32: d = 1024 at N = 2^20 runs as two blocks of 2^19 frames, for every variant
                step = N if N * d * 4 < (1 << 32) else N // 2
                spans = [(s, s + step) for s in range(0, N, step)]

                def search():
                    for s, e in spans:
                        lib.call('msmc_vq_search_wide', lib.ptr(x[s:e]), lib.ptr(et), lib.ptr(en), lib.ptr(quant[s:e]), lib.ptr(diff[s:e]),
                                 lib.ptr(i0[s:e]), e - s, d, K, st)

                def labels(ind, dd):
                    for s, e in spans:
                        lib.call('msmc_vq_assign_wide', lib.ptr(x[s:e]), lib.ptr(et), lib.ptr(en), lib.ptr(ind[s:e]),
                                 None if dd is None else lib.ptr(dd[s:e]), e - s, d, K, st)

                fns = {'msmc_vq_search_wide': search, 'msmc_vq_assign_wide': lambda: labels(i1, dist),
                       'msmc_vq_assign_wide, no dist': lambda: labels(i2, None)}
                calls = 3 if quick else (500 if N <= 6400 else 4)
                us = rounds_us(fns, calls, rounds)
                assert torch.equal(i0, i1) and torch.equal(i0, i2), 'the labels of the two entry points differ'
                base = statistics.median(us['msmc_vq_search_wide'])
                print('d = %d, K = %d, N = %d (%d calls per block; labels equal):' % (d, K, N, calls))
                for name, v in us.items():
                    print(line(name, v) + ('' if name == 'msmc_vq_search_wide' else '   %.3f of the search' % (statistics.median(v) / base)),
                          flush=True)
                del x, quant, diff


def unit_kernels(quick, rounds):
    from msmctts_amd.hip import units
    B, T, K = 64, 2000, 1000
    gen = torch.Generator().manual_seed(1)
    runs = torch.randint(0, K, (B, T), generator=gen)
    keep = torch.rand(B, T, generator=gen) < 0.75                     # a frame repeats its predecessor's label: runs of mean 4
    idx = torch.where(keep, torch.zeros((), dtype=torch.int64), torch.arange(T).expand(B, T))
    ind = torch.gather(runs, 1, torch.cummax(idx, 1).values).to(dev)
    length = torch.randint(T // 2, T + 1, (B,), generator=gen).to(dev)
    out = (torch.empty_like(ind), torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int64, device=dev))
    counts = torch.zeros(K, dtype=torch.int64, device=dev)
    st = lib.stream(ind)
    fns = {
        'msmc_units_collapse': lambda: lib.call('msmc_units_collapse', lib.ptr(ind), lib.ptr(length), lib.ptr(out[0]), lib.ptr(out[1]),
                                                lib.ptr(out[2]), B, T, st),
        'msmc_units_usage': lambda: lib.call('msmc_units_usage', lib.ptr(ind), lib.ptr(length), lib.ptr(counts), B, T, K, 0, st),
        'msmc_units_usage, accumulate': lambda: lib.call('msmc_units_usage', lib.ptr(ind), lib.ptr(length), lib.ptr(counts), B, T, K, 1, st),
    }
    us = rounds_us(fns, 3 if quick else 200, rounds)
    u, du, n = units.collapse_units(ind, length)
    print('B = %d, T = %d, K = %d: %d valid frames in %d runs:' % (B, T, K, int(length.sum()), int(n.sum())))
    for name, v in us.items():
        print(line(name, v), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to measure without one'
    assign(args.quick, args.rounds)
    unit_kernels(args.quick, args.rounds)
