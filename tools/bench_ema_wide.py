#!/usr/bin/env python
"""Runs ON the GPU box: the EMA codebook update of one wide head (csrc/ema_wide.hip, ``vq_ema_update(wide=True)``) at
(d, K) in {(768, 500), (1024, 1000), (1024, 2000)} x N in {6 400, 51 200} frames (B utterances of T = 200 frames, lengths drawn
from [T / 2, T]), against the wide search of the same shape.

  update      ``vq_ema_update(..., wide=True)`` (msmc_vq_ema_wide_update: nine launches), device events around ``--calls`` calls
  search      ``vq_prepare`` + ``vq_search`` of the same frames on the same codebook (msmc_vq_search_wide), timed the same way
  kernels     the launches of one update one by one, from the library's own event pairs (msmc_prof_*): the three of
              ema_wide.hip (ew_mask_kernel, ew_cs_kernel, ew_apply_kernel) and the six of the statistics
  bytes       what the update must move -- the valid rows of x, 16 bytes of label per frame (read, masked copy written and read),
              and 16 d K for the sums read once, embed_avg read and written and embed written -- over the update time,
              against 6.3 TB/s (what a streaming read achieves on this chip)

Two warm-up rounds, then ``--rounds`` timed rounds in which update and search alternate; median / min per call.

    python tools/bench_ema_wide.py [--rounds 7] [--calls 20] [--quick]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
from msmctts_amd.hip import lib, vq

dev = torch.device('cuda:0')
STREAM_BYTES = 6.3e12
SHAPES, FRAMES, T = ((768, 500), (1024, 1000), (1024, 2000)), (6400, 51200), 200
OWN = ('ew_mask_kernel', 'ew_cs_kernel', 'ew_apply_kernel')


def event_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def kernel_breakdown(fn):
    """{kernel name: us} of the library's launches inside one call of ``fn``"""
    L = lib.get()
    torch.cuda.synchronize()
    L.msmc_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    buf, ms, out = ctypes.create_string_buffer(128), ctypes.c_float(), {}
    for i in range(L.msmc_prof_count()):
        assert L.msmc_prof_read(i, buf, 128, ctypes.byref(ms)) == 0
        name = buf.value.decode()
        out[name] = out.get(name, 0.0) + ms.value * 1e3
    L.msmc_prof_enable(0)
    return out


def one_shape(d, K, N, rounds, calls):
    B = N // T
    gen = torch.Generator(device=dev).manual_seed(d + K + N)
    true = torch.randn(K, d, device=dev, generator=gen)
    x = (true[torch.randint(0, K, (N,), device=dev, generator=gen)] + 0.5 * torch.randn(N, d, device=dev, generator=gen)).view(B, T, d)
    length = torch.randint(T // 2, T + 1, (B,), device=dev, generator=gen)
    embed = true.t().contiguous().unsqueeze(0)
    cs, ea = torch.ones(1, K, device=dev), embed.clone()
    state = {'ws': None}
    with torch.no_grad():
        et, en = vq.vq_prepare(embed, frames=N)
        ind = vq.vq_search(x, et, en, wide=True)[2]

        def update():
            state['ws'] = vq.vq_ema_update(x, ind, length, embed, cs, ea, 0.99, 1e-5, state['ws'], wide=True)

        def search():
            et, en = vq.vq_prepare(embed, frames=N)
            state['ind'] = vq.vq_search(x, et, en, wide=True)[2]

        pieces = {'update': update, 'search': search}
        times = {k: [] for k in pieces}
        for r in range(2 + rounds):
            for name, fn in pieces.items():
                t = event_us(fn, calls)
                if r >= 2:
                    times[name].append(t)
        valid = int(length.sum())
        byts = 4.0 * valid * d + 24.0 * N + 16.0 * d * K
        med = {k: statistics.median(v) for k, v in times.items()}
        print('d = %d, K = %d, N = %d (%d valid frames), %d calls per timed span' % (d, K, N, valid, calls))
        for name in pieces:
            print('  %-8s %9.1f / %9.1f us per call (median / min of %d)' % (name, med[name], min(times[name]), rounds))
        print('  update / search = %.2f; update moves %.1f MB -> %.2f TB/s, %.1f %% of 6.3 TB/s' % (
            med['update'] / med['search'], byts / 1e6, byts / med['update'] / 1e6, 100.0 * byts / STREAM_BYTES / (med['update'] * 1e-6)))
        parts = kernel_breakdown(update)
        print('  launches of ema_wide.hip (us, one call): ' + '  '.join('%s %.1f' % (k, parts.get(k, float('nan'))) for k in OWN))
        print('  launches of the statistics (us, one call): ' + '  '.join('%s %.1f' % kv for kv in parts.items() if kv[0] not in OWN),
              flush=True)
    vq._F32_OF['last'] = None


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20, help='calls between one pair of device events')
    ap.add_argument('--quick', action='store_true', help='d = 1024, K = 1000, N = 6400 only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to measure without one'
    print(torch.cuda.get_device_name(0))
    for d, K in (((1024, 1000),) if args.quick else SHAPES):
        for N in ((6400,) if args.quick else FRAMES):
            one_shape(d, K, N, args.rounds, args.calls)
            torch.cuda.empty_cache()
