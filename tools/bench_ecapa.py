#!/usr/bin/env python
"""Runs ON the GPU box: the speaker reference encoder's kernels (csrc/tdnn.hip) and the whole ECAPA_TDNN.

  kernels   every launch of relu_batch_norm / se_residual / attentive_stats_pool, forward + backward, at B = 16, T = 400, bf16
            (C = 256; the pooling at 3 x 256 = 768) from the library's own event pairs (msmc_prof_*), next to the algorithmic
            bytes of each pass
  encoder   ECAPA_TDNN(in_channels=80, channels=256) forward + backward in bf16 on the kernels next to ``use_hip = False`` (the
            stock-operator form, which runs in fp32), device events around blocks
            of calls, the two alternated, three rounds
"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
import torch.nn as nn
from msmctts_amd.hip import lib, tdnn as hiptdnn
from msmctts_amd.networks.vqgantts.tdnn import ECAPA_TDNN

dev = torch.device('cuda:0')
B, T, C = 16, 400, 256


def profiled(label, fn, byts, iters=50):
    L = lib.get()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    L.msmc_prof_enable(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    times, order = {}, []
    buf, ms = ctypes.create_string_buffer(128), ctypes.c_float()
    for i in range(L.msmc_prof_count()):
        assert L.msmc_prof_read(i, buf, 128, ctypes.byref(ms)) == 0
        k = buf.value.decode().split('<')[0]
        if k not in times:
            order.append(k)
        times.setdefault(k, []).append(ms.value * 1e3)
    L.msmc_prof_enable(0)
    print('%s: launch durations (event pairs, us; median / min over %d)' % (label, iters))
    for k in order:
        med = statistics.median(times[k])
        nb = byts.get(k, 0)
        print('  %-24s %7.1f / %7.1f us   %8d algorithmic bytes  %5.0f GB/s' % (k, med, min(times[k]), nb, nb / med / 1e3), flush=True)


def kernels():
    n, n3, sz = B * T * C, B * T * 3 * C, 2
    x = torch.randn(B, T, C, device=dev).bfloat16().requires_grad_(True)
    res = torch.randn(B, T, C, device=dev).bfloat16().requires_grad_(True)
    g = torch.randn(B, T, C, device=dev).bfloat16()
    bn = nn.BatchNorm1d(C).to(dev).train()
    profiled('relu_batch_norm %dx%dx%d bf16' % (B, T, C), lambda: hiptdnn.relu_batch_norm(x, bn).backward(g),
             {'rbn_stats_kernel': n * sz, 'rbn_norm_kernel': 2 * n * sz, 'rbn_bwd_stats_kernel': 2 * n * sz, 'rbn_bwd_apply_kernel': 3 * n * sz})
    l1, l2 = nn.Linear(C, C // 2).to(dev), nn.Linear(C // 2, C).to(dev)
    profiled('se_residual %dx%dx%d bf16' % (B, T, C), lambda: hiptdnn.se_residual(x, res, l1, l2).backward(g),
             {'se_sums_kernel': n * sz, 'se_scale_kernel': 3 * n * sz, 'se_gate_kernel': 4 * C * C, 'se_merge_kernel': 0})
    x3 = torch.randn(B, T, 3 * C, device=dev).relu().bfloat16().requires_grad_(True)
    a3 = torch.randn(B, T, 3 * C, device=dev).bfloat16().requires_grad_(True)
    go = torch.randn(B, 6 * C, device=dev)
    profiled('attentive_stats_pool %dx%dx%d bf16' % (B, T, 3 * C), lambda: hiptdnn.attentive_stats_pool(x3, a3).backward(go),
             {'asp_part_kernel': 2 * n3 * sz, 'asp_bwd_kernel': 4 * n3 * sz, 'asp_merge_kernel': 0})
    print('(se_sums_kernel runs twice per call -- forward reads x, backward g and x: 2 n sizeof; se_scale_kernel twice: the '
          'backward form reads g only: 2 n sizeof)')


def encoder(rounds=3, calls=20):
    x = torch.randn(B, T, 80, device=dev)
    cot = torch.randn(B, 192, device=dev)
    ms = {}
    models = {}
    for hip in (True, False):
        torch.manual_seed(0)
        m = ECAPA_TDNN(in_channels=80, embd_dim=192, channels=C).to(dev).train()
        m.use_hip, m.hip_dtype = hip, torch.bfloat16
        models[hip] = m

    def run(m):
        for p in m.parameters():
            p.grad = None
        (m(x) * cot).sum().backward()
    for m in models.values():
        for _ in range(3):
            run(m)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for hip, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                run(m)
            e1.record()
            torch.cuda.synchronize()
            ms.setdefault(hip, []).append(e0.elapsed_time(e1) / calls)
    print('ECAPA_TDNN(80 -> 192, channels %d) forward + backward, B = %d, T = %d, eager (ms per call, %d rounds of %d):' % (C, B, T, rounds, calls))
    print('  kernels (bf16 frames)    %s' % ' '.join('%.3f' % v for v in ms[True]))
    print('  use_hip = False (fp32)   %s' % ' '.join('%.3f' % v for v in ms[False]), flush=True)


if __name__ == '__main__':
    kernels()
    encoder()
