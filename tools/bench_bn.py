#!/usr/bin/env python
"""Runs ON the GPU box: the BatchNorm kernels of the normalised quantiser (csrc/norm.hip msmc_bn_*).

  kernels   the four training launches at the product's size (N = 16 x 400 frames, C = 256, bf16 in, fp32 out) from the library's
            own event pairs (msmc_prof_*), and the whole forward + backward call next to the stock F.batch_norm on the transposed
            view (device events around 200 calls each, the two alternated, three rounds)
  step      the graphed bf16 train step of bench.py's configuration (bench.build) with ``norm: True`` next to ``norm: False``:
            ms per step from a host clock around synchronised blocks of replays, the two trainers alternated
"""
import ctypes
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
import torch.nn as nn
import torch.nn.functional as F
from msmctts_amd.hip import lib, norm

dev = torch.device('cuda:0')


def kernels(B=16, T=400, C=256, iters=50):
    L = lib.get()
    x = torch.randn(B, T, C, device=dev).bfloat16().requires_grad_(True)
    g = torch.randn(B, T, C, device=dev)
    bn = nn.BatchNorm1d(C, affine=False).to(dev).train()
    for _ in range(5):
        norm.batch_norm(x, bn, out_fp32=True).backward(g)
    torch.cuda.synchronize()
    L.msmc_prof_enable(1)
    for _ in range(iters):
        norm.batch_norm(x, bn, out_fp32=True).backward(g)
    torch.cuda.synchronize()
    times = {}
    buf, ms = ctypes.create_string_buffer(128), ctypes.c_float()
    for i in range(L.msmc_prof_count()):
        assert L.msmc_prof_read(i, buf, 128, ctypes.byref(ms)) == 0
        times.setdefault(buf.value.decode(), []).append(ms.value * 1e3)
    L.msmc_prof_enable(0)
    N = B * T
    byts = {'bn_stats_kernel': N * C * 2, 'bn_norm_kernel': N * C * (2 + 4), 'bn_bwd_stats_kernel': N * C * (2 + 4),
            'bn_bwd_apply_kernel': N * C * (2 + 4 + 2)}
    print('%d x %d bf16 in, fp32 out: launch durations (event pairs, us; median / min over %d)' % (N, C, iters))
    for name, v in times.items():
        key = name.split('<')[0]
        print('  %-24s %6.1f / %6.1f us   %5.0f GB/s of algorithmic bytes' % (key, statistics.median(v), min(v),
                                                                             byts.get(key, 0) / statistics.median(v) / 1e3), flush=True)

    def stock():
        y = F.batch_norm(x.transpose(1, 2), sbn.running_mean, sbn.running_var, None, None, True, 0.1, 1e-5).transpose(1, 2)
        y.backward(gb)
    sbn = nn.BatchNorm1d(C, affine=False).to(dev).train()
    gb = g.bfloat16()

    def ours():
        norm.batch_norm(x, bn, out_fp32=True).backward(g)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rnd in range(3):
        for name, fn in (('hip  batch_norm forward + backward (4 launches)', ours), ('stock F.batch_norm on the transposed view   ', stock)):
            for _ in range(10):
                fn()
            ev[0].record()
            for _ in range(200):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            print('  round %d  %s %7.1f us per call' % (rnd, name, ev[0].elapsed_time(ev[1]) * 1e3 / 200), flush=True)


def step(steps=30, rounds=3):
    import bench
    from msmctts_amd.synthetic import make_batch

    trainers = {}
    for flag in (False, True):
        class A(object):
            batch, frames, graph, dtype, no_autocast, exchange = 16, 400, True, 'bf16', False, 'serial'
            model_kw = dict(n_heads=4, embedding_sizes=64, norm=flag)
        cfg, tr = bench.build(A, dev, 0, 1)
        batch = make_batch(A.batch, A.frames, 80, 300, seed=1234, rank=0, device='cpu')
        lengths = batch['mel_length'].tolist()
        batch = {k: v.to(dev) for k, v in batch.items()}
        batch['mel_length_host'] = lengths
        tr.rng = random.Random(1234)
        for i in range(3):
            tr.train_step(batch, 10 + i)
        torch.cuda.synchronize()
        trainers[flag] = (tr, batch)
        print('norm=%s: captured, use_hip=%s' % (flag, tr.model.autoencoder.quantizer.use_hip), flush=True)
    it = 20
    for rnd in range(rounds):
        for flag in (False, True):
            tr, batch = trainers[flag]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(batch, it)
                it += 1
            torch.cuda.synchronize()
            print('  round %d  norm=%-5s %7.2f ms per graphed bf16 step (%d steps)' % (rnd, flag, (time.perf_counter() - t0) * 1e3 / steps, steps),
                  flush=True)


if __name__ == '__main__':
    torch.cuda.set_device(0)
    {'kernels': kernels, 'step': step}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
