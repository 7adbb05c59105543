#!/usr/bin/env python
"""Runs ON the GPU box: the streamed exact search (csrc/vq_stream.inc) on the shapes no resident kernel takes, next to the
stock-operator chain of the reference expression on the same tensors (matmul, norms, arg-max of the negated distance, gather,
diff), and -- on a shape where residency is possible -- next to msmc_vq_search.  Device events, an otherwise idle process;
profiles/vq_stream.md holds the tables."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
from msmctts_amd.hip import lib, vq

dev = torch.device('cuda:0')
NS = [int(v) for v in os.environ.get('NS', '6400,1048576').split(',')]


def timed(fn, N):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    iters = 20 if N <= 200000 else 5
    best = float('inf')
    for _ in range(3):                      # best of three event-timed batches
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        t.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(t) / iters * 1e3)
    return best


def stock_chain(x, embed):
    H, d, K = embed.shape
    quants, diffs, inds = [], [], []
    for h in range(H):
        flat = x[:, h * d:(h + 1) * d]
        dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ embed[h] + embed[h].pow(2).sum(0, keepdim=True)
        ind = (-dist).max(1)[1]
        q = torch.nn.functional.embedding(ind, embed[h].t())
        diffs.append((q - flat).pow(2))
        quants.append(flat + (q - flat))
        inds.append(ind)
    return torch.cat(quants, -1), sum(diffs) / H, torch.stack(inds, -1)


print('%-12s %9s | %-26s %10s | %-14s %10s | indices equal' % ('H x d x K', 'N', 'kernel', 'us', 'reference', 'us'))
for H, d, K, against in ((1, 256, 512, 'stock'), (2, 128, 512, 'stock'), (4, 64, 256, 'resident')):
    D = H * d
    g = torch.Generator().manual_seed(0)
    e = torch.randn(H, d, K, generator=g).to(dev)
    et, en = vq.vq_prepare(e, frames=0)
    for N in NS:
        x = torch.randn(N, D, generator=g).to(dev)
        out = vq.vq_search(x, et, en, stream_chunk=0)
        name = lib.get().msmc_vq_last_kernel().decode()
        us = timed(lambda: vq.vq_search(x, et, en, stream_chunk=0), N)
        if against == 'stock':
            ref = stock_chain(x, e)
            rus = timed(lambda: stock_chain(x, e), N)
            rname = 'stock chain'
        else:
            ref = vq.vq_search(x, et, en, shortlist=False)
            rname = lib.get().msmc_vq_last_kernel().decode()
            rus = timed(lambda: vq.vq_search(x, et, en, shortlist=False), N)
        same = float((out[2] == ref[2]).double().mean())
        print('%-12s %9d | %-26s %10.1f | %-14s %10.1f | %.6f' % ('%dx%dx%d' % (H, d, K), N, name, us, rname, rus, same))
        sys.stdout.flush()
        del x, out, ref
