#!/usr/bin/env python
"""Runs ON the GPU box: compute_triple_loss forward + backward through the gfx950 kernels (csrc/triple_stream.inc where no head's
codebook fits LDS, the resident triple_loss_kernel for scale) next to the stock operator chain the modules fall back to, on the
same tensors, interleaved call by call in one process.  N = the frames per stage of BASELINE config #4 at B = 64 (6 400 at the
coarse stage, 25 600 at the fine one).  Device events around every call, median of the timed calls after a warm-up, an otherwise
idle process; profiles/triple_stream.md holds the table."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
from msmctts_amd.hip import lib, losses, vq

dev = torch.device('cuda:0')
NS = [int(v) for v in os.environ.get('NS', '6400,25600').split(',')]
ROUNDS = int(os.environ.get('ROUNDS', '30'))


def stock(p, trg, embed, reduction):
    """the chain of Quantize.compute_triple_loss per head, and the head mean"""
    H, d, K = embed.shape
    out = []
    for h in range(H):
        flat = p[:, h * d:(h + 1) * d]
        e = embed[h]
        dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ e + e.pow(2).sum(0, keepdim=True)
        pos = torch.nn.functional.mse_loss(flat, torch.nn.functional.embedding(trg[:, h], e.t()), reduction='none').sum(-1)
        triple = pos.unsqueeze(-1) - dist
        triple = (triple != 0) * (torch.clamp(triple + 1e-6, min=0) / d)
        out.append(triple.mean(-1) if reduction == 'mean' else triple.sum(-1))
    return sum(out) / H


def kernel(p, trg, et, en, reduction):
    return losses.triple_loss(p, trg, et, en, reduction).sum(-1) / en.shape[0]


def one(fn, p, w):
    p.grad = None
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    (fn(p) * w).sum().backward()
    t.record()
    return s, t


print('%-12s %7s | %-26s %9s %9s | %-12s %9s | ratio | max |dloss| max |dgrad|' %
      ('H x d x K', 'N', 'kernel', 'us', 'MB', 'reference', 'us'))
for H, d, K in ((1, 256, 512), (2, 128, 512), (4, 64, 256)):
    D = H * d
    g = torch.Generator().manual_seed(0)
    embed = torch.randn(H, d, K, generator=g).to(dev)
    et, en = vq.vq_prepare(embed, frames=0)
    for N in NS:
        trg = torch.randint(0, K, (N, H), generator=g).to(dev)
        near = torch.cat([embed[h].t()[trg[:, h]] for h in range(H)], dim=-1)
        # a third of the frames each near the target, between codewords and far away (small, mixed and full hinge sets)
        spread = torch.tensor([0.05, 0.5, 3.0])[torch.arange(N) % 3].view(N, 1).to(dev)
        p = (near + spread * torch.randn(N, D, generator=g).to(dev)).requires_grad_(True)
        w = torch.rand(N, generator=g).to(dev)
        fk = lambda q: kernel(q, trg, et, en, 'sum')
        fs = lambda q: stock(q, trg, embed, 'sum')
        lk = fk(p); (lk * w).sum().backward(); gk = p.grad.clone(); p.grad = None
        name = lib.get().msmc_loss_last_kernel().decode()
        ls = fs(p); (ls * w).sum().backward(); gs = p.grad.clone(); p.grad = None
        for _ in range(5):
            one(fk, p, w), one(fs, p, w)
        torch.cuda.synchronize()
        ev = []
        for _ in range(ROUNDS):                               # interleaved: kernel, stock, kernel, stock ...
            ev.append((one(fk, p, w), one(fs, p, w)))
        torch.cuda.synchronize()
        tk = sorted(a.elapsed_time(b) * 1e3 for (a, b), _ in ev)[ROUNDS // 2]
        ts = sorted(a.elapsed_time(b) * 1e3 for _, (a, b) in ev)[ROUNDS // 2]
        # counted bytes of the kernel form, each tensor once: forward p, trg, codebook rows + norms, lossh, gp; backward gp, the
        # incoming gradient, the gradient of p
        byts = 4.0 * N * D + 8.0 * N * H + 4.0 * H * K * (d + 1) + 4.0 * N * H + 4.0 * N * D + 4.0 * N * D + 4.0 * N * H + 4.0 * N * D
        print('%-12s %7d | %-26s %9.1f %9.2f | %-12s %9.1f | %5.2f | %.3e %.3e' %
              ('%dx%dx%d' % (H, d, K), N, name, tk, byts / 1e6, 'stock chain', ts, ts / tk,
               float((lk - ls).abs().max()), float((gk - gs).abs().max())))
        sys.stdout.flush()
        del p, trg, near, w, lk, ls, gk, gs
