#!/usr/bin/env python
"""Runs ON the GPU box: compute_triple_loss forward + backward through the gfx950 kernels (csrc/triple_stream.inc where no head's
codebook fits LDS, the resident triple_loss_kernel for scale) next to the stock operator chain the modules fall back to, on the
same tensors, interleaved call by call in one process.  N = the frames per stage of BASELINE config #4 at B = 64 (6 400 at the
coarse stage, 25 600 at the fine one).  Device events around every call, median of the timed calls after a warm-up, an otherwise
idle process; profiles/triple_stream.md holds the table.
SET=wide: the single wide heads of the k-means unit codebooks (d = 768 / 1024, K = 500 / 2000; csrc/triple_wide.inc) at N = 51 200
frames instead, with the peak of torch.cuda.max_memory_allocated over one forward + backward of either form above what is
allocated before it, and the times of the kernel's two launches from the library's launch log; profiles/triple_wide.md."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
from msmctts_amd.hip import lib, losses, vq

dev = torch.device('cuda:0')
WIDE = os.environ.get('SET', 'stream') == 'wide'
NS = [int(v) for v in os.environ.get('NS', '51200' if WIDE else '6400,25600').split(',')]
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


def peak_mb(fn, p, w):
    """peak of the allocator over one forward + backward, above what is allocated before it"""
    p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    (fn(p) * w).sum().backward()
    torch.cuda.synchronize()
    p.grad = None
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def launches(fn, p):
    """(name, us) of the library's launches during one forward"""
    import ctypes
    L = lib.get()
    torch.cuda.synchronize()
    L.msmc_prof_enable(1)
    with torch.no_grad():
        fn(p)
    torch.cuda.synchronize()
    L.msmc_prof_enable(0)
    out = []
    name, ms = ctypes.create_string_buffer(128), ctypes.c_float()
    for i in range(L.msmc_prof_count()):
        if L.msmc_prof_read(i, name, 128, ctypes.byref(ms)) == 0:
            out.append((name.value.decode(), ms.value * 1e3))
    return out


print('%-12s %7s | %-26s %9s %9s | %-12s %9s | ratio | max |dloss| max |dgrad|' %
      ('H x d x K', 'N', 'kernel', 'us', 'MB', 'reference', 'us'))
for H, d, K in (((1, 768, 500), (1, 768, 2000), (1, 1024, 500), (1, 1024, 2000)) if WIDE else
                ((1, 256, 512), (2, 128, 512), (4, 64, 256))):
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
        if WIDE:
            mk, ms_ = peak_mb(fk, p, w), peak_mb(fs, p, w)
            print('    peak MB above the inputs: kernel %.1f, stock chain %.1f (the mask: %.1f MB)' % (mk, ms_, N * ((K + 63) // 64) * 8 / 1e6))
            for nm, us in launches(fk, p):
                # fp32 MFMA roof 157.3 TFLOP/s; 2 N K d flops per launch.  HBM roof 8 TB/s over the compulsory bytes: pass 1 reads
                # p and the codebook and writes the mask and lossh, pass 2 reads the mask and the codebook and writes gp
                byts1 = 4.0 * N * d + 4.0 * K * (d + 1) + N * ((K + 63) // 64) * 8 + 12.0 * N
                tf = 2.0 * N * K * d / (us * 1e-6) / 1e12
                print('    %-28s %9.1f us  %6.1f TFLOP/s = %4.1f %% of the fp32 MFMA roof, %4.1f %% of the HBM roof' %
                      (nm, us, tf, 100 * tf / 157.3, 100 * byts1 / (us * 1e-6) / 8e12))
        sys.stdout.flush()
        del p, trg, near, w, lk, ls, gk, gs
