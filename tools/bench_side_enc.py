#!/usr/bin/env python
"""Runs ON the GPU box: the pitch / energy side branch of ``MAMSEncoder`` -- fused (csrc/side_enc.hip + the implicit-GEMM kernels,
``fused_side = True``) against the stock chain it replaces (``fused_side = False``: torch.cat, four nn.Conv1d / three nn.Tanh,
avg_pool1d between transposes, the addition), on the same weights and inputs.

  side      the side branch alone: tracks [B, T, 1] x 2 -> encoding -> per stage pooled and added to a stage output [B, T_i, C] in the
            model's dtype; forward, and forward + backward (gradients of the eight parameters and of the stage outputs).
            B = 16, T = 400, C = 256, downsample_scales [1] and [1, 4], fp32 and bf16 stage outputs.  Device events around
            ``iters`` calls, the two paths alternated within a round, ``rounds`` rounds after a warm-up; printed per round, then
            the median and the spread (max - min over rounds) of each.
  steps     one ``EmbVQGANTrainer`` step per phase at tools/bench_emb.py's sizes with pitch_dim = energy_dim = 1, batch with and
            without tracks (without: zeros, so the same code runs), fused and stock: ms per eager step.

Without an argument both sections run as child processes under their own ``timeout``; the first that fails ends the run."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd'), os.path.join(ROOT, 'tools')]

SECTIONS = (('side', 240), ('steps', 420))
B, T, C = 16, 400, 256


def side_branch(enc, pitch, energy, feats, scales):
    """what ``MAMSEncoder.forward`` does for the side encoding, without the FFT stacks between: -> the stage outputs"""
    import torch
    import torch.nn.functional as F
    from msmctts_amd.hip import side_enc
    side = enc._side_fused(pitch, energy)
    fused = side is not None
    if not fused:
        side = enc.pitch_encoder(torch.cat((pitch, energy), dim=-1).transpose(1, 2).float()).transpose(1, 2)
    outs = []
    for feat, scale in zip(feats, scales):
        if fused:
            side, out = side_enc.pool_add(side, feat, scale)
        else:
            if scale > 1:
                side = F.avg_pool1d(side.transpose(1, 2), kernel_size=scale, stride=scale, ceil_mode=True).transpose(1, 2)
            out = feat + side.to(feat.dtype)
        outs.append(out)
    return outs


def side(iters=100, rounds=5):
    import torch
    import msmctts_amd  # noqa: F401
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import MAMSEncoder
    dev = torch.device('cuda:0')
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    gen = torch.Generator().manual_seed(1)
    pitch, energy = torch.randn(B, T, 1, generator=gen).to(dev), torch.rand(B, T, 1, generator=gen).to(dev)
    for scales in ([1], [1, 4]):
        torch.manual_seed(2)
        enc = MAMSEncoder(C, pitch_dim=1, energy_dim=1, downsample_scales=scales, n_layers=1).to(dev).train()
        params = list(enc.pitch_encoder.parameters())
        for dtype in (torch.float32, torch.bfloat16):
            feats, gouts, Tn = [], [], T
            for s in scales:
                Tn = -(-Tn // s)
                feats.append(torch.randn(B, Tn, C, generator=gen).to(dev).to(dtype).requires_grad_(True))
                gouts.append(torch.randn(B, Tn, C, generator=gen).to(dev).to(dtype))

            def run(fused, backward):
                enc.fused_side = fused
                with torch.set_grad_enabled(backward):
                    outs = side_branch(enc, pitch, energy, feats, scales)
                if backward:
                    for p in params + feats:
                        p.grad = None
                    torch.autograd.backward(outs, gouts)
                return outs
            a, b = run(True, False), run(False, False)
            worst = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b))
            print('side branch  scales %s  %s  max |fused - stock| of the stage outputs %.2e' % (scales, str(dtype)[6:], worst), flush=True)
            for backward in (False, True):
                us = {True: [], False: []}
                for fused in (True, False):
                    for _ in range(20):
                        run(fused, backward)
                for rnd in range(rounds):
                    for fused in ((True, False) if rnd % 2 == 0 else (False, True)):
                        torch.cuda.synchronize()
                        ev[0].record()
                        for _ in range(iters):
                            run(fused, backward)
                        ev[1].record()
                        torch.cuda.synchronize()
                        us[fused].append(ev[0].elapsed_time(ev[1]) * 1e3 / iters)
                for fused in (True, False):
                    v = us[fused]
                    print('  %-9s %-5s scales %-7s %-6s us per call by round %s  median %8.1f  spread %6.1f' % (
                        'fwd+bwd' if backward else 'fwd', str(dtype)[6:], scales, 'fused' if fused else 'stock',
                        ' '.join('%8.1f' % x for x in v), statistics.median(v), max(v) - min(v)), flush=True)


def steps(nsteps=8, rounds=3, warm=4):
    import random
    import torch
    import bench_emb
    from msmctts_amd.synthetic import make_emb_batch
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    dev = torch.device('cuda:0')
    raw = bench_emb.config()
    raw['task']['autoencoder'].update(pitch_dim=1, energy_dim=1)
    cfg = Config(raw)
    torch.manual_seed(cfg.seed)
    task = build_task(cfg, mode='train')
    tr = build_trainer(cfg, task, num_gpus=1, rank=0)
    tr.optimizer = build_optimizer(tr.model, cfg.optimizer)
    tr.amp_dtype = torch.bfloat16
    tr.rng = random.Random(1234)
    tr.model.train()
    enc = tr.model.autoencoder.encoder
    with_tracks = make_emb_batch(bench_emb.B, bench_emb.T, bench_emb.EMB, 80, bench_emb.HOP, seed=1234, device=dev, tracks=True)
    zeros = dict(with_tracks, pitch=torch.zeros_like(with_tracks['pitch']), energy=torch.zeros_like(with_tracks['energy']))
    for which, iteration in ((0, 5), (1, 15), (2, 25)):
        assert tr._phase(iteration) == which
        for name, batch in (('tracks', with_tracks), ('zero tracks', zeros)):
            for fused in (True, False):
                enc.fused_side = fused
                for _ in range(warm):
                    log = tr.train_step(batch, iteration)
                torch.cuda.synchronize()
                assert all(float(v) == float(v) for v in log['loss'].values()), 'a loss is NaN'
                ms = []
                for _ in range(rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(nsteps):
                        tr.train_step(batch, iteration)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3 / nsteps)
                print('  phase %d  bf16  %-11s %-6s ms per eager step by round %s' % (which, name, 'fused' if fused else 'stock',
                                                                                    ' '.join('%8.2f' % x for x in ms)), flush=True)


def main(argv):
    names = [a for a in argv if a in dict(SECTIONS)]
    if names:
        import torch
        assert torch.cuda.is_available(), 'tools/bench_side_enc.py measures on the GPU'
        torch.cuda.set_device(0)
        for name in names:
            side() if name == 'side' else steps()
        return 0
    for name, limit in SECTIONS:
        rc = subprocess.call(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), name])
        if rc != 0:
            print('section %s ended with status %d: stopping' % (name, rc), flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
