#!/usr/bin/env python
"""Runs ON the GPU box: the wide nearest-centroid search (csrc/vq_wide.inc, msmc_vq_search_wide) and the EmbVQGANTrainer step
of a KMeansVQGANEmb task.

  search    d = 1024 with K = 1000 and K = 2000, d = 768 with K = 500, at N = 6400 (B = 16, T = 400) and N = 2^17:
            * the kernel from the library's own event pairs (msmc_prof_*): the launcher's choice of waves per frame tile and
              each forced choice (msmc_vq_wide_set_split 1 / 2 / 4);
            * vq_search (prepare excluded: the centroids are frozen) next to the reference's expression on stock operators
              -- ``x.pow(2).sum(1, keepdim=True) - 2 x @ e + e.pow(2).sum(0)``, ``max``, ``embedding`` and the two element-wise
              outputs -- device events around blocks of calls, the two alternated, three rounds;
            * the indices of the two, compared at the timed size (near-ties may differ: counted);
            * work 2 N d K flop against the fp32-MFMA peak (157.3 TFLOP/s), bytes N d 4 (x) + K d 4 (centroids) + N d 8 (quant,
              diff) against 8 TB/s: the roofline time is the larger of the two, the fraction is roofline / kernel time.
  trainer   (``--trainer``) one EmbVQGANTrainer step per phase on a KMeansVQGANEmb task: emb_dim 1024, K = 1000, n_model_size
            256, B = 8, T = 200, device events, median of five steps after two warm-up steps.

    python tools/bench_kmeans.py [--trainer] [--quick]
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import numpy as np
import torch
import torch.nn.functional as F
from msmctts_amd.hip import lib, vq

dev = torch.device('cuda:0')
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
SHAPES = ((1024, 1000), (1024, 2000), (768, 500))
FRAMES = (6400, 1 << 17)


def kernel_us(fn, iters):
    L = lib.get()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    L.msmc_prof_enable(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    buf, ms, times = ctypes.create_string_buffer(128), ctypes.c_float(), []
    for i in range(L.msmc_prof_count()):
        assert L.msmc_prof_read(i, buf, 128, ctypes.byref(ms)) == 0
        if buf.value.decode().startswith('vq_search_wide_kernel'):
            times.append(ms.value * 1e3)
    L.msmc_prof_enable(0)
    assert len(times) == iters, (len(times), iters)
    return statistics.median(times), min(times)


def stock(x, e):
    """reference modules.py:26-33, :59-60 on stock operators"""
    dist = x.pow(2).sum(1, keepdim=True) - 2 * x @ e + e.pow(2).sum(0, keepdim=True)
    ind = (-dist).max(1)[1]
    q = F.embedding(ind, e.t())
    return x + (q - x), (q - x).pow(2), ind


def search(quick):
    L = lib.get()
    gen = torch.Generator().manual_seed(0)
    for d, K in SHAPES:
        e = torch.randn(1, d, K, generator=gen).to(dev)
        et, en = vq.vq_prepare(e, frames=0)
        for N in FRAMES:
            x = torch.randn(N, d, generator=gen).to(dev)
            iters = 5 if quick else (40 if N <= 6400 else 12)
            flop, byts = 2.0 * N * d * K, 4.0 * N * d + 4.0 * K * d + 8.0 * N * d
            roof_us = max(flop / PEAK_FLOPS, byts / PEAK_BYTES) * 1e6
            bound = 'fp32 MFMA' if flop / PEAK_FLOPS >= byts / PEAK_BYTES else 'HBM'
            print('d = %d, K = %d, N = %d: %.2f GFLOP, %.1f MB, roofline %.1f us (%s)' % (d, K, N, flop / 1e9, byts / 1e6, roof_us, bound))
            for wc in (0, 1, 2, 4):
                L.msmc_vq_wide_set_split(wc)
                med, lo = kernel_us(lambda: vq.vq_search(x, et, en, wide=True), iters)
                print('  vq_search_wide_kernel  split %s  %8.1f / %8.1f us (median / min of %d)  %5.1f TFLOP/s  %4.1f %% of the roofline'
                      % (wc or 'auto', med, lo, iters, flop / med / 1e6, 100.0 * roof_us / med), flush=True)
            L.msmc_vq_wide_set_split(0)
            got = vq.vq_search(x, et, en, wide=True)[2].view(-1)
            want = stock(x, e[0])[2]
            print('  indices that differ from the stock chain: %d of %d' % (int((got != want).sum()), N))
            ms = {}
            calls = iters
            fns = {'kernel': lambda: vq.vq_search(x, et, en, wide=True), 'stock': lambda: stock(x, e[0])}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(3):
                for name, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.setdefault(name, []).append(e0.elapsed_time(e1) / calls * 1e3)
            print('  vq_search (wide), us per call, 3 rounds of %d:  %s' % (calls, ' '.join('%.1f' % v for v in ms['kernel'])))
            print('  stock operator chain, us per call:              %s' % ' '.join('%.1f' % v for v in ms['stock']), flush=True)
            del x


def trainer():
    import random
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    B, T, HOP, EMB, K, MEL, MODEL = 8, 200, 300, 1024, 1000, 80, 256
    fft = dict(max_seq_len=512, n_layers=2, n_head=2, d_k=64, d_v=64, d_inner=1024, fft_conv1d_kernel=3, fft_conv1d_padding=1,
               dropout=0.0, attn_dropout=0.0, fused_layernorm=False)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'centroids.npy')
        np.save(path, np.random.default_rng(0).standard_normal((K, EMB)).astype(np.float32))
        ae = {'_name': 'KMeansVQGANEmb', 'emb_dim': EMB, 'n_model_size': MODEL, 'quantizer_path': path,
              'global_encoder_config': {'_name': 'ECAPA_TDNN'}, 'frame_decoder_config': fft, 'pred_mel': True, 'mel_dim': MEL,
              'decoder_config': dict(upsample_rates=[6, 5, 5, 2], upsample_kernel_sizes=[12, 11, 11, 4], upsample_initial_channel=256,
                                     resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])}
        disc = {'_name': 'UnivNetDiscriminator',
                'mrd_config': dict(hop_lengths=[15, 60], hidden_channels=[32, 32], domain='double', mel_scale=True, sample_rate=24000),
                'mpd_config': dict(periods=[2, 3], channels=4, max_channels=16)}
        cfg = Config({'id': 'bench_kmeans', 'task': {'_name': 'NASynTTSEmb', 'autoencoder': ae, 'discriminator': disc},
                      'trainer': dict(_name='EmbVQGANTrainer', grad_clip_thresh=1.0, sample_batch_size=-1, sample_lengths=6000,
                                      frame_loss_supervised_step=2, stft_loss_supervised_step=4, lambda_frame=450, lambda_fm=2,
                                      lambda_stft=45),
                      'optimizer': {'_default': dict(_name='AdamW', learning_rate=2e-4, betas=[0.8, 0.99], eps=1e-8, weight_decay=0.0)},
                      'dataset': dict(samplerate=24000, feature=['emb', 'mel', 'wav'], frameshift=[HOP, HOP, 1])})
        torch.manual_seed(0)
        task = build_task(cfg, mode='train').to(dev).train()
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.model = task
    tr.optimizer = build_optimizer(task, cfg.optimizer)
    tr.rng = random.Random(0)
    gen = torch.Generator().manual_seed(1)
    lengths = torch.full((B,), T, dtype=torch.int64)
    batch = {'emb': torch.randn(B, T, EMB, generator=gen), 'emb_length': lengths, 'mel': torch.randn(B, T, MEL, generator=gen),
             'wav': torch.rand(B, T * HOP, 1, generator=gen) * 2 - 1, 'wav_length': lengths * HOP}
    batch = {k: v.to(dev) for k, v in batch.items()}
    batch['emb_length_host'] = lengths.tolist()
    print('EmbVQGANTrainer step, KMeansVQGANEmb(emb_dim %d, K %d, n_model_size %d), B = %d, T = %d (ms, median / min of 5):' % (EMB, K, MODEL, B, T))
    for phase, iteration in ((0, 1), (1, 3), (2, 6)):
        times = []
        for i in range(7):
            task.zero_grad()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.train_step(batch, iteration)
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        print('  phase %d: %.2f / %.2f   (search: %s)' % (phase, statistics.median(times), min(times), lib.get().msmc_vq_last_kernel().decode()),
              flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--trainer', action='store_true')
    ap.add_argument('--quick', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to measure without one'
    search(args.quick)
    if args.trainer:
        trainer()
