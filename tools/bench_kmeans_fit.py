#!/usr/bin/env python
"""Runs ON the GPU box: one Lloyd iteration of ``fit_kmeans`` (msmctts_amd/hip/kmeans.py) piece by piece, at N = 2^20 synthetic
frames, d in {768, 1024}, K in {100, 500, 2000}.

  E step      ``vq_prepare`` + per block ``vq_search`` + the float64 sum of its squared error (as the fit runs it)
  statistics  ``centroid_stats`` per block, accumulating (msmc_kmeans_stats: six launches), labels of the E step
  update      ``centroid_update`` (msmc_kmeans_update)
  stock       the same M step on stock operators: ``zeros.index_add_(0, labels, x)`` + ``bincount`` + the division
  kernels     the launches of msmc_kmeans_stats one by one, from the library's own event pairs (msmc_prof_*)
  HBM bound   bytes the statistics must move -- one read of x plus 8 bytes of label per frame -- over the statistics time,
              against 8 TB/s (peak) and 6.3 TB/s (what a streaming read achieves on this chip)

  seeding     (K >= 500) ``kmeans_plusplus`` (msmc_kmeanspp_seed) of the same frames: its two launches per step from the library's
              event pairs, the pass over x against the bytes of x over a streaming read of x measured in the same run, the whole
              seeding against one Lloyd iteration, and ``fit_kmeans(init='k-means++')`` against ``init=None`` after ``--fit-iters``

Frames: K centres N(0, 1), a frame = a random centre + 0.5 N(0, 1); the centres searched are K frames.  Device events around
each piece, two warm-up rounds, then ``--rounds`` timed rounds in which the pieces alternate; median / min.

    python tools/bench_kmeans_fit.py [--rounds 5] [--frames 1048576] [--quick]
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
from msmctts_amd.hip import kmeans, lib, vq

dev = torch.device('cuda:0')
PEAK_BYTES, STREAM_BYTES = 8.0e12, 6.3e12
WIDTHS, CLUSTERS = (768, 1024), (100, 500, 2000)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


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


def blob_frames(N, d, K):
    gen = torch.Generator(device=dev).manual_seed(d + K)
    true = torch.randn(K, d, device=dev, generator=gen)
    x = torch.empty(N, d, device=dev)
    for s in range(0, N, 1 << 16):                       # (in slabs: no second N x d temporary)
        n = min(N, s + (1 << 16)) - s
        which = torch.randint(0, K, (n,), device=dev, generator=gen)
        x[s:s + n] = true[which] + 0.5 * torch.randn(n, d, device=dev, generator=gen)
    return x, gen


def seeding(N, d, K, rounds, fit_iters):
    """k-means++ seeding (msmc_kmeanspp_seed) of the same blob frames: a step against the bytes of x over the rate of a plain
    streaming read of x measured here, the whole seeding against one Lloyd iteration, and the fit it starts against the fit from
    K frames drawn uniformly"""
    x, _ = blob_frames(N, d, K)
    L = kmeans.default_local_trials(K)
    with torch.no_grad():
        read = [event_us(lambda: x.view(-1).sum(dtype=torch.float32)) for _ in range(2 + rounds)][2:]
        stream = 4.0 * N * d / statistics.median(read) / 1e6                  # TB/s
        few = 1 + 16                                        # centre 0 and sixteen steps: the launches one by one
        kmeans.kmeans_plusplus(x, few, seed=1, n_local_trials=L)
        torch.cuda.synchronize()
        state = {}

        def short():
            state['out'] = kmeans.kmeans_plusplus(x, few, seed=1, n_local_trials=L)

        parts = kernel_breakdown(short)
        dist = (parts['kpp_dist_kernel'] - 0.0) / few       # (centre 0 is a pass with one candidate: counted as a step)
        select = parts['kpp_select_kernel'] / few
        whole = [event_us(lambda: state.update(out=kmeans.kmeans_plusplus(x, K, seed=1, n_local_trials=L))) for _ in range(1 + min(rounds, 3))][1:]
        med = statistics.median(whole)
        byts = 4.0 * N * d
        print('d = %d, K = %d, N = %d, %d candidates per step: streaming read of x (torch sum) %.2f TB/s' % (d, K, N, L, stream))
        print('  per step: kpp_dist_kernel %.1f us, kpp_select_kernel %.1f us (means over %d launches); %.1f MB of x -> the pass reads at '
              '%.2f TB/s; bytes / measured streaming rate = %.1f us, bytes / 6.3 TB/s = %.1f us' % (
                  dist, select, few, byts / 1e6, byts / dist / 1e6, byts / stream / 1e6, byts / STREAM_BYTES * 1e6))
        print('  whole seeding: %.1f / %.1f ms (median / min of %d) = %.1f us per centre' % (med / 1e3, min(whole) / 1e3, len(whole), med / K))
        potential = state['out'][2].cpu()
        print('  seeding potential: %.6g after centre 0, %.6g after centre %d' % (float(potential[0]), float(potential[-1]), K - 1))
        fits = {}
        for name, init in (('uniform draw', None), ('k-means++', 'k-means++')):
            rec = []
            t = event_us(lambda: fits.update({name: kmeans.fit_kmeans(x, K, max_iter=fit_iters, tol=0.0, seed=1, init=init,
                                                                     callback=lambda it, r: rec.append(r))}))
            f = fits[name]
            print('  fit from %-13s %d iterations in %.1f ms (seeding included): inertia %.9g, %d empty centroids; inertia of the first E '
                  'step %.9g' % (name + ':', f.n_iter_, t / 1e3, f.inertia_, int((f.counts_ == 0).sum()), rec[0]['inertia']), flush=True)
            if init is None:                                # (the variance pass and the final search are in: an upper figure)
                per_iter = t / f.n_iter_
                print('  one Lloyd iteration: at most %.1f ms (that fit / its iterations) -> the whole seeding is %.1f of them' % (
                    per_iter / 1e3, med / per_iter))
    vq._F32_OF['last'] = None


def one_shape(N, d, K, rounds):
    x, gen = blob_frames(N, d, K)
    centers = x[torch.randperm(N, device=dev, generator=gen)[:K]].clone()
    block = kmeans.default_block_frames(d)
    spans = [(s, min(N, s + block)) for s in range(0, N, block)]
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    sums, counts = torch.empty(K, d, device=dev), torch.empty(K, device=dev)
    workspace = kmeans._workspace(min(N, block), d, K, dev)
    state = {}

    def e_step():
        et, en = vq.vq_prepare(centers.t().unsqueeze(0).contiguous(), frames=min(N, block))
        inertia = torch.zeros((), dtype=torch.float64, device=dev)
        for s, e in spans:
            _, diff, ind = vq.vq_search(x[s:e], et, en)
            inertia += diff.sum(dtype=torch.float64)
            labels[s:e] = ind.reshape(-1)
        state['inertia'] = inertia

    def stats():
        for b, (s, e) in enumerate(spans):
            kmeans.centroid_stats(x[s:e], labels[s:e], K, out=(sums, counts), accumulate=b > 0, workspace=workspace)

    def update():
        state['shift2'] = kmeans.centroid_update(sums, counts, state['moved'])

    def stock():
        s = torch.zeros(K, d, device=dev).index_add_(0, labels, x)
        c = torch.bincount(labels, minlength=K).float()
        state['stock'] = torch.where(c.unsqueeze(1) > 0, s / c.unsqueeze(1), centers)

    pieces = {'E step': e_step, 'statistics': stats, 'update': update, 'stock M step': stock}
    with torch.no_grad():
        times = {k: [] for k in pieces}
        for r in range(2 + rounds):
            for name, fn in pieces.items():
                if name == 'update':
                    state['moved'] = centers.clone()            # (updated in place: a fresh copy, outside the timed span)
                t = event_us(fn)
                if r >= 2:
                    times[name].append(t)
        got, want = state['moved'], state['stock']
        scale = float(want.abs().max())
        print('d = %d, K = %d, N = %d (%d block%s of at most %d frames), %d empty centroids; centres of the kernels against the stock '
              'M step: max |difference| %.3g (largest centre value %.3g)' % (d, K, N, len(spans), '' if len(spans) == 1 else 's', block,
                                                                       int((counts == 0).sum()), float((got - want).abs().max()), scale))
        for name in pieces:
            print('  %-14s %10.1f / %10.1f us (median / min of %d)' % (name, statistics.median(times[name]), min(times[name]), rounds))
        byts = 4.0 * N * d + 8.0 * N
        med = statistics.median(times['statistics'])
        print('  statistics: %.1f MB of x and labels -> %.2f TB/s, %.1f %% of 8 TB/s, %.1f %% of 6.3 TB/s; kernel M step (statistics + '
              'update) / stock M step = %.2f' % (byts / 1e6, byts / med / 1e6, 100.0 * byts / PEAK_BYTES / (med * 1e-6),
                                               100.0 * byts / STREAM_BYTES / (med * 1e-6),
                                               (med + statistics.median(times['update'])) / statistics.median(times['stock M step'])))
        parts = kernel_breakdown(stats)
        print('  launches of the statistics (us, one call): ' + '  '.join('%s %.1f' % kv for kv in parts.items()), flush=True)
    vq._F32_OF['last'] = None


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--quick', action='store_true', help='d = 1024, K = 500 only')
    ap.add_argument('--seeding', action='store_true', help='the k-means++ seeding section (d in {768, 1024}, K in {500, 2000}) only')
    ap.add_argument('--fit-iters', type=int, default=10, help='Lloyd iterations of the two fits the seeding section compares')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to measure without one'
    print(torch.cuda.get_device_name(0))
    try:
        print('shader clock as the driver reports it before the runs: %d MHz' % torch.cuda.clock_rate())
    except Exception as err:                                 # (no management library in this installation)
        print('shader clock: not read (%s)' % type(err).__name__)
    for d in ((1024,) if args.quick else WIDTHS):
        for K in ((500,) if args.quick else CLUSTERS):
            if not args.seeding:
                one_shape(args.frames, d, K, args.rounds)
                torch.cuda.empty_cache()
            if K >= 500:
                seeding(args.frames, d, K, args.rounds, args.fit_iters)
                torch.cuda.empty_cache()
