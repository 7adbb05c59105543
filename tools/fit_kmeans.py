#!/usr/bin/env python
"""Fits the k-means unit codebook of ``KMeansVQGANEmb`` from feature files, on the gfx950 kernels (``fit_kmeans``,
msmctts_amd/hip/kmeans.py), and writes the ``.npy`` of centres [K, d] that ``quantizer_path`` names.

    python tools/fit_kmeans.py train.list 'feats/hubert/{0}.npy' --clusters 1000 --frames 1000000 -o units.npy

``id_list``: one utterance per line, whitespace-separated attributes; ``pattern``: the feature path with ``{0}``, ``{1}`` ... for
the attributes, as the dataset configurations write it (``.npy``, ``.pt``, headerless float32 ``.dat`` / ``.mgc`` / ``.ap`` through
the readers of datasets/readers.py; ``--dimension`` for the formats that need it).  ``--frames M`` keeps a seeded subsample of
M frames drawn without replacement from all utterances (0: every frame).  ``--init k-means++`` seeds the first centres with
greedy k-means++ on the card (``--local-trials`` candidates per step) in place of K frames drawn uniformly.  Prints the inertia, the number of empty centroids
and the movement of the centres per iteration.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
from msmctts_amd.datasets import readers  # noqa: E402

_RAW = ('.dat', '.mgc', '.ap')


def read_feature(path, dimension=None, shape_only=False):
    """[frames, d] (or its shape) of one feature file, by its extension"""
    ext = os.path.splitext(path)[-1]
    if ext == '.npy':
        return readers.read_npy(path, shape_only=shape_only)
    if ext in _RAW:
        return readers.read_raw_float32(path, dimension, shape_only=shape_only)
    if ext == '.pt':
        return readers.read_torch(path, dimension, shape_only=shape_only)
    raise ValueError('%s: not a frame feature file (.npy, .pt, %s)' % (path, ', '.join(_RAW)))


def load_frames(id_list, pattern, frames=0, seed=0, dimension=None):
    """every frame of the listed utterances, or a seeded subsample of ``frames`` of them, in utterance order -> [M, d] float32"""
    with open(id_list) as f:
        ids = [tuple(line.split()) for line in f if line.strip()]
    paths = [pattern.format(*attrs) for attrs in ids]
    counts = [int(read_feature(p, dimension, shape_only=True)[0]) for p in paths]
    total = sum(counts)
    if total < 1:
        raise ValueError('%s: no frames' % id_list)
    keep = None
    if 0 < frames < total:
        keep = np.sort(np.random.default_rng(seed).choice(total, size=frames, replace=False))
    out, first = [], 0
    for path, n in zip(paths, counts):
        rows = None if keep is None else keep[np.searchsorted(keep, first):np.searchsorted(keep, first + n)] - first
        first += n
        if rows is not None and len(rows) == 0:
            continue
        x = np.asarray(read_feature(path, dimension), dtype=np.float32)
        out.append(x if rows is None else x[rows])
    return np.ascontiguousarray(np.concatenate(out, axis=0))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('id_list')
    ap.add_argument('pattern')
    ap.add_argument('--frames', type=int, default=0, help='seeded subsample of this many frames (0: all)')
    ap.add_argument('--clusters', type=int, required=True)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--tol', type=float, default=1e-4)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--init', choices=('frames', 'k-means++'), default='frames',
                    help='the first centres: K frames drawn uniformly, or k-means++ seeding on the card')
    ap.add_argument('--local-trials', type=int, default=None, help='candidates per k-means++ step (default 2 + floor(ln K), at most 16)')
    ap.add_argument('--dimension', type=int, default=None)
    ap.add_argument('--block-frames', type=int, default=None)
    ap.add_argument('--device', default=None, help='default: the current GPU')
    ap.add_argument('-o', '--output', required=True, help='the centroid file, .npy')
    args = ap.parse_args(argv)
    if not args.output.endswith('.npy'):
        ap.error('the centroid file is recognised by its .npy suffix')
    from msmctts_amd.hip.kmeans import fit_kmeans
    x = load_frames(args.id_list, args.pattern, args.frames, args.seed, args.dimension)
    print('%d frames of %d channels, %d clusters' % (x.shape[0], x.shape[1], args.clusters), flush=True)

    def report(it, rec):
        print('iteration %3d  inertia %.9g  empty centroids %d  movement %.4g' % (it, rec['inertia'], rec['empty'], rec['shift']), flush=True)

    fit = fit_kmeans(x, args.clusters, max_iter=args.iters, tol=args.tol, seed=args.seed, block_frames=args.block_frames,
                     device=args.device, callback=report, init=None if args.init == 'frames' else args.init,
                     n_local_trials=args.local_trials)
    fit.save(args.output)
    print('%s: [%d, %d] after %d iterations, inertia %.9g, %d empty centroids' % (
        args.output, fit.cluster_centers_.shape[0], fit.cluster_centers_.shape[1], fit.n_iter_, fit.inertia_,
        int((fit.counts_ == 0).sum())))
    return fit


if __name__ == '__main__':
    main()
