#!/usr/bin/env python
"""Turns feature files into discrete units with a fitted k-means codebook, on the gfx950 kernels (msmctts_amd/hip/units.py):
nearest-centre labels per frame (``msmc_vq_assign_wide``), optionally collapsed into (unit, duration) runs, and the usage of
the codebook over the whole list.

    python tools/extract_units.py train.list 'feats/hubert/{0}.npy' -c units.npy -o out_dir [--collapse] [--jobs 16]

``id_list`` / ``pattern`` as tools/fit_kmeans.py takes them; an utterance is named by the first attribute of its line.
Writes ``out_dir/indices/<id>.npy`` (int64 [T], as the reference's vq_analysis.py saves them), with ``--collapse`` also
``out_dir/units/<id>.npy`` (int64 [runs]) and ``out_dir/durations/<id>.npy`` (int32 [runs]), and ``out_dir/usage.npy`` (int64 [K]
frames per code, accumulated on the card over the list).  ``--jobs B`` utterances share a launch.  Prints ``used entropy_bits``
-- the codes used and their entropy in bits -- as the reference script's ``compute_codebook_complexity`` does.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd'), os.path.join(ROOT, 'tools')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402
from fit_kmeans import read_feature  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('id_list')
    ap.add_argument('pattern')
    ap.add_argument('-c', '--centers', required=True, help='the centroid file [K, d], .npy (tools/fit_kmeans.py writes it)')
    ap.add_argument('-o', '--output-dir', required=True)
    ap.add_argument('--collapse', action='store_true', help='also write the (unit, duration) runs')
    ap.add_argument('-j', '--jobs', type=int, default=1, help='utterances per launch')
    ap.add_argument('--dimension', type=int, default=None)
    ap.add_argument('--device', default=None, help='default: the current GPU')
    args = ap.parse_args(argv)
    if args.jobs < 1:
        ap.error('--jobs must be positive')
    from msmctts_amd.hip import units
    centers = np.load(args.centers, allow_pickle=False)
    K = int(centers.shape[0])
    with open(args.id_list) as f:
        ids = [tuple(line.split()) for line in f if line.strip()]
    kinds = ('indices',) + (('units', 'durations') if args.collapse else ())
    for kind in kinds:
        os.makedirs(os.path.join(args.output_dir, kind), exist_ok=True)
    counts = None
    for first in range(0, len(ids), args.jobs):
        batch = ids[first:first + args.jobs]
        feats = [np.asarray(read_feature(args.pattern.format(*attrs), args.dimension), dtype=np.float32) for attrs in batch]
        lengths = [int(x.shape[0]) for x in feats]
        labels, _ = units.assign_units(np.concatenate(feats, axis=0), centers, want_dist=False, device=args.device)
        T = max(max(lengths), 1)
        ind = torch.full((len(batch), T), -1, dtype=torch.int64, device=labels.device)
        for b, part in enumerate(labels.split(lengths)):
            ind[b, :lengths[b]] = part
        length = torch.tensor(lengths, dtype=torch.int64, device=labels.device)
        counts = units.unit_usage(ind, length, K, counts)
        runs = [t.cpu().numpy() for t in units.collapse_units(ind, length)] if args.collapse else None
        ind = ind.cpu().numpy()
        for b, attrs in enumerate(batch):
            np.save(os.path.join(args.output_dir, 'indices', attrs[0] + '.npy'), ind[b, :lengths[b]])
            if runs is not None:
                n = int(runs[2][b])
                np.save(os.path.join(args.output_dir, 'units', attrs[0] + '.npy'), runs[0][b, :n])
                np.save(os.path.join(args.output_dir, 'durations', attrs[0] + '.npy'), runs[1][b, :n])
    counts = np.zeros(K, dtype=np.int64) if counts is None else counts.cpu().numpy()
    np.save(os.path.join(args.output_dir, 'usage.npy'), counts)
    used, entropy = units.usage_summary(counts)
    print(used, entropy)
    return counts


if __name__ == '__main__':
    main()
