#!/usr/bin/env python
"""Extracts the multi-stage code indices of a corpus with a trained ``MSMCVQGANEmb``: the frozen ``analysis`` (encoder + code
search on the gfx950 kernels) run once, so that ``EmbPredictorTrainer`` can train on stored codes (``codes_<i>`` features)
without running it at every step.

    python tools/extract_codes.py train.list 'feats/hubert/{0}.npy' -m checkpoint -o out_dir [-c config.yaml]
                                  [--pitch 'pitch/{0}.npy' --energy 'energy/{0}.npy'] [--jobs 16]

``id_list`` / ``pattern`` as tools/fit_kmeans.py takes them; an utterance is named by the first attribute of its line.
Writes ``out_dir/codes_<i>/<id>.npy`` for every stage i (0 the coarsest): [T_i, H] labels trimmed to the stage's valid length,
int16 when the codebook has at most 32767 entries, else int32.  ``--jobs B`` utterances share a pass, zero-padded to the longest
as a training batch is: with a down-sampling stage the last pooled frame of a shorter utterance then sees that padding, as it
does in training from frames (``--jobs 1`` pads nothing).  Prints, per stage and head, ``stage head used entropy_bits`` -- the
codes used and their entropy in bits over the list, the two numbers of the reference's examples/qs-tts/scripts/vq_analysis.py
(``compute_codebook_complexity``) -- from ``unit_usage`` / ``usage_summary`` (msmctts_amd/hip/units.py).
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


def _track(pattern, attrs, frames):
    """a pitch / energy file as [frames, width] float32"""
    x = np.asarray(read_feature(pattern.format(*attrs)), dtype=np.float32)
    x = x.reshape(x.shape[0], -1)
    if x.shape[0] != frames:
        raise ValueError('%s has %d frames, the embedding %d' % (pattern.format(*attrs), x.shape[0], frames))
    return x


def _pad(arrays, device):
    T = max(a.shape[0] for a in arrays)
    out = np.zeros((len(arrays), T, arrays[0].shape[1]), dtype=np.float32)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return torch.from_numpy(out).to(device)


def extract(model, ids, pattern, output_dir, pitch=None, energy=None, jobs=1, dimension=None, out=sys.stdout):
    """``ids``: a list of attribute tuples.  Returns {(stage, head): counts [K] int64 numpy} and prints the usage lines."""
    from msmctts_amd.hip import units
    model.eval()
    device = next(model.parameters()).device
    quantizers = model.quantizer.quantizer
    sizes = [q.n_embed for q in quantizers]
    for i in range(len(quantizers)):
        os.makedirs(os.path.join(output_dir, 'codes_%d' % i), exist_ok=True)
    counts = {}
    for first in range(0, len(ids), jobs):
        batch = ids[first:first + jobs]
        feats = [np.asarray(read_feature(pattern.format(*attrs), dimension), dtype=np.float32) for attrs in batch]
        length = torch.tensor([x.shape[0] for x in feats], dtype=torch.int32, device=device)
        tracks = {}
        for name, pat in (('pitch', pitch), ('energy', energy)):
            if pat is not None:
                tracks[name] = _pad([_track(pat, attrs, x.shape[0]) for attrs, x in zip(batch, feats)], device)
        with torch.no_grad():
            qs = model.analysis(_pad(feats, device), length, **tracks)
        for i, (ind, slen) in enumerate(zip(qs['quantizer_indices'], qs['quantizer_lengths'])):
            ind = ind.unsqueeze(-1) if ind.dim() == 2 else ind                 # (a single-head stage: [B, T_i])
            for h in range(ind.shape[-1]):
                counts[(i, h)] = units.unit_usage(ind[..., h].contiguous(), slen, sizes[i], counts.get((i, h)))
            host, slen = ind.cpu().numpy(), slen.cpu().tolist()
            dtype = np.int16 if sizes[i] <= 32767 else np.int32
            for b, attrs in enumerate(batch):
                np.save(os.path.join(output_dir, 'codes_%d' % i, attrs[0] + '.npy'), host[b, :int(slen[b])].astype(dtype))
    counts = {k: v.cpu().numpy() for k, v in counts.items()}
    for (i, h), c in sorted(counts.items()):
        used, entropy = units.usage_summary(c)
        print(i, h, used, entropy, file=out)
    return counts


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('id_list')
    ap.add_argument('pattern')
    ap.add_argument('-m', '--model', required=True, help='checkpoint of the task whose autoencoder is the MSMCVQGANEmb')
    ap.add_argument('-c', '--config', default=None, help='default: the configuration stored in the checkpoint')
    ap.add_argument('-o', '--output-dir', required=True)
    ap.add_argument('--pitch', default=None, help='pattern of the pitch track files')
    ap.add_argument('--energy', default=None, help='pattern of the energy track files')
    ap.add_argument('-j', '--jobs', type=int, default=1, help='utterances per pass')
    ap.add_argument('--dimension', type=int, default=None)
    ap.add_argument('--device', default='cuda', help='default: the current GPU')
    args = ap.parse_args(argv)
    if args.jobs < 1:
        ap.error('--jobs must be positive')
    from msmctts_amd.tasks import load_model
    model = load_model('autoencoder', args.model, args.config).to(args.device)
    with open(args.id_list) as f:
        ids = [tuple(line.split()) for line in f if line.strip()]
    return extract(model, ids, args.pattern, args.output_dir, args.pitch, args.energy, args.jobs, args.dimension)


if __name__ == '__main__':
    main()
