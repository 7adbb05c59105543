#!/usr/bin/env python
"""Turns stored discrete units back into speech with a trained ``KMeansVQGANEmb``, on the gfx950 kernels: the files
tools/extract_units.py writes go straight into ``synthesis_units`` (no embedding frames, no nearest-centroid search).

    python tools/synthesize_units.py test.list 'out/indices/{0}.npy' -m checkpoints/model_100000 [-c config.yaml] -o wav_dir
    python tools/synthesize_units.py test.list 'out/units/{0}.npy' --durations 'out/durations/{0}.npy' -m ... -o wav_dir

``id_list`` / ``pattern`` as tools/extract_units.py takes them; an utterance is named by the first attribute of its line.
Without ``--durations`` a file holds frame labels (int64 [T]); with it, the units of (unit, duration) runs (int64 [runs]) next
to their durations (int32 [runs]), expanded on the card (``expand_units``).  ``--ref`` is the pattern of the reference mel
files [frames, mel_dim] (``.npy``) a model with a global encoder needs.  ``--jobs B`` utterances share a launch.  Writes
``out_dir/<id>.wav`` through infer.py's writer at ``--sample-rate`` (default: the configuration's ``dataset.samplerate``).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd'), os.path.join(ROOT, 'tools')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402
from infer import save_feature  # noqa: E402


def _padded(rows, value, dtype, device):
    out = torch.full((len(rows), max(max(len(r) for r in rows), 1)), value, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.from_numpy(np.ascontiguousarray(r)).to(dtype)
    return out.to(device)


def main(argv=None, task=None):
    """``task``: a task already built (in-process callers); otherwise ``-m`` / ``-c`` restore one"""
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('id_list')
    ap.add_argument('pattern')
    ap.add_argument('--durations', default=None, help='pattern of the duration files: ``pattern`` then names unit files')
    ap.add_argument('-m', '--model', default=None, help='checkpoint')
    ap.add_argument('-c', '--config', default=None, help='default: the checkpoint\'s own configuration')
    ap.add_argument('--ref', default=None, help='pattern of the reference mel files (a model with a global encoder)')
    ap.add_argument('-o', '--output-dir', required=True)
    ap.add_argument('-j', '--jobs', type=int, default=1, help='utterances per launch')
    ap.add_argument('--sample-rate', type=int, default=None)
    ap.add_argument('--device', default=None, help='default: the current GPU')
    args = ap.parse_args(argv)
    if args.jobs < 1:
        ap.error('--jobs must be positive')
    if task is None:
        if args.model is None:
            ap.error('-m/--model is required')
        from msmctts_amd.tasks import build_task
        task = build_task(args.config, mode='infer', checkpoint=args.model)
    model = task.autoencoder
    if not hasattr(model, 'synthesis_units'):
        raise TypeError('%s has no synthesis_units: units are synthesised by a model with a frozen codebook, such as '
                        'KMeansVQGANEmb' % type(model).__name__)
    if hasattr(model, 'global_encoder') and args.ref is None:
        ap.error('this model has a global encoder: --ref is required')
    device = torch.device(args.device) if args.device is not None else torch.device('cuda', torch.cuda.current_device())
    model = model.to(device).eval()
    rate = args.sample_rate
    if rate is None:
        rate = int(task.config.dataset.samplerate)
    with open(args.id_list) as f:
        ids = [tuple(line.split()) for line in f if line.strip()]
    os.makedirs(args.output_dir, exist_ok=True)
    for first in range(0, len(ids), args.jobs):
        batch = ids[first:first + args.jobs]
        rows = [np.load(args.pattern.format(*attrs), allow_pickle=False).reshape(-1) for attrs in batch]
        ind = _padded(rows, -1, torch.int64, device)
        count = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=device)
        ref = None
        if args.ref is not None and hasattr(model, 'global_encoder'):
            mels = [np.asarray(np.load(args.ref.format(*attrs), allow_pickle=False), dtype=np.float32) for attrs in batch]
            ref = torch.zeros(len(batch), max(len(m) for m in mels), mels[0].shape[1])
            for b, m in enumerate(mels):
                ref[b, :len(m)] = torch.from_numpy(m)
            ref = ref.to(device)
        with torch.no_grad():
            if args.durations is not None:
                durs = [np.load(args.durations.format(*attrs), allow_pickle=False).reshape(-1) for attrs in batch]
                if [len(d) for d in durs] != [len(r) for r in rows]:
                    raise ValueError('units and durations of different lengths in %s' % (batch,))
                dur = _padded(durs, 0, torch.int32, device)
                frames = [int(np.maximum(d, 0).sum()) for d in durs]
                wav = model.synthesis_units(ind, ref=ref, dur=dur, ulen=count)
            else:
                frames = [len(r) for r in rows]
                wav = model.synthesis_units(ind, count, ref=ref)
        wav = wav.float().cpu().numpy().reshape(len(batch), -1)
        hop = wav.shape[1] // max(max(frames), 1)                 # samples per frame: the vocoder's total upsampling
        for b, attrs in enumerate(batch):
            save_feature(os.path.join(args.output_dir, attrs[0] + '.wav'), wav[b, :frames[b] * hop], '.wav', rate)


if __name__ == '__main__':
    main()
