#!/usr/bin/env python
"""Golden fixture for the quantiser-free voice-conversion model, generated from the reference itself.

    python tests/golden/make_golden_vc.py        # writes tests/golden/small_vc.npz

A small EmbVC (reference networks/vqgantts/msmc_vqgan_emb.py:472-628) after the recipe of make_golden_emb.py / make_golden_ecapa.py:
emb_dim 24, pitch / energy tracks on, ECAPA_TDNN global encoder, frame decoder and ``pred_mel``.  Two things differ from
small_emb's sizes, both forced: ``n_model_size`` is 64 and ``mel_dim`` 24 (the global encoder is built with
``channels = n_model_size``; the product refuses channels % 64 != 0 and in_channels % 8 != 0, as small_ecapa_emb has it), and
``downsample_scales`` is [1, 1] (the reference feeds the LAST stage's output to a frame decoder whose positions run over the
input's frames: a down-sampled last stage does not run there).  Two stages, so the side encoding is added twice.

Size: the weights are rounded to fp16-representable values BEFORE the reference runs and stored as float16 (lossless); the global
encoder reuses small_ecapa.npz's weights and is not stored again.
Stored: state_dict keys and shapes, weights, batch, training-mode outputs for explicit windows with dropout forced to 0 (every
dictionary entry, a scalar of them and its gradients with respect to the embeddings, ``mel`` and the side encoder's parameters),
the global encoder's buffers afterwards, evaluation-mode window='full' ``decoder_outputs``.  Data only; no reference source.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shims)

import torch  # noqa: E402

from make_golden_ecapa import fp16_representable, store16  # noqa: E402
from make_golden_emb import EMB_CFG, WINDOWS  # noqa: E402
from msmctts.networks.vqgantts.msmc_vqgan_emb import EmbVC  # noqa: E402
from msmctts.utils.config import Config  # noqa: E402

VC_CFG = {k: v for k, v in copy.deepcopy(EMB_CFG).items() if k != 'quantizer_config'}
VC_CFG.update(n_model_size=64, mel_dim=24, global_encoder_config={'_name': 'ECAPA_TDNN'})
VC_CFG['encoder_config']['downsample_scales'] = [1, 1]


def main():
    ze = np.load(os.path.join(HERE, 'small_ecapa.npz'))
    torch.manual_seed(97531)
    cfg = copy.deepcopy(VC_CFG)
    cfg['global_encoder_config'] = Config(cfg['global_encoder_config'])
    m = EmbVC(**cfg)
    G.zero_dropout(m)
    m.global_encoder.load_state_dict({k[len('enc.state.'):]: torch.from_numpy(ze[k].astype(np.float32) if ze[k].dtype == np.float16
                                                                               else ze[k]) for k in ze.files if k.startswith('enc.state.')})
    fp16_representable(m)
    out = {'cfg': np.frombuffer(json.dumps(VC_CFG).encode(), dtype=np.uint8), 'windows': np.asarray(WINDOWS, dtype=np.int64)}
    for k, v in m.state_dict().items():
        out['state.' + k] = store16(v) if not k.startswith('global_encoder.') else np.zeros(0, dtype=np.float16)
        out['shape.' + k] = np.asarray(tuple(v.shape), dtype=np.int64)
    g = torch.Generator().manual_seed(11)
    lengths = torch.tensor([24, 17, 9], dtype=torch.int64)
    emb = torch.randn(3, 24, 24, generator=g)
    pitch, energy = torch.randn(3, 24, 1, generator=g), torch.rand(3, 24, 1, generator=g)
    mel = torch.randn(3, 24, 24, generator=g)             # (left dense: see make_golden_ecapa.py)
    for i, n in enumerate(lengths.tolist()):
        emb[i, n:], pitch[i, n:], energy[i, n:] = 0.0, 0.0, 0.0
    for k, v in (('emb', emb), ('emb_length', lengths), ('pitch', pitch), ('energy', energy), ('mel', mel)):
        out['batch.' + k] = G.npy(v)

    def put(prefix, d):
        for k, v in d.items():
            if torch.is_tensor(v):
                out['%s.%s' % (prefix, k)] = G.npy(v)
            elif isinstance(v, (tuple, list)):
                for i, t in enumerate(v):
                    if torch.is_tensor(t):
                        out['%s.%s.%d' % (prefix, k, i)] = G.npy(t)

    m.train()
    e, r = emb.clone().requires_grad_(True), mel.clone().requires_grad_(True)
    o = m(e, lengths, pitch, energy, mel=r, window=WINDOWS)
    put('train', o)
    scalar = (o['decoder_outputs'].pow(2).mean() + o['mel_outputs'].mean() + o['content_representations'].mean()
              + sum(f.pow(2).mean() for f in o['encoder_outputs']))
    scalar.backward()
    out['train.scalar'] = G.npy(scalar)
    out['train.grad_emb'] = G.npy(e.grad)
    out['train.grad_mel'] = G.npy(r.grad)
    for k, p in m.encoder.pitch_encoder.named_parameters():
        out['train.grad.encoder.pitch_encoder.' + k] = G.npy(p.grad)
    for k, v in m.state_dict().items():
        if 'global_encoder' in k and ('running' in k or 'num_batches' in k):
            out['after.' + k] = G.npy(v).copy()
    m.eval()
    with torch.no_grad():
        out['eval.full.decoder_outputs'] = G.npy(m(emb, lengths, pitch, energy, ref=mel)['decoder_outputs'])
    path = os.path.join(HERE, 'small_vc.npz')
    np.savez_compressed(path, **out)
    print('wrote small_vc.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
