#!/usr/bin/env python
"""Golden fixture for the speaker reference encoder, generated from the reference itself.

    python tests/golden/make_golden_ecapa.py        # writes tests/golden/small_ecapa.npz and small_ecapa_emb.npz

Size: both modules' weights are rounded to fp16-representable values BEFORE the reference runs and stored as float16 (lossless);
the four parameter gradients of more than 8192 elements are stored as every 4th element of the flattened tensor
(``enc.train.grad4.*``), all others in full; (b) reuses (a)'s weights for its global encoder and lives in its own file.

(a) ``enc.*``: a small ECAPA_TDNN (reference networks/vqgantts/tdnn.py:180-244; in_channels 24, embd_dim 64, channels 64):
    state_dict, input [3][37][24], training-mode output, the input gradient and every parameter gradient for a stored random
    cotangent (a sum() of the outputs has no gradient behind the final BatchNorm), the buffers afterwards, the evaluation-mode
    output, and the ``manipulate`` output for two references mixed with a stored ``alpha``.
(b) ``emb.*``: MSMCVQGANEmb (reference msmc_vqgan_emb.py:123-291) with small_emb's configuration at n_model_size 64, mel_dim 24
    and the global encoder on: training-mode forward over windows with ``mel`` as the reference input, the gradients of a scalar
    of the outputs with respect to the embeddings and to ``mel``, evaluation-mode analysis -> synthesis(ref=...), window='full'.
Data only; no reference source.
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

from make_golden_emb import EMB_CFG, WINDOWS  # noqa: E402
from msmctts.networks.vqgantts.msmc_vqgan_emb import MSMCVQGANEmb  # noqa: E402
from msmctts.networks.vqgantts.tdnn import ECAPA_TDNN  # noqa: E402
from msmctts.utils.config import Config  # noqa: E402

ENC_CFG = dict(in_channels=24, embd_dim=64, channels=64)
EMB_ECAPA_CFG = dict(copy.deepcopy(EMB_CFG), n_model_size=64, mel_dim=24, global_encoder_config={'_name': 'ECAPA_TDNN'})
EMB_ECAPA_CFG['quantizer_config']['embedding_dims'] = 64
EMB_ECAPA_CFG['decoder_config']['upsample_initial_channel'] = 32


def fp16_representable(m):
    with torch.no_grad():
        for t in list(m.parameters()) + list(m.buffers()):
            if t.is_floating_point():
                t.copy_(t.half().float())


def store16(v):
    a = G.npy(v)
    return a.astype(np.float16) if a.dtype.kind == 'f' else a.copy()


def encoder(out):
    torch.manual_seed(1357)
    m = ECAPA_TDNN(**ENC_CFG)
    with torch.no_grad():                                 # BatchNorm parameters and buffers off their initial 1 / 0
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0.0, 0.2)
                mod.running_mean.normal_(0.0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    fp16_representable(m)
    out['enc.cfg'] = np.frombuffer(json.dumps(ENC_CFG).encode(), dtype=np.uint8)
    for k, v in m.state_dict().items():
        out['enc.state.' + k] = store16(v)
    STATE.append(copy.deepcopy(m.state_dict()))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 37, 24, generator=g)
    cot = torch.randn(3, 64, generator=g)
    x2 = torch.randn(3, 29, 24, generator=g)
    alpha = torch.softmax(torch.randn(3, 2, 1, generator=g), dim=1)
    for k, v in (('x', x), ('cotangent', cot), ('x2', x2), ('alpha', alpha)):
        out['enc.' + k] = G.npy(v)
    m.train()
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * cot).sum().backward()
    out['enc.train.y'] = G.npy(y)
    out['enc.train.grad_x'] = G.npy(xi.grad)
    for k, p in m.named_parameters():
        if p.numel() > 8192:
            out['enc.train.grad4.' + k] = G.npy(p.grad).reshape(-1)[::4].copy()
        else:
            out['enc.train.grad.' + k] = G.npy(p.grad)
    for k, v in m.named_buffers():
        out['enc.after.' + k] = G.npy(v).copy()
    m.eval()
    with torch.no_grad():
        out['enc.eval.y'] = G.npy(m(x))
        out['enc.eval.manipulate'] = G.npy(m(([x, x2], alpha)))


def autoencoder(out, enc_state):
    torch.manual_seed(2468)
    cfg = copy.deepcopy(EMB_ECAPA_CFG)
    cfg['global_encoder_config'] = Config(cfg['global_encoder_config'])
    m = MSMCVQGANEmb(**cfg)
    G.zero_dropout(m)
    m.global_encoder.load_state_dict(enc_state)           # (a)'s weights: not stored twice
    fp16_representable(m)
    out['emb.cfg'] = np.frombuffer(json.dumps(EMB_ECAPA_CFG).encode(), dtype=np.uint8)
    out['emb.windows'] = np.asarray(WINDOWS, dtype=np.int64)
    for k, v in m.state_dict().items():
        out['emb.state.' + k] = store16(v) if not k.startswith('global_encoder.') else np.zeros(0, dtype=np.float16)
    g = torch.Generator().manual_seed(5)
    lengths = torch.tensor([24, 17, 9], dtype=torch.int64)
    emb = torch.randn(3, 24, 24, generator=g)
    pitch, energy = torch.randn(3, 24, 1, generator=g), torch.rand(3, 24, 1, generator=g)
    mel = torch.randn(3, 24, 24, generator=g)
    for i, n in enumerate(lengths.tolist()):
        emb[i, n:], pitch[i, n:], energy[i, n:] = 0.0, 0.0, 0.0
    # (mel is left dense: all-zero frames leave channels of the encoder with one or two positive frames per batch, where the
    #  BatchNorm gradient is the difference of nearly equal numbers and two correct fp32 implementations disagree)
    for k, v in (('emb', emb), ('emb_length', lengths), ('pitch', pitch), ('energy', energy), ('mel', mel)):
        out['emb.batch.' + k] = G.npy(v)

    def put(prefix, d):
        for k, v in d.items():
            if torch.is_tensor(v):
                out['%s.%s' % (prefix, k)] = G.npy(v)
            elif isinstance(v, (tuple, list)):
                for i, t in enumerate(v):
                    if torch.is_tensor(t):
                        out['%s.%s.%d' % (prefix, k, i)] = G.npy(t)
            elif isinstance(v, dict):
                put('%s.%s' % (prefix, k), v)

    m.train()
    e, r = emb.clone().requires_grad_(True), mel.clone().requires_grad_(True)
    o = m(e, lengths, pitch, energy, mel=r, window=WINDOWS)
    put('emb.train', o)
    scalar = (o['decoder_outputs'].pow(2).mean() + o['mel_outputs'].mean() + sum(d.mean() for d in o['encoder_diffs'])
              + o['decoder_diffs']['total_loss'] + o['content_representations'].mean())
    scalar.backward()
    out['emb.train.scalar'] = G.npy(scalar)
    out['emb.train.grad_emb'] = G.npy(e.grad)
    out['emb.train.grad_mel'] = G.npy(r.grad)
    for k, v in m.state_dict().items():
        if 'quantizer.quantizer' in k or ('global_encoder' in k and ('running' in k or 'num_batches' in k)):
            out['emb.after.' + k] = G.npy(v).copy()
    m.eval()
    with torch.no_grad():
        qs = m.analysis(emb, lengths, pitch, energy)
        put('emb.eval_analysis', qs)
        out['emb.eval.wav'] = G.npy(m.synthesis(qs, qs['quantizer_lengths'], ref=mel))
        out['emb.eval.full.decoder_outputs'] = G.npy(m(emb, lengths, pitch, energy, ref=mel)['decoder_outputs'])


def main():
    for name, fill in (('small_ecapa.npz', encoder), ('small_ecapa_emb.npz', lambda o: autoencoder(o, STATE[0]))):
        out = {}
        fill(out)
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        print('wrote %s: %d arrays, %d bytes' % (name, len(out), os.path.getsize(path)))


STATE = []


if __name__ == '__main__':
    main()
