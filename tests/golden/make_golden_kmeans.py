#!/usr/bin/env python
"""Golden fixture for the k-means unit synthesiser, generated from the reference itself.

    python tests/golden/make_golden_kmeans.py        # writes tests/golden/small_kmeans.npz

A small KMeansVQGANEmb (reference networks/vqgantts/msmc_vqgan_emb.py:294-469): emb_dim 272, 24 centroids, n_model_size 64,
mel_dim 24, with the global encoder, a frame decoder and ``pred_mel``.  The centroid file the reference unpickles is written
here, into a temporary directory, from a small class of this script.  Evaluation mode: forward with window='full', forward
over a window list, and analysis -> synthesis(ref=mel) (which quantises its inputs again).

Size: the weights are rounded to fp16-representable values BEFORE the reference runs and stored as float16 (lossless); the
global encoder takes the weights of small_ecapa.npz (``enc.state.*``, same sizes) and is not stored again.  The inputs are
frames near the centroids (a quarter N(0, 1)), rounded to fp16-representable values as well.
Data only; no reference source.
"""
import copy
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shims)

import torch  # noqa: E402

from make_golden_ecapa import fp16_representable, store16  # noqa: E402
from make_golden_emb import FFT, WINDOWS  # noqa: E402
from msmctts.networks.vqgantts.msmc_vqgan_emb import KMeansVQGANEmb  # noqa: E402
from msmctts.utils.config import Config  # noqa: E402

EMB_DIM, K = 272, 24
KMEANS_CFG = dict(emb_dim=EMB_DIM, n_model_size=64, global_encoder_config={'_name': 'ECAPA_TDNN'},
                  frame_decoder_config=dict(FFT), pred_mel=True, mel_dim=24,
                  decoder_config=dict(upsample_rates=[5, 4, 2], upsample_kernel_sizes=[11, 8, 4], upsample_initial_channel=32,
                                      resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]]))


class KMeansModel(object):
    """stands in for the scikit-learn model the reference unpickles: it reads ``cluster_centers_`` only"""

    def __init__(self, centers):
        self.cluster_centers_ = centers


def main():
    g = torch.Generator().manual_seed(97)
    centers = torch.randn(K, EMB_DIM, generator=g).half().float()
    lengths = torch.tensor([24, 17, 9], dtype=torch.int64)
    B, T = 3, 24
    emb = torch.randn(B, T, EMB_DIM, generator=g)
    a = torch.randint(0, K, (B, T), generator=g)
    b = (a + 1 + torch.randint(0, K - 1, (B, T), generator=g)) % K
    t = 0.25 + 0.23 * torch.rand(B, T, 1, generator=g)
    near = centers[a] + t * (centers[b] - centers[a]) + 0.1 * emb
    random_frames = (torch.arange(B * T).view(B, T) % 4 == 0).unsqueeze(-1)
    emb = torch.where(random_frames, emb, near).half().float()
    mel = torch.randn(B, T, 24, generator=g).half().float()
    for i, n in enumerate(lengths.tolist()):
        emb[i, n:] = 0.0
    enc_state = {k[len('enc.state.'):]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v)
                 for k, v in np.load(os.path.join(HERE, 'small_ecapa.npz')).items() if k.startswith('enc.state.')}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'kmeans.pkl')
        with open(path, 'wb') as fout:
            pickle.dump(KMeansModel(centers.numpy()), fout)
        torch.manual_seed(1212)
        cfg = copy.deepcopy(KMEANS_CFG)
        cfg['global_encoder_config'] = Config(cfg['global_encoder_config'])
        m = KMeansVQGANEmb(quantizer_path=path, **cfg)
    G.zero_dropout(m)
    m.global_encoder.load_state_dict(enc_state)
    fp16_representable(m)
    out = {'cfg': np.frombuffer(json.dumps(KMEANS_CFG).encode(), dtype=np.uint8), 'windows': np.asarray(WINDOWS, dtype=np.int64),
           'centers': G.npy(centers)}
    for k, v in m.state_dict().items():
        out['state.' + k] = store16(v) if not k.startswith('global_encoder.') else np.zeros(0, dtype=np.float16)
    for k, v in (('emb', emb), ('emb_length', lengths), ('mel', mel)):
        out['batch.' + k] = G.npy(v)
    m.eval()
    with torch.no_grad():
        for tag, window in (('full', 'full'), ('window', WINDOWS)):
            o = m(emb, lengths, mel=mel, window=window)
            assert set(o) == {'encoder_indices', 'mel_outputs', 'decoder_outputs'}
            out[tag + '.encoder_indices.0'] = G.npy(o['encoder_indices'][0])
            out[tag + '.mel_outputs'] = G.npy(o['mel_outputs'])
            out[tag + '.decoder_outputs'] = G.npy(o['decoder_outputs'])
        qs = m.analysis(emb, lengths)
        out['eval.synthesis'] = G.npy(m.synthesis(list(qs['quantizer_outputs']), qs['quantizer_lengths'], ref=mel))
    path = os.path.join(HERE, 'small_kmeans.npz')
    np.savez_compressed(path, **out)
    print('wrote small_kmeans.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
