#!/usr/bin/env python
"""Golden fixture for the single-channel spectral domains of the resolution discriminators, generated from the reference itself.

    python tests/golden/make_golden_mrd_domains.py        # writes tests/golden/small_mrd_domains.npz

The reference's MultiResolutionDiscriminator (networks/hifigan/discriminator.py:79-116) with ``domain`` in {'linear', 'log'} x
``mel_scale`` in {True, False}: hop lengths 15 / 50 / 240 (F = 31 / 101 / 481), the hidden width of the small discriminator of
make_golden.py (32), ONE seeded state_dict for all four cases (the single-channel stacks have the same shapes), B = 3 waveforms
of L = 2410 samples (no multiple of any hop, above the largest reflection pad of 480) with a loud, a decaying and a partly silent
row, so that the log channel meets both clamp edges.  Stored per case: every score, a digest of every feature map (mean, mean
absolute value, standard deviation, element count, and DIGEST_SAMPLES evenly spaced elements over the WHOLE map -- the full maps
of four cases are 3.5 MB), the gradient of sum(score^2) with respect to the waveform and to the three parameters of each
stack's first convolution.  Data only; no reference source.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shims)

import torch  # noqa: E402

from msmctts.networks.hifigan.discriminator import MultiResolutionDiscriminator  # noqa: E402

HOPS = [15, 50, 240]
HIDDEN = [G.SMALL_TASK['discriminator']['mrd_config']['hidden_channels'][0]] * len(HOPS)
B, L = 3, 2410
DIGEST_SAMPLES = 384
CASES = [(d, m) for d in ('linear', 'log') for m in (True, False)]


def digest(t):
    """[mean, mean |.|, std, count, DIGEST_SAMPLES elements at evenly spaced flat positions (first and last included)]"""
    f = t.detach().reshape(-1).double()
    idx = np.unique(np.linspace(0, f.numel() - 1, DIGEST_SAMPLES).round().astype(np.int64))
    return np.concatenate([[f.mean().item(), f.abs().mean().item(), f.std().item(), float(f.numel())],
                           f[torch.from_numpy(idx)].numpy()]).astype(np.float64)


def waveforms():
    g = torch.Generator().manual_seed(77)
    n = torch.randn(B, L, generator=g)
    tt = torch.arange(L, dtype=torch.float32)
    wav = torch.empty(B, L)
    wav[0] = 6.0 * n[0] + 3.0 * torch.sin(2 * np.pi * 440.0 / 24000.0 * tt)        # loud: above the upper clamp edge
    wav[1] = n[1] * torch.exp(-tt / L * 12.0)                                      # decaying over five decades
    wav[2] = 0.3 * n[2]
    wav[2, 900:1700] = 0.0                                                         # a silent stretch longer than any frame
    return wav


def main():
    out = {'hops': np.asarray(HOPS, dtype=np.int64), 'hidden': np.asarray(HIDDEN, dtype=np.int64),
           'digest_samples': np.asarray(DIGEST_SAMPLES, dtype=np.int64)}
    wav = waveforms()
    out['wav'] = G.npy(wav)
    torch.manual_seed(4321)
    seed_model = MultiResolutionDiscriminator(hop_lengths=HOPS, hidden_channels=HIDDEN, domain='linear', mel_scale=True)
    with torch.no_grad():                  # weight_norm initialises g = |v|: move it, so that a wrong g shows
        for k, p in seed_model.named_parameters():
            if k.endswith('weight_g'):
                p.mul_(0.75 + 0.5 * torch.rand(p.shape))
    state = {k: v.detach().clone() for k, v in seed_model.state_dict().items()}
    for k, v in state.items():
        out['state.' + k] = G.npy(v).copy()
    for domain, mel_scale in CASES:
        tag = '%s.%s' % (domain, 'mel' if mel_scale else 'plain')
        m = MultiResolutionDiscriminator(hop_lengths=HOPS, hidden_channels=HIDDEN, domain=domain, mel_scale=mel_scale)
        m.load_state_dict(state)
        x = wav.clone().requires_grad_(True)
        scores, fmaps = m(x.unsqueeze(1))
        assert len(scores) == len(HOPS) and all(len(f) == 6 for f in fmaps)
        sum(s.pow(2).sum() for s in scores).backward()
        for i, s in enumerate(scores):
            out['%s.score.%d' % (tag, i)] = G.npy(s)
            for j, f in enumerate(fmaps[i]):
                out['%s.fmap.%d.%d' % (tag, i, j)] = digest(f).astype(np.float32)
                out['%s.fmap_shape.%d.%d' % (tag, i, j)] = np.asarray(f.shape)
        out['%s.grad_wav' % tag] = G.npy(x.grad)
        for n, p in m.named_parameters():
            if '.discriminator.0.1.' in n:
                out['%s.grad.%s' % (tag, n)] = G.npy(p.grad)
    path = os.path.join(HERE, 'small_mrd_domains.npz')
    np.savez_compressed(path, **out)
    print('wrote small_mrd_domains.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
