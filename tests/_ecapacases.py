"""Shared module-level cases of the speaker reference encoder against the reference's own outputs (tests/golden/small_ecapa.npz
and small_ecapa_emb.npz, written by tests/golden/make_golden_ecapa.py): tests/test_ecapa.py runs them on the kernel interpreter,
tests/test_gpu_tdnn.py on the GPU.  Tolerances are check_emb_autoencoder's: ``close`` at 1e-3 (gradients: 1e-3 of the largest
entry), VQ indices exact, running buffers 1e-5."""
import json

import numpy as np
import pytest
import torch

from _parity import close, load_npz, t


# The softmax over frames does not see a per-channel constant, so the gradient of the bias behind the logits is identically zero:
# the reference's stored values are rounding noise of its own summation order (1e-7 next to terms of 1e-1), and 1e-3 of their
# largest entry is no scale.  The bias is the layer's weight for a constant input 1, so its gradient is held to the scale of
# the same layer's weight gradient.
ZERO_GRADIENT = {'pooling.linear2.bias': 'enc.train.grad4.pooling.linear2.weight',
                 # ... and a constant added in front of a training-mode BatchNorm (bn2) is removed by its mean subtraction
                 'bn1.bias': 'enc.train.grad.bn1.weight', 'linear.bias': 'enc.train.grad4.linear.weight'}


def _cfg(raw):
    return json.loads(bytes(raw).decode())


def _grad_tol(want):
    return 1e-3 * max(1e-6, float(np.abs(want).max())) + 1e-7


def build_encoder(device, z=None):
    from msmctts_amd.networks.vqgantts.tdnn import ECAPA_TDNN
    z = load_npz('small_ecapa.npz') if z is None else z
    m = ECAPA_TDNN(**_cfg(z['enc.cfg']))
    want_keys = [k[len('enc.state.'):] for k in z if k.startswith('enc.state.')]
    assert list(m.state_dict().keys()) == want_keys                # the reference's keys, in its order, every buffer included
    m.load_state_dict({k: t(z['enc.state.' + k].astype(np.float32) if z['enc.state.' + k].dtype == np.float16
                            else z['enc.state.' + k]) for k in want_keys})
    return m.to(device), z


def check_encoder(device, use_hip=True):
    m, z = build_encoder(device)
    m.use_hip = use_hip
    x, cot = t(z['enc.x']).to(device), t(z['enc.cotangent']).to(device)
    m.train()
    xi = x.clone().requires_grad_(True)
    y = m(xi)
    (y * cot).sum().backward()
    close(y, z['enc.train.y'], what='train y')
    close(xi.grad, z['enc.train.grad_x'], _grad_tol(z['enc.train.grad_x']), what='grad x')
    seen = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if 'enc.train.grad.' + k in z:
            want, got = z['enc.train.grad.' + k], p.grad
        else:                                                      # the four large tensors: every 4th element
            want, got = z['enc.train.grad4.' + k], p.grad.reshape(-1)[::4]
        close(got, want, _grad_tol(z[ZERO_GRADIENT[k]] if k in ZERO_GRADIENT else want), what='grad ' + k)
        seen += 1
    assert seen == len(list(m.parameters())) >= 100
    for k, v in m.named_buffers():
        ref = z['enc.after.' + k]
        close(v, ref, 1e-5 * max(1.0, float(np.abs(ref).max())), 1e-5, what='buffer ' + k)
    m.eval()
    with torch.no_grad():
        close(m(x), z['enc.eval.y'], what='eval y')
        close(m(([x, t(z['enc.x2']).to(device)], t(z['enc.alpha']).to(device))), z['enc.eval.manipulate'], what='manipulate')


def check_paths_agree(device):
    """use_hip = True and use_hip = False on the same weights, fp32: outputs and gradients"""
    res = []
    for hip in (True, False):
        m, z = build_encoder(device)
        m.use_hip = hip
        m.train()
        xi = t(z['enc.x']).to(device).requires_grad_(True)
        y = m(xi)
        (y * t(z['enc.cotangent']).to(device)).sum().backward()
        res.append((y.detach(), xi.grad, {k: p.grad for k, p in m.named_parameters()}, dict(m.named_buffers())))
    (ya, ga, pa, ba), (yb, gb, pb, bb) = res
    close(ya, yb, what='y')
    close(ga, gb, _grad_tol(gb.cpu().numpy()), what='grad x')
    for k in pa:
        scale = pb[ZERO_GRADIENT[k].split('.', 3)[3]] if k in ZERO_GRADIENT else pb[k]
        close(pa[k], pb[k], _grad_tol(scale.cpu().numpy()), what='grad ' + k)
    for k in ba:
        close(ba[k], bb[k], 1e-5, 1e-5, what='buffer ' + k)


def check_construction_and_path_policy(device):
    from msmctts_amd.hip import lib
    from msmctts_amd.networks.vqgantts.tdnn import ECAPA_TDNN
    with pytest.raises(NotImplementedError, match='channels'):
        ECAPA_TDNN(in_channels=24, embd_dim=32, channels=32)
    with pytest.raises(NotImplementedError, match='in_channels'):
        ECAPA_TDNN(in_channels=20, embd_dim=64, channels=64)
    m = ECAPA_TDNN(in_channels=24, embd_dim=64, channels=64)
    assert m.use_hip is True
    saved = lib._host_pointers_ok
    lib._host_pointers_ok = False
    try:
        with pytest.raises(RuntimeError, match='gfx950 kernels only'):         # no silent fallback off the GPU
            m(torch.zeros(2, 9, 24))
    finally:
        lib._host_pointers_ok = saved


def build_autoencoder(device):
    from msmctts_amd.networks import find_modules
    z, ze = load_npz('small_ecapa_emb.npz'), load_npz('small_ecapa.npz')
    cfg = _cfg(z['emb.cfg'])
    (_, m), = find_modules({'autoencoder': dict(cfg, _name='MSMCVQGANEmb')})
    want_keys = [k[len('emb.state.'):] for k in z if k.startswith('emb.state.')]
    assert list(m.state_dict().keys()) == want_keys
    keys = list(m.state_dict().keys())
    enc = [i for i, k in enumerate(keys) if k.startswith('global_encoder.')]
    assert keys[enc[0] - 1].startswith('encoder.') and keys[enc[-1] + 1].startswith('quantizer.')

    def val(k):
        a = ze['enc.state.' + k[len('global_encoder.'):]] if k.startswith('global_encoder.') else z['emb.state.' + k]
        return t(a.astype(np.float32) if a.dtype == np.float16 else a)
    m.load_state_dict({k: val(k) for k in want_keys})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.to(device), z, cfg


def check_autoencoder(device, encoder_use_hip=True):
    from msmctts_amd.networks import find_modules
    m, z, cfg = build_autoencoder(device)
    m.global_encoder.use_hip = encoder_use_hip
    m.train()
    b = {k[len('emb.batch.'):]: t(v).to(device) for k, v in z.items() if k.startswith('emb.batch.')}
    windows = [tuple(int(v) for v in row) for row in z['emb.windows']]

    def compare(prefix, d):
        seen = 0
        for k, v in d.items():
            if torch.is_tensor(v):
                items = [('%s.%s' % (prefix, k), v)]
            elif isinstance(v, (tuple, list)):
                items = [('%s.%s.%d' % (prefix, k, i), x) for i, x in enumerate(v) if torch.is_tensor(x)]
            elif isinstance(v, dict):
                seen += compare('%s.%s' % (prefix, k), v)
                continue
            else:
                continue
            for name, got in items:
                want = z[name]
                if 'indices' in name or 'lengths' in name:
                    assert np.array_equal(got.cpu().numpy(), want), name
                else:
                    close(got, want, what=name)
                seen += 1
        return seen

    e, r = b['emb'].clone().requires_grad_(True), b['mel'].clone().requires_grad_(True)
    o = m(e, b['emb_length'], b['pitch'], b['energy'], mel=r, window=windows)
    assert compare('emb.train', o) >= 13
    scalar = (o['decoder_outputs'].pow(2).mean() + o['mel_outputs'].mean() + sum(d.mean() for d in o['encoder_diffs'])
              + o['decoder_diffs']['total_loss'] + o['content_representations'].mean())
    scalar.backward()
    close(scalar, z['emb.train.scalar'], what='scalar')
    close(e.grad, z['emb.train.grad_emb'], _grad_tol(z['emb.train.grad_emb']), what='grad emb')
    close(r.grad, z['emb.train.grad_mel'], _grad_tol(z['emb.train.grad_mel']), what='grad mel')
    sd = m.state_dict()
    for k in z:
        if k.startswith('emb.after.'):
            ref = z[k]
            close(sd[k[len('emb.after.'):]], ref, 1e-5 * max(1.0, float(np.abs(ref).max())), 1e-5, what=k)
    m.eval()
    with torch.no_grad():
        qs = m.analysis(b['emb'], b['emb_length'], b['pitch'], b['energy'])
        assert compare('emb.eval_analysis', qs) >= 8
        close(m.synthesis(qs, qs['quantizer_lengths'], ref=b['mel']), z['emb.eval.wav'], what='synthesis(ref)')
        close(m(b['emb'], b['emb_length'], b['pitch'], b['energy'], ref=b['mel'])['decoder_outputs'],
              z['emb.eval.full.decoder_outputs'], what="window='full'")
        with pytest.raises(AssertionError):
            m.synthesis(qs, qs['quantizer_lengths'])
    with pytest.raises(ValueError, match='Wrong global encoder'):
        find_modules({'autoencoder': dict(cfg, _name='MSMCVQGANEmb', global_encoder_config={'_name': 'XVectorTDNN'})})
    with pytest.raises(NotImplementedError):
        find_modules({'autoencoder': dict(cfg, _name='MSMCVQGANEmb', n_model_size=32)})
