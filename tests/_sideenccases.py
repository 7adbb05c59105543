"""Shared cases of the pitch / energy side encoder on the kernels (csrc/side_enc.hip, hip/side_enc.py, ``MAMSEncoder.fused_side``), of
``EmbVC`` against the reference's own outputs (tests/golden/small_vc.npz, written by tests/golden/make_golden_vc.py) and of
``EmbVQGANTrainer`` over both: tests/test_side_enc_emu.py runs them on the kernel interpreter, tests/test_gpu_side_enc.py on the GPU.

Reference of the kernel comparisons: a float64 numpy restatement from the same fp32 / bf16 input bits.  Every output is pre-filled
with NaN and none may remain, every output carries guard elements behind its end (tests/_normcases.py ``Out``), every case runs
twice and the two results must agree bit for bit (``dw`` / ``db`` among them).  u = 2^-24, ub = 2^-8 (a bf16 rounding is within
half an ulp, at most ub |v|, of v).  The bounds, from the order the source documents:

  front fwd   z = bias + n products added one at a time, n = (P + E) taps: every product within u of itself, every one of the n
              partial sums within u of itself and at most S = |bias| + sum |w x| in size: |z - z64| <= E_z = (n + 1) u S (1 + 2^-16)
              (the factor covers the second-order terms: (n + 1) u < 2^-17).  tanh is 1-Lipschitz: E_z carries over.  tanhf is
              library code: its bound is the yardstick of tests/_normcases.py (``yard``: RATIO = 4 x the error of torch's own fp32
              tanh on the CPU against float64), taken here in the max norm at the same pre-activations rounded to fp32:
              Y = RATIO max |torch.tanh(z32) - tanh(z32 in float64)|.  A bf16 output adds its half ulp (``half_ulp``).
              |y - tanh(z64)| <= E_z + Y + half.
  front bwd   dz = gy (1 - y y) in three roundings: e_dz = |gy| (u y^2 + 2 u |1 - y^2|) (1 + 2^-20), the tanh_bwd bound of
              tests/_normcases.py.  A weight-gradient element adds N = B T products: each within u of itself, and a term passes
              through at most 32 additions in its tile and one per tile in the second launch, D = 33 + tiles additions with the
              +0 starts: |dw - dw64| <= (sum e_dz |x| + (D + 1) u sum |dz x|) (1 + 2^-12); db the same with x = 1 and no
              product rounding.
  pool fwd    a window of n frames: n - 1 additions and the quotient: E_p = mean(e_in) + n u mean |side| (1 + 2^-20) with e_in the
              bound the input carries (0 for a first stage).  out in fp32: one addition, E_p + u |out|; in bf16: the pooled value
              rounded, then the sum rounded: E_p (1 + ub) + ub (|p| + (|out| + ub |p| + E_p)) (1 + ub).
  pool bwd    one addition and one quotient: 2 u |ref| (1 + 2^-20) (a bf16 gout widens exactly).
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _normcases import E_SHAPE, RATIO, U, Out, at, gen_for, half_ulp, held
from _parity import close, load_npz, t
from _spectralcases import twice

UB = 2.0 ** -8
DTYPES = ((0, torch.float32, 'fp32'), (1, torch.bfloat16, 'bf16'))
FRONT_T = (1, 2, 3, 4, 7, 65, 401)
FRONT_B = (1, 3)
FRONT_PE = ((1, 1), (1, 0), (0, 1), (2, 1))
FRONT_C = (8, 32, 256)
TAPS = 7
FRONT_CASES = ['T%d-C%d' % (T, C) for T in FRONT_T for C in FRONT_C]
POOL_SCALES = (1, 2, 3, 4)
SF_FT = 32                     # frames of a tile (csrc/side_enc.hip)


def L():
    from msmctts_amd.hip import lib
    return lib


def pool_tins(scale):
    return sorted(set(n for n in (1, scale - 1, scale, scale + 1, 4 * scale + 1, 401) if n >= 1))


# ---- front kernel ------------------------------------------------------------------------------------------------------------------
def front_ref(pitch, energy, w, b):
    """z64 [B, T, C], S = |b| + sum |w x|, and the zero-padded input x [B, T + taps - 1, Cin], all float64"""
    x = torch.cat([v.double() for v in (pitch, energy) if v is not None], dim=-1)
    taps = w.shape[2]
    pad = (taps - 1) // 2
    xp = F.pad(x, (0, 0, pad, pad))
    T = x.shape[1]
    win = torch.stack([xp[:, k:k + T] for k in range(taps)], dim=-1)               # [B, T, Cin, taps]
    z = torch.einsum('btik,cik->btc', win, w.double()) + b.double()
    S = torch.einsum('btik,cik->btc', win.abs(), w.double().abs()) + b.double().abs()
    return z, S, win


def check_front(dev, T, C):
    lib = L()
    for B in FRONT_B:
        for P, E in FRONT_PE:
            gen = gen_for(T, C, B, P, E)
            pitch = torch.randn(B, T, P, generator=gen) if P else None
            energy = torch.rand(B, T, E, generator=gen) if E else None
            w = torch.randn(C, P + E, TAPS, generator=gen) * 0.4
            b = torch.randn(C, generator=gen) * 0.3
            z64, S, win = front_ref(pitch, energy, w, b)
            n = (P + E) * TAPS
            e_z = (n + 1) * U * S * (1 + 2.0 ** -16)
            z32 = z64.float()
            yardstick = RATIO * float((torch.tanh(z32).double() - torch.tanh(z32.double())).abs().max())
            want = torch.tanh(z64)
            pd, ed, wd, bd = at(pitch, dev), at(energy, dev), at(w, dev), at(b, dev)
            tiles = (T + SF_FT - 1) // SF_FT
            for code, dtype, name in DTYPES:
                tag = 'B%d T%d P%d E%d C%d %s' % (B, T, P, E, C, name)

                def fwd():
                    y = Out((B, T, C), dev, dtype)
                    lib.call('msmc_side_front_fwd', lib.ptr(pd), lib.ptr(ed), lib.ptr(wd), lib.ptr(bd), lib.ptr(y.t), code, B, T, P, E, C,
                             TAPS, lib.stream(wd))
                    return (y.get(),)

                y, = twice(fwd)
                held('front fwd', tag, y, want, e_z + yardstick + half_ulp(want, dtype))
                assert bool((y.float().abs() <= 1).all())
                # backward from the kernel's own y and a random cotangent in y's dtype
                gy = torch.randn(B, T, C, generator=gen).to(dtype)
                yd, gd = at(y, dev), at(gy, dev)
                nbytes = int(lib.get().msmc_side_front_bwd_workspace(B, T, P, E, C, TAPS))
                assert nbytes == B * tiles * (C * n + C) * 4
                ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32).to(dev)

                def bwd():
                    dw, db = Out((C, P + E, TAPS), dev), Out((C,), dev)
                    lib.call('msmc_side_front_bwd', lib.ptr(pd), lib.ptr(ed), lib.ptr(yd), lib.ptr(gd), code, lib.ptr(dw.t), lib.ptr(db.t),
                             lib.ptr(ws), nbytes, B, T, P, E, C, TAPS, lib.stream(wd))
                    return dw.get(), db.get()

                dw, db = twice(bwd)
                y64, g64 = y.double(), gy.double()
                dz = g64 * (1 - y64 * y64)
                e_dz = g64.abs() * (U * y64 * y64 + 2 * U * (1 - y64 * y64).abs()) * (1 + 2.0 ** -20)
                D = 33 + B * tiles
                dw64 = torch.einsum('btc,btik->cik', dz, win)
                bound = (torch.einsum('btc,btik->cik', e_dz, win.abs())
                         + (D + 1) * U * torch.einsum('btc,btik->cik', dz.abs(), win.abs())) * (1 + 2.0 ** -12)
                held('front bwd dw', tag, dw, dw64, bound)
                held('front bwd db', tag, db, dz.sum((0, 1)), (e_dz.sum((0, 1)) + D * U * dz.abs().sum((0, 1))) * (1 + 2.0 ** -12))


def check_front_workspace_refused(dev):
    """a workspace one byte short: MSMC_E_WORKSPACE, nothing written"""
    lib = L()
    B, T, P, E, C = 1, 5, 1, 1, 8
    gen = gen_for(5, 8)
    pd, ed = at(torch.randn(B, T, P, generator=gen), dev), at(torch.randn(B, T, E, generator=gen), dev)
    yd = at(torch.rand(B, T, C, generator=gen), dev)
    nbytes = int(lib.get().msmc_side_front_bwd_workspace(B, T, P, E, C, TAPS))
    ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32).to(dev)
    dw, db = Out((C, P + E, TAPS), dev), Out((C,), dev)
    rc = lib.get().msmc_side_front_bwd(lib.ptr(pd), lib.ptr(ed), lib.ptr(yd), lib.ptr(yd), 0, lib.ptr(dw.t), lib.ptr(db.t), lib.ptr(ws),
                                       nbytes - 1, B, T, P, E, C, TAPS, lib.stream(yd))
    assert rc == -3
    assert bool(torch.isnan(dw.get(written=False)).all()) and bool(torch.isnan(db.get(written=False)).all())


# ---- pooling + addition ------------------------------------------------------------------------------------------------------------
def pool_ref(side64, e_in, scale):
    """float64 ceil-mode mean over windows of ``scale`` frames of [B, Tin, C], and the bound E_p of the module docstring"""
    B, Tin, C = side64.shape
    Tout = -(-Tin // scale)
    p, e = torch.zeros(B, Tout, C, dtype=torch.float64), torch.zeros(B, Tout, C, dtype=torch.float64)
    for u in range(Tout):
        blk = slice(u * scale, min(Tin, (u + 1) * scale))
        n = blk.stop - blk.start
        p[:, u] = side64[:, blk].sum(1) / n
        e[:, u] = e_in[:, blk].mean(1) + n * U * side64[:, blk].abs().mean(1) * (1 + 2.0 ** -20)
    return p, e


def out_bound(p64, e_p, out64, dtype):
    if dtype == torch.float32:
        return e_p + U * out64.abs() * (1 + 2.0 ** -20)
    return e_p * (1 + UB) + UB * (p64.abs() + (out64.abs() + UB * p64.abs() + e_p)) * (1 + UB)


def run_pool(dev, side, feat, scale):
    """(pooled or None, out) through the C entry, twice"""
    lib = L()
    B, Tin, C = side.shape
    Tout = feat.shape[1]
    code = 0 if feat.dtype == torch.float32 else 1
    sd, fd = at(side, dev), at(feat, dev)

    def fwd():
        pooled, out = Out((B, Tout, C), dev), Out((B, Tout, C), dev, feat.dtype)
        lib.call('msmc_pool_add_fwd', lib.ptr(sd), lib.ptr(fd), code, lib.ptr(pooled.t), lib.ptr(out.t), B, Tin, Tout, C, scale, lib.stream(sd))
        return pooled.get(written=scale > 1), out.get()

    pooled, out = twice(fwd)
    if scale == 1:
        assert bool(torch.isnan(pooled).all()), 'scale 1 wrote pooled'
        return None, out
    return pooled, out


def check_pool(dev, scale):
    lib = L()
    for Tin in pool_tins(scale):
        Tout = -(-Tin // scale)
        for B, C in ((1, 8), (3, 20), (2, 7), (1, 256)):
            for code, dtype, name in DTYPES:
                gen = gen_for(scale, Tin, B, C, code)
                tag = 'scale %d Tin %d B%d C%d %s' % (scale, Tin, B, C, name)
                side = torch.randn(B, Tin, C, generator=gen)
                feat = torch.randn(B, Tout, C, generator=gen).to(dtype)
                pooled, out = run_pool(dev, side, feat, scale)
                p64, e_p = pool_ref(side.double(), torch.zeros(B, Tin, C, dtype=torch.float64), scale)
                if scale == 1:
                    p64, e_p = side.double(), torch.zeros_like(p64)
                else:
                    held('pool fwd pooled', tag, pooled, p64, e_p)
                    want = F.avg_pool1d(side.double().transpose(1, 2), scale, scale, ceil_mode=True).transpose(1, 2)
                    assert float((want - p64).abs().max()) <= 1e-14, 'the restatement is not avg_pool1d(ceil_mode=True)'
                out64 = feat.double() + p64
                held('pool fwd out', tag, out, out64, out_bound(p64, e_p, out64, dtype))
                # backward: both gradients, gout alone, gpooled alone
                gout = torch.randn(B, Tout, C, generator=gen).to(dtype)
                gpool = torch.randn(B, Tout, C, generator=gen)
                cnt = torch.tensor([min(scale, Tin - (f // scale) * scale) for f in range(Tin)], dtype=torch.float64)[None, :, None]
                idx = torch.arange(Tin) // scale
                for which, go, gp in (('both', gout, gpool), ('gout', gout, None), ('gpooled', None, gpool)):
                    god, gpd = at(go, dev), at(gp, dev)

                    def bwd():
                        gs = Out((B, Tin, C), dev)
                        lib.call('msmc_pool_add_bwd', lib.ptr(god), code if go is not None else 0, lib.ptr(gpd), lib.ptr(gs.t), B, Tin, Tout,
                                 C, scale, lib.stream(gs.t))
                        return (gs.get(),)

                    gs, = twice(bwd)
                    tot = (go.double() if go is not None else 0) + (gp.double() if gp is not None else 0)
                    ref = tot[:, idx] / cnt
                    held('pool bwd ' + which, tag, gs, ref, 2 * U * ref.abs() * (1 + 2.0 ** -20))


def check_pool_chain(dev):
    """downsample_scales = [1, 4, 2]: the add of stage 0, then two pooled stages fed by each other, against F.avg_pool1d applied
    twice in float64; through hip/side_enc.py's pool_add, with the gradient of the side encoding through all three"""
    from msmctts_amd.hip import side_enc
    for Tin, B, C in ((401, 2, 64), (9, 1, 8), (1, 1, 8)):
        for code, dtype, name in DTYPES:
            gen = gen_for(401, Tin, code)
            tag = 'chain Tin %d %s' % (Tin, name)
            side = torch.randn(B, Tin, C, generator=gen)
            s64 = side.double()
            sd = side.to(dev).requires_grad_(True)
            cur, e_cur, cur64, Tcur = sd, torch.zeros_like(s64), s64, Tin
            outs, gouts = [], []
            for scale in (1, 4, 2):
                Tout = -(-Tcur // scale)
                feat = torch.randn(B, Tout, C, generator=gen).to(dtype)
                cur, out = side_enc.pool_add(cur, feat.to(dev), scale)
                if scale > 1:
                    want = F.avg_pool1d(cur64.transpose(1, 2), scale, scale, ceil_mode=True).transpose(1, 2)
                    cur64, e_cur = pool_ref(cur64, e_cur, scale)
                    assert float((want - cur64).abs().max()) <= 1e-14
                    held('chain pooled x%d' % scale, tag, cur.detach().cpu(), cur64, e_cur)
                out64 = feat.double() + cur64
                held('chain out x%d' % scale, tag, out.detach().cpu(), out64, out_bound(cur64, e_cur, out64, dtype))
                outs.append(out)
                gouts.append(torch.randn(B, Tout, C, generator=gen).to(dtype))
                Tcur = Tout
            torch.autograd.backward(outs, [g.to(dev) for g in gouts])
            s = s64.clone().requires_grad_(True)
            p4 = F.avg_pool1d(s.transpose(1, 2), 4, 4, ceil_mode=True)
            p8 = F.avg_pool1d(p4, 2, 2, ceil_mode=True)
            ((s * gouts[0].double()).sum() + (p4.transpose(1, 2) * gouts[1].double()).sum()
             + (p8.transpose(1, 2) * gouts[2].double()).sum()).backward()
            # three terms of at most two roundings each and two additions between them: 8 u of the sum of their magnitudes
            mag = (gouts[0].double().abs() + F.interpolate(gouts[1].double().abs().transpose(1, 2), scale_factor=4)[..., :Tin].transpose(1, 2)
                   + F.interpolate(gouts[2].double().abs().transpose(1, 2), scale_factor=8)[..., :Tin].transpose(1, 2))
            held('chain gside', tag, sd.grad.cpu(), s.grad, 8 * U * mag)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    lib = L()
    h = lib.get()
    B, T, C = 2, 9, 16
    gen = gen_for(77)
    x = at(torch.randn(B, T, 8, generator=gen), dev)                 # read as pitch and as energy: wide enough for every width tried
    w, b = at(torch.randn(C + 8, 9, 8, generator=gen), dev), at(torch.randn(C + 8, generator=gen), dev)
    big = at(torch.randn(B, T, C + 8, generator=gen), dev)
    ws = torch.empty(1 << 16, dtype=torch.float32).to(dev)
    st = lib.stream(x)
    for P, E, C_, taps in ((0, 0, C, 7), (5, 4, C, 7), (9, 0, C, 7), (1, 1, C, 6), (1, 1, C, 0), (1, 1, C, 17), (1, 1, C + 4, 7), (1, 1, 0, 7)):
        tag = 'P%d E%d C%d taps%d' % (P, E, C_, taps)
        for code, dtype, _ in DTYPES:
            y = Out((B, T, C + 8), dev, dtype)
            assert h.msmc_side_front_fwd(lib.ptr(x), lib.ptr(x), lib.ptr(w), lib.ptr(b), lib.ptr(y.t), code, B, T, P, E, C_, taps, st) == E_SHAPE, tag
            assert bool(torch.isnan(y.get(written=False).float()).all()), tag + ': a refused call launched'
            dw, db = Out((C + 8, 9, 17), dev), Out((C + 8,), dev)
            assert h.msmc_side_front_bwd(lib.ptr(x), lib.ptr(x), lib.ptr(big), lib.ptr(big), 0, lib.ptr(dw.t), lib.ptr(db.t), lib.ptr(ws),
                                         ws.numel() * 4, B, T, P, E, C_, taps, st) == E_SHAPE, tag
            assert bool(torch.isnan(dw.get(written=False)).all()) and bool(torch.isnan(db.get(written=False)).all()), tag
            assert int(h.msmc_side_front_bwd_workspace(B, T, P, E, C_, taps)) == 0, tag
    side = at(torch.randn(B, T, C, generator=gen), dev)
    for scale, Tout in ((0, T), (-1, T), (2, 4), (2, 6), (1, T - 1)):               # scale 0; Tout != ceil(Tin / scale)
        for code, dtype, _ in DTYPES:
            feat = at(torch.randn(B, T, C, generator=gen).to(dtype), dev)
            pooled, out, gs = Out((B, T, C), dev), Out((B, T, C), dev, dtype), Out((B, T, C), dev)
            assert h.msmc_pool_add_fwd(lib.ptr(side), lib.ptr(feat), code, lib.ptr(pooled.t), lib.ptr(out.t), B, T, Tout, C, scale, st) == E_SHAPE
            assert h.msmc_pool_add_bwd(lib.ptr(feat), code, lib.ptr(side), lib.ptr(gs.t), B, T, Tout, C, scale, st) == E_SHAPE
            for o in (pooled, out, gs):
                assert bool(torch.isnan(o.get(written=False).float()).all()), 'scale %d: a refused call launched' % scale


# ---- MAMSEncoder: fused against the stock chain ---------------------------------------------------------------------------------------
def _grad_tol(want):
    return 1e-3 * max(1e-6, float(want.abs().max())) + 1e-7


def build_encoder(dev, bf16, scales=(1, 2), C=64, P=1, E=1, seed=5):
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import MAMSEncoder
    torch.manual_seed(seed)
    m = MAMSEncoder(C, pitch_dim=P, energy_dim=E, downsample_scales=list(scales), max_seq_len=64, n_layers=1, n_head=2, d_k=64, d_v=64,
                    d_inner=64, fft_conv1d_kernel=3, fft_conv1d_padding=1, dropout=0.0, attn_dropout=0.0, fused_layernorm=False)
    if bf16:
        for mod in m.modules():
            if hasattr(mod, 'hip_dtype'):
                mod.hip_dtype = torch.bfloat16
    return m.to(dev).train()


def encoder_batch(dev, C=64, P=1, E=1, T=13, lengths=(13, 7, 4), seed=6):
    gen = torch.Generator().manual_seed(seed)
    B = len(lengths)
    ln = torch.tensor(lengths, dtype=torch.int64)
    valid = torch.arange(T)[None, :, None] < ln[:, None, None]
    emb = torch.where(valid, torch.randn(B, T, C, generator=gen), torch.zeros(()))
    pitch = torch.where(valid, torch.randn(B, T, P, generator=gen), torch.zeros(()))
    energy = torch.where(valid, torch.rand(B, T, E, generator=gen), torch.zeros(()))
    return emb.to(dev), ln.to(dev), pitch.to(dev), energy.to(dev)


def check_autograd(dev, bf16):
    """fused ``MAMSEncoder`` against ``fused_side = False`` on the same weights: every stage output, the content representation,
    the gradients of every ``pitch_encoder`` parameter and of ``emb``; tolerances of ``_parity.check_emb_autoencoder`` (outputs 1e-3,
    gradients 1e-3 of the largest entry)"""
    fused = build_encoder(dev, bf16, scales=(1, 2, 2))
    stock = copy.deepcopy(fused)
    stock.fused_side = False
    assert type(fused).fused_side is True and fused.fused_side
    emb, ln, pitch, energy = encoder_batch(dev)
    res = []
    for m in (fused, stock):
        e = emb.clone().requires_grad_(True)
        outs, content = m(e, ln, pitch, energy)
        gen = torch.Generator().manual_seed(9)
        loss = content.float().mean()
        for feat, _ in outs:
            loss = loss + (feat.float() * torch.randn(feat.shape, generator=gen).to(dev)).sum() / feat.shape[1]
        loss.backward()
        res.append((outs, content, e.grad, {k: p.grad for k, p in m.pitch_encoder.named_parameters()}))
    (fo, fc, fe, fg), (so, sc, se, sg) = res
    assert len(fg) == 8 and all(g is not None for g in fg.values())
    for i, ((a, la), (b, lb)) in enumerate(zip(fo, so)):
        assert a.dtype == b.dtype and torch.equal(la, lb)
        close(a.float(), b.float(), what='stage %d output' % i)
    close(fc.float(), sc.float(), what='content')
    close(fe, se, _grad_tol(se), what='grad emb')
    for k in sg:
        close(fg[k], sg[k], _grad_tol(sg[k]), what='grad pitch_encoder.' + k)
    # tracks that need a gradient keep the stock chain (the kernels give none), and still get it
    p = pitch.clone().requires_grad_(True)
    outs, _ = fused(emb, ln, p, energy)
    outs[-1][0].float().sum().backward()
    assert p.grad is not None and float(p.grad.abs().max()) > 0


def check_fused_path_ran(dev):
    """pitch_dim = energy_dim = 1, C = 64 on the device: with ``nn.Conv1d.forward`` patched to raise the forward still runs -- the
    four layers are on the kernels; with ``F.avg_pool1d`` patched to raise as well it runs at downsample_scales [1, 1], and at
    [1, 2] the only call left is the pooling of the embedding stream itself (one call, where the stock chain makes two)."""
    import torch.nn as nn
    emb, ln, pitch, energy = encoder_batch(dev)
    real_conv, real_pool = nn.Conv1d.forward, F.avg_pool1d
    calls = []

    def no_conv(self, x):
        raise AssertionError('nn.Conv1d.forward ran: the side encoder is on stock operators')

    def no_pool(*a, **k):
        raise AssertionError('F.avg_pool1d ran')

    def counted(*a, **k):
        calls.append(a[0].shape)
        return real_pool(*a, **k)
    try:
        nn.Conv1d.forward = no_conv
        F.avg_pool1d = no_pool
        m = build_encoder(dev, False, scales=(1, 1))
        outs, _ = m(emb, ln, pitch, energy)
        assert len(outs) == 2
        m.fused_side = False
        with pytest.raises(AssertionError, match='Conv1d.forward ran'):
            m(emb, ln, pitch, energy)
        F.avg_pool1d = counted
        m = build_encoder(dev, False, scales=(1, 2))
        outs, _ = m(emb, ln, pitch, energy)
        assert len(calls) == 1 and outs[1][0].shape[1] == 7
        nn.Conv1d.forward = real_conv
        del calls[:]
        m.fused_side = False
        m(emb, ln, pitch, energy)
        assert len(calls) == 2
    finally:
        nn.Conv1d.forward, F.avg_pool1d = real_conv, real_pool


# ---- EmbVC against the reference ---------------------------------------------------------------------------------------------------
def build_vc(dev):
    from msmctts_amd.networks import find_modules
    z, ze = load_npz('small_vc.npz'), load_npz('small_ecapa.npz')
    cfg = json.loads(bytes(z['cfg']).decode())
    (_, m), = find_modules({'autoencoder': dict(cfg, _name='EmbVC')})
    want_keys = [k[len('state.'):] for k in z if k.startswith('state.')]
    assert list(m.state_dict().keys()) == want_keys                          # the reference's keys in its order
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(int(n) for n in z['shape.' + k]), k

    def val(k):
        a = ze['enc.state.' + k[len('global_encoder.'):]] if k.startswith('global_encoder.') else z['state.' + k]
        return t(a.astype(np.float32) if a.dtype == np.float16 else a)
    m.load_state_dict({k: val(k) for k in want_keys}, strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.to(dev), z, cfg


def check_vc_golden(dev):
    """strict load of the reference's state_dict, training-mode forward over explicit windows (every dictionary entry 1e-3, the
    gradients of a scalar of them 1e-3 of the largest entry), the global encoder's buffers afterwards (1e-5), evaluation-mode
    window='full': the tolerances of ``_parity.check_emb_autoencoder``"""
    from msmctts_amd.networks import find_modules
    m, z, cfg = build_vc(dev)
    m.train()
    b = {k[len('batch.'):]: t(v).to(dev) for k, v in z.items() if k.startswith('batch.')}
    windows = [tuple(int(v) for v in row) for row in z['windows']]
    e, r = b['emb'].clone().requires_grad_(True), b['mel'].clone().requires_grad_(True)
    o = m(e, b['emb_length'], b['pitch'], b['energy'], mel=r, window=windows)
    assert sorted(o) == ['content_representations', 'decoder_outputs', 'encoder_lengths', 'encoder_outputs', 'mel_outputs']
    seen = 0
    for k, v in o.items():
        for name, got in ([('train.' + k, v)] if torch.is_tensor(v) else [('train.%s.%d' % (k, i), x) for i, x in enumerate(v)]):
            if 'lengths' in name:
                assert np.array_equal(got.cpu().numpy(), z[name]), name
            else:
                close(got, z[name], what=name)
            seen += 1
    assert seen == 7
    scalar = (o['decoder_outputs'].pow(2).mean() + o['mel_outputs'].mean() + o['content_representations'].mean()
              + sum(f.pow(2).mean() for f in o['encoder_outputs']))
    scalar.backward()
    close(scalar, z['train.scalar'], what='scalar')
    for name, got in (('grad_emb', e.grad), ('grad_mel', r.grad)):
        close(got, z['train.' + name], _grad_tol(torch.from_numpy(z['train.' + name])), what=name)
    for k, p in m.encoder.pitch_encoder.named_parameters():
        want = z['train.grad.encoder.pitch_encoder.' + k]
        close(p.grad, want, _grad_tol(torch.from_numpy(want)), what='grad pitch_encoder.' + k)
    sd = m.state_dict()
    for k in z:
        if k.startswith('after.'):
            close(sd[k[len('after.'):]], z[k], 1e-5 * max(1.0, float(np.abs(z[k]).max())), 1e-5, what=k)
    m.eval()
    with torch.no_grad():
        close(m(b['emb'], b['emb_length'], b['pitch'], b['energy'], ref=b['mel'])['decoder_outputs'], z['eval.full.decoder_outputs'],
              what="window='full'")
    with pytest.raises(ValueError, match='Wrong global encoder'):
        find_modules({'autoencoder': dict(cfg, _name='EmbVC', global_encoder_config={'_name': 'XVectorTDNN'})})
    with pytest.raises(NotImplementedError):                                   # MSMCVQGANEmb's size refusals
        find_modules({'autoencoder': dict(cfg, _name='EmbVC', n_model_size=32)})


def check_vc_unsupported(dev):
    m, z, _ = build_vc(dev)
    x, ln = torch.zeros(1, 4, 24, device=dev), torch.tensor([4], device=dev)
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(NotImplementedError, match=':568'):
            m.analysis(x, ln)
        with pytest.raises(NotImplementedError, match=':587'):
            m.synthesis([x], [ln])
        with pytest.raises(NotImplementedError, match=':628'):
            m.compute_embedding_loss([x], [ln], {})


def check_vc_infer(dev):
    """``NASynTTSEmb.infer_step`` over an EmbVC autoencoder: a waveform of T x hop samples per utterance, equal to the golden
    window='full' output"""
    from msmctts_amd.tasks import build_task
    from msmctts_amd.utils.config import Config
    m, z, cfg = build_vc(dev)
    task = build_task(Config({'id': 'small_vc', 'task': {'_name': 'NASynTTSEmb', 'autoencoder': dict(cfg, _name='EmbVC')},
                              'dataset': dict(samplerate=16000, feature=['emb', 'mel', 'wav'], frameshift=[40, 40, 1])}), mode='infer')
    assert type(task.autoencoder).__name__ == 'EmbVC'
    task.autoencoder = m
    task = task.to(dev).eval()
    b = {k[len('batch.'):]: t(v).to(dev) for k, v in z.items() if k.startswith('batch.')}
    with torch.no_grad():
        res = task.infer_step({'emb': b['emb'], 'emb_length': b['emb_length'], 'pitch': b['pitch'], 'energy': b['energy'],
                               'ref': b['mel']})
    assert tuple(res['wav'].shape) == (3, 24 * 40)
    close(res['wav'], z['eval.full.decoder_outputs'][..., 0], what='infer_step wav')


# ---- trainer ----------------------------------------------------------------------------------------------------------------------
def check_trainer(dev, model):
    """one ``EmbVQGANTrainer`` step per phase over ``model`` ('EmbVC' or 'MSMCVQGANEmb' with pitch_dim = energy_dim = 1) on
    ``make_emb_batch(tracks=True)``: finite losses, VQ keys only where there is a quantiser, every ``pitch_encoder`` parameter moves"""
    import _embcases as E
    from msmctts_amd.synthetic import make_emb_batch
    from msmctts_amd.tasks import build_task
    cfg = E.config(False)
    ae = cfg.task.autoencoder
    ae['pitch_dim'], ae['energy_dim'] = 1, 1
    if model == 'EmbVC':
        ae['_name'] = 'EmbVC'
        del ae['quantizer_config']
        ae['encoder_config']['downsample_scales'] = [1, 1]
    torch.manual_seed(31)
    task = build_task(cfg, mode='train')
    assert type(task.autoencoder).__name__ == model
    task = task.to(dev).train()
    tr = E._trainer(cfg, task, seed=7)
    batch = make_emb_batch(3, E.T, E.EMB_DIM, E.MEL_DIM, E.HOP, seed=5, device=dev, tracks=True)
    assert tuple(batch['pitch'].shape) == (3, E.T, 1) and batch['pitch'].dtype == torch.float32
    enc = task.autoencoder.encoder
    for phase in (0, 1, 2):
        iteration = E.PHASE_ITERATION[phase]
        assert tr._phase(iteration) == phase
        before = {k: p.detach().clone() for k, p in enc.pitch_encoder.named_parameters()}
        log = tr.train_step(batch, iteration)
        losses = {k: float(v) for k, v in log['loss'].items()}
        assert losses and all(np.isfinite(v) for v in losses.values()), losses
        has_vq = any(k == 'vq_loss' or k.startswith('latent_loss') for k in losses)
        assert has_vq == (model != 'EmbVC'), sorted(losses)
        assert (phase == 0) == (tr.last_windows is None)
        for k, p in enc.pitch_encoder.named_parameters():
            assert not torch.equal(p.detach(), before[k]), 'phase %d: pitch_encoder.%s did not move' % (phase, k)


def check_batch_tracks():
    from msmctts_amd.synthetic import make_emb_batch
    plain = make_emb_batch(3, 20, 16, 8, 10, seed=3)
    default = make_emb_batch(3, 20, 16, 8, 10, seed=3, tracks=False)
    tracks = make_emb_batch(3, 20, 16, 8, 10, seed=3, tracks=True)
    assert list(plain) == list(default) == ['emb', 'emb_length', 'mel', 'wav', 'wav_length', 'emb_length_host']
    assert set(tracks) == set(plain) | {'pitch', 'energy'}
    for k, v in plain.items():
        for other in (default, tracks):
            assert torch.equal(v, other[k]) if torch.is_tensor(v) else v == other[k], k
    valid = torch.arange(20)[None, :, None] < tracks['emb_length'][:, None, None]
    for k in ('pitch', 'energy'):
        v = tracks[k]
        assert tuple(v.shape) == (3, 20, 1) and v.dtype == torch.float32
        assert bool((v[~valid] == 0).all()) and bool((v[valid] != 0).all())


def check_feature_present():
    lib = L()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'msmc_hip.h')) as f:
        header = f.read()
    for name in ('msmc_side_front_fwd', 'msmc_side_front_bwd', 'msmc_side_front_bwd_workspace', 'msmc_pool_add_fwd', 'msmc_pool_add_bwd'):
        assert name + '(' in header, name
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
    assert os.path.isfile(os.path.join(root, 'msmc-tts_amd', 'csrc', 'side_enc.hip'))
    import inspect
    from msmctts_amd.hip.side_enc import pool_add, side_front  # noqa: F401
    from msmctts_amd.networks.vqgantts import EmbVC
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import MAMSEncoder
    from msmctts_amd.synthetic import make_emb_batch
    from msmctts_amd.utils.utils import module_search
    assert MAMSEncoder.fused_side is True
    assert inspect.signature(make_emb_batch).parameters['tracks'].default is False
    import msmctts_amd.networks as nets
    assert module_search(['EmbVC'], os.path.dirname(nets.__file__), nets.__name__)[0] is EmbVC
