#!/usr/bin/env python
"""Runs ON the GPU box (under ``timeout``; one pass).

``bench_attention.py`` (or ``... fp32``): forward + backward of the fp32 attention core at the CSMSC shapes --
the gfx950 kernels (hip/attn.py, msmc_attn_fwd_f32 / msmc_attn_bwd_f32) next to the stock operator the fp32 stacks used before
(``F.scaled_dot_product_attention`` on strided views of the fused projection with the additive key bias, as
networks/acoustic_models/transformer.py calls it with MSMC_ATTN_FP32=0).

Per shape: the two are warmed up, then alternated for ROUNDS rounds of CALLS calls each between one pair of device events; the
table gives the median and the spread (min .. max) of the per-round us per call, and the ratio of the medians.  A HIP error
raises (non-zero exit).  The results of the two paths are compared before anything is timed.

``bench_attention.py bf16``: the bf16 kernels against the same operator (forward, and forward + backward, with dropout).
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa
import torch
import torch.nn.functional as F
from msmctts_amd.hip import attn

dev = torch.device('cuda:0')
SHAPES = ((16, 400, 2, 'encoder / decoder stack'), (16, 100, 2, 'down-sampled stage'), (64, 400, 2, 'configuration 4'))
ROUNDS, CALLS, WARM = 5, 100, 20
SCALE = 0.125


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(3e7))
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def bf16():
    """the bf16 kernels (csrc/attn.hip) against the stock operator at the bench configuration's shapes, with dropout"""
    from msmctts_amd.hip import norm
    for B, T, H, pd in ((16, 400, 2, 0.1), (16, 100, 2, 0.1), (16, 400, 2, 0.0), (4, 2400, 2, 0.1)):
        torch.manual_seed(0)
        qkv = (torch.randn(B, T, H * 192, device=dev) * 0.5).bfloat16().requires_grad_(True)
        pos = torch.arange(1, T + 1, device=dev).repeat(B, 1)
        pos[1:, T - T // 5:] = 0
        bias = attn.pad_key_bias(pos)
        add = torch.zeros(B, 1, 1, T, dtype=torch.bfloat16, device=dev).masked_fill_(pos.eq(0).view(B, 1, 1, T), float('-inf'))
        go = torch.randn(B, T, H * 64, device=dev).bfloat16()
        salt = norm.new_salt()

        def ours_f():
            return attn.attention(qkv, bias, H, 0.125, pd, salt)

        def ours_fb():
            qkv.grad = None
            ours_f().backward(go)

        def sdpa_f():
            x = qkv.view(B, T, H, 192).transpose(1, 2)
            o = F.scaled_dot_product_attention(x[..., :64], x[..., 64:128], x[..., 128:], attn_mask=add, dropout_p=pd, scale=0.125)
            return o.transpose(1, 2).reshape(B, T, H * 64)

        def sdpa_fb():
            qkv.grad = None
            sdpa_f().backward(go)

        with torch.no_grad():
            a, b = timed(ours_f), timed(sdpa_f)
        c, d = timed(ours_fb), timed(sdpa_fb)
        print('B %2d T %4d H %d p %.1f | forward: kernel %6.1f us, sdpa %6.1f us | forward+backward: kernel %6.1f us, sdpa %6.1f us'
              % (B, T, H, pd, a, b, c, d), flush=True)


def one_shape(B, T, H):
    gen = torch.Generator().manual_seed(B * 1000 + T)
    qkv = torch.randn(B, T, H * 192, generator=gen).to(dev).requires_grad_(True)
    go = torch.randn(B, T, H * 64, generator=gen).to(dev)
    lengths = torch.linspace(T, T // 2, B).long()
    pos = (torch.arange(1, T + 1)[None, :] * (torch.arange(T)[None, :] < lengths[:, None])).to(dev)
    bias = attn.pad_key_bias(pos)
    key_keep = torch.zeros(B, 1, 1, T, device=dev).masked_fill_(pos.eq(0).view(B, 1, 1, T), float('-inf'))

    def ours():
        qkv.grad = None
        out = attn.attention(qkv, bias, H, SCALE)
        out.backward(go)
        return out

    def stock():
        qkv.grad = None
        x = qkv.view(B, T, H, 192).transpose(1, 2)
        out = F.scaled_dot_product_attention(x[..., :64], x[..., 64:128], x[..., 128:], attn_mask=key_keep, scale=SCALE)
        out = out.transpose(1, 2).reshape(B, T, H * 64)
        out.backward(go)
        return out

    a, ga = ours().detach().clone(), qkv.grad.clone()
    b, gb = stock().detach().clone(), qkv.grad.clone()
    torch.cuda.synchronize()
    for name, u, v in (('out', a, b), ('dqkv', ga, gb)):
        err = float((u - v).abs().max()) / float(v.abs().max())
        assert err < 1e-3, '%s: kernels and stock operator differ by %.3e of the scale' % (name, err)
    per = {'kernels': [], 'stock': []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for fn in (ours, stock):
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in (('kernels', ours), ('stock', stock)):
            for _ in range(5):
                fn()
            ev[0].record()
            for _ in range(CALLS):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            per[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / CALLS)
    return per


def fp32():
    print('fp32 attention core, forward + backward, us per call: median (min .. max) over %d rounds of %d calls, alternated'
          % (ROUNDS, CALLS))
    print('| B | T | H | gfx950 kernels (3 launches) | stock scaled_dot_product_attention | stock / kernels |')
    print('|---|---|---|---|---|---|')
    for B, T, H, _ in SHAPES:
        per = one_shape(B, T, H)
        k, s = per['kernels'], per['stock']
        print('| %d | %d | %d | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f |' % (
            B, T, H, statistics.median(k), min(k), max(k), statistics.median(s), min(s), max(s),
            statistics.median(s) / statistics.median(k)), flush=True)


if __name__ == '__main__':
    torch.cuda.set_device(0)
    {'fp32': fp32, 'bf16': bf16}[sys.argv[1] if len(sys.argv) > 1 else 'fp32']()
