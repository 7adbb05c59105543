"""Shared cases of the fp32 attention core (csrc/attn.hip attn_*_f32_kernel, msmc_attn_fwd_f32 / msmc_attn_bwd_f32):
tests/test_attn_fp32_emu.py runs them on the kernel interpreter, tests/test_gpu_attn_fp32.py on the GPU.

Reference of every comparison: the chain

    S = scale Q K^T + bias,  P = softmax(S),  O = (P * mask / (1 - p)) V

written with einsum as tests/_parity.py check_attention does, and its autograd gradients dq | dk | dv for a random output
gradient, evaluated in float64 from the same fp32 input bits.

Bound.  err(x) = max |x - x64| / max |x64| over the whole tensor.  For out, dq, dk, dv of every case the kernel's err may be at
most RATIO = 4 x the err of the SAME chain evaluated by torch in fp32 on the CPU -- the factor is for another order of the sums
(32-key tiles, the online rescale, the merge of four partial softmaxes) -- and in any case below the project's fp32 bar of 1e-3.
Where the float64 tensor is identically zero (dq and dk of a single frame: the softmax over one key is constant) there is no
magnitude to divide by and torch's own chain returns exact zeros (g - g * 1); the kernels' value there is the residue
scale k (dP - D) of two fp32 evaluations of the SAME dot product dO . V in different orders, each within
gamma_64 sum |dO_c V_c| of it (gamma_n = n u / (1 - n u), u = 2^-24), hence |dq_c| <= 2 gamma_64 scale max|k| max_q sum_c |dO_c V_c|
(for dk with max|q|): that is the bound used for such a tensor.  Every comparison is appended to MEASURED and printed; the
ratios are recorded in profiles/attention_fp32.md.
"""
import torch

SCALE = 0.125
RATIO = 4.0
FP32_BAR = 1e-3
E_SHAPE = -2
MEASURED = []          # (case, quantity, kernel err, torch fp32 err)

# tag, B, T, H, gain on the q and k channels, valid keys per utterance
VALUE_CASES = (
    ('1x1x1', 1, 1, 1, 1.0, (1,)),                       # a single frame: dq and dk identically zero
    ('2x32x4', 2, 32, 4, 1.0, (32, 19)),                 # exactly one key tile, four heads
    ('2x33x1 one-key', 2, 33, 1, 1.0, (33, 1)),          # one tile plus one key; an utterance with ONE valid key
    ('3x45x2', 3, 45, 2, 1.0, (45, 32, 45)),             # ragged, second row 13 frames short
    ('2x129x2 flat', 2, 129, 2, 0.7, (129, 1)),          # wave 0 streams two tiles, the second with one row; one-key utterance
    ('2x129x2 peaked', 2, 129, 2, 2.0, (129, 1)),
    ('2x161x2 flat', 2, 161, 2, 0.7, (161, 130)),        # second tile for waves 0 and 1, ragged last tile, tile 4 partly masked
    ('2x161x2 peaked', 2, 161, 2, 2.0, (161, 130)),      # the running maximum moves from tile to tile
)
DROPOUT_CASES = (                                        # tag, B, T, H, gain, valid keys, p_drop
    ('2x50x2 drop', 2, 50, 2, 0.7, (50, 37), 0.25),
    ('2x161x2 drop', 2, 161, 2, 2.0, (161, 130), 0.25),
)
STACK_CFG = dict(max_seq_len=200, n_layers=2, n_head=2, d_k=64, d_v=64, d_model=128, d_inner=256, fft_conv1d_kernel=3,
                 fft_conv1d_padding=1, dropout=0.1, attn_dropout=0.1)
STACK_LENGTHS = {45: (45, 32), 161: (161, 130)}


def inputs(B, T, H, gain, lens, seed):
    """fp32 projection [B, T, H*192], fp32 output gradient [B, T, H*64], positions [B, T] (0 = padding); drawn on the CPU so that
    the interpreter and the GPU see the same values"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, H, 192, generator=gen)
    x[..., :128] *= gain
    go = torch.randn(B, T, H * 64, generator=gen)
    pos = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        pos[b, :n] = torch.arange(1, n + 1)
    return x.reshape(B, T, H * 192), go, pos


def run(dev, qkv, go, pos, H, p_drop=0.0, salt=0):
    """forward and backward on the kernels -> out [B, T, H*64], qkv.grad [B, T, H*192] (on the CPU, in the dtype of qkv)"""
    from msmctts_amd.hip import attn
    x = qkv.detach().clone().to(dev).requires_grad_(True)
    out = attn.attention(x, attn.pad_key_bias(pos.to(dev)), H, SCALE, p_drop, salt)
    assert out.dtype == qkv.dtype
    out.backward(go.to(dev))
    assert x.grad.dtype == qkv.dtype
    return out.detach().cpu(), x.grad.cpu()


def chain(qkv, go, pos, H, mask, p_drop, dtype):
    """the reference chain and its autograd gradients in ``dtype`` on the CPU: out [B, T, H, 64], dq, dk, dv likewise"""
    B, T, _ = qkv.shape
    x = qkv.to(dtype).reshape(B, T, H, 192).requires_grad_(True)
    bias = torch.zeros(B, T, dtype=dtype).masked_fill_(pos.eq(0), float('-inf'))
    s = torch.einsum('bqhd,bkhd->bhqk', x[..., :64], x[..., 64:128]) * SCALE + bias[:, None, None, :]
    o = torch.einsum('bhqk,bkhd->bqhd', torch.softmax(s, -1) * mask.to(dtype) / (1 - p_drop), x[..., 128:])
    o.backward(go.to(dtype).reshape(B, T, H, 64))
    g = x.grad
    return {'out': o.detach(), 'dq': g[..., :64], 'dk': g[..., 64:128], 'dv': g[..., 128:]}


def heads(out, grad, H):
    B, T, _ = out.shape
    g = grad.reshape(B, T, H, 192)
    return {'out': out.reshape(B, T, H, 64), 'dq': g[..., :64], 'dk': g[..., 64:128], 'dv': g[..., 128:]}


def zero_tensor_bound(name, qkv, go, H):
    """see the module docstring: bound of a gradient whose float64 value is identically zero"""
    B, T, _ = qkv.shape
    x = qkv.double().reshape(B, T, H, 192)
    other = x[..., 64:128] if name == 'dq' else x[..., :64]
    dots = (go.double().reshape(B, T, H, 64).abs().unsqueeze(2) * x[..., 128:].abs().unsqueeze(1)).sum(-1)     # [B, q, k, H]
    u = 2.0 ** -24
    return 2 * (64 * u / (1 - 64 * u)) * SCALE * float(other.abs().max()) * float(dots.max())


def compare(tag, got, t32, ref, qkv, go, H):
    failed = []
    for name in ('out', 'dq', 'dk', 'dv'):
        r = ref[name]
        mag = float(r.abs().max())
        ek, et = float((got[name].double() - r).abs().max()), float((t32[name].double() - r).abs().max())
        if mag == 0.0:
            bound = zero_tensor_bound(name, qkv, go, H)
            MEASURED.append((tag, name, ek, None))
            print('attention fp32 %-16s %-3s exactly zero in float64: kernel %.3e  bound %.3e' % (tag, name, ek, bound))
            if not ek <= bound:
                failed.append('%s: %.3e > %.3e' % (name, ek, bound))
            continue
        ek, et = ek / mag, et / mag
        MEASURED.append((tag, name, ek, et))
        print('attention fp32 %-16s %-3s err kernel %.3e  torch fp32 %.3e  ratio %s' % (tag, name, ek, et,
                                                                                      '%.2f' % (ek / et) if et else 'inf'))
        if not (ek <= RATIO * et and ek < FP32_BAR):
            failed.append('%s: kernel %.3e > %.0f x torch fp32 %.3e (or the 1e-3 bar)' % (name, ek, RATIO, et))
    assert not failed, (tag, failed)


# ---- 1, 2: values and gradients; the one-key utterance ---------------------------------------------------------------------------
def check_values(dev, n):
    tag, B, T, H, gain, lens = VALUE_CASES[n]
    qkv, go, pos = inputs(B, T, H, gain, lens, seed=400 + n)
    mask = torch.ones(B, H, T, T)
    ref, t32 = chain(qkv, go, pos, H, mask, 0.0, torch.float64), chain(qkv, go, pos, H, mask, 0.0, torch.float32)
    out, grad = run(dev, qkv, go, pos, H)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all()), tag
    compare(tag, heads(out, grad, H), t32, ref, qkv, go, H)
    for b, n_valid in enumerate(lens):
        if n_valid == 1 and T > 1:          # every query of the one-key utterance returns that key's value row
            v = qkv[b, 0].reshape(H, 192)[:, 128:]
            o = out[b].reshape(T, H, 64)
            assert bool(((o - v).abs() <= 2.0 ** -23 * v.abs()).all()), (tag, 'single key', float((o - v).abs().max()))


# ---- 3: dropout --------------------------------------------------------------------------------------------------------------------
def keep_mask(dev, B, T, H, p_drop, salt, dtype):
    """the kernels' own keep mask [B, H, T, T] for (seed word, salt): ceil(T / 64) probe calls with scale 0 (uniform scores) and
    one-hot values on keys 64 c .. 64 c + 63 -- output channel j of call c is keep(q, 64 c + j) / (T (1 - p))"""
    from msmctts_amd.hip import attn
    flat = attn.pad_key_bias(torch.ones(B, T, dtype=torch.long, device=dev))
    mask = torch.zeros(B, H, T, T)
    for c in range((T + 63) // 64):
        n = min(64, T - 64 * c)
        probe = torch.zeros(B, T, H, 192)
        for j in range(n):
            probe[:, 64 * c + j, :, 128 + j] = 1.0
        o = attn.attention(probe.reshape(B, T, H * 192).to(dtype).to(dev), flat, H, 0.0, p_drop, salt)
        mask[..., 64 * c:64 * c + n] = (o.float().cpu().reshape(B, T, H, 64)[..., :n].permute(0, 2, 1, 3) > 0).float()
    return mask


def check_dropout(dev, n):
    from msmctts_amd.hip import norm
    tag, B, T, H, gain, lens, pd = DROPOUT_CASES[n]
    qkv, go, pos = inputs(B, T, H, gain, lens, seed=500 + n)
    salt = norm.new_salt()
    mask = keep_mask(dev, B, T, H, pd, salt, torch.float32)
    rate = float(mask.mean())
    print('attention fp32 %-16s keep rate %.4f' % (tag, rate))
    assert abs(rate - (1 - pd)) < 0.03, (tag, rate)
    assert torch.equal(mask, keep_mask(dev, B, T, H, pd, salt, torch.bfloat16)), '%s: fp32 and bf16 kernels drop different entries' % tag
    assert not torch.equal(mask, keep_mask(dev, B, T, H, pd, norm.new_salt(), torch.float32)), tag
    ref, t32 = chain(qkv, go, pos, H, mask, pd, torch.float64), chain(qkv, go, pos, H, mask, pd, torch.float32)
    out, grad = run(dev, qkv, go, pos, H, pd, salt)
    compare(tag, heads(out, grad, H), t32, ref, qkv, go, H)          # holds only if both backward kernels used exactly that mask


# ---- 4: exact properties ----------------------------------------------------------------------------------------------------------
def check_exact_properties(dev):
    """no dropout, bit for bit: an utterance alone (T = 140) and followed by 160 padded frames (random q | k | v behind it, zero
    output gradient as the masked model output has) gives the same output and gradient rows; a batch row alone and among others
    likewise; two identical calls give identical results"""
    H = 2
    qkv, go, pos = inputs(1, 300, H, 2.0, (140,), seed=600)
    go[:, 140:] = 0.0
    long_out, long_grad = run(dev, qkv, go, pos, H)
    short_out, short_grad = run(dev, qkv[:, :140].contiguous(), go[:, :140].contiguous(), pos[:, :140].contiguous(), H)
    assert bool(qkv[:, 140:].abs().max() > 1)
    assert torch.equal(long_out[:, :140], short_out), 'padded frames changed the output'
    assert torch.equal(long_grad[:, :140], short_grad), 'padded frames changed the gradient'
    qkv, go, pos = inputs(3, 161, H, 2.0, (161, 130, 40), seed=601)
    out, grad = run(dev, qkv, go, pos, H)
    again = run(dev, qkv, go, pos, H)
    assert torch.equal(out, again[0]) and torch.equal(grad, again[1]), 'a repeated call changed bits'
    for b in range(3):
        o1, g1 = run(dev, qkv[b:b + 1], go[b:b + 1], pos[b:b + 1], H)
        assert torch.equal(out[b:b + 1], o1), ('out', b)
        assert torch.equal(grad[b:b + 1], g1), ('qkv.grad', b)


# ---- 5: rejected arguments; the wrapper's gradient casts -----------------------------------------------------------------------------
class _raises(object):
    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc) and self.text in str(val), (tp, val)
        return True


def check_rejected_arguments(dev):
    from msmctts_amd.hip import attn, lib
    B, T, H = 2, 45, 2
    qkv, go, pos = inputs(B, T, H, 1.0, (45, 32), seed=700)
    bias = attn.pad_key_bias(pos.to(dev))
    x, g, dx = qkv.to(dev), go.to(dev), torch.empty_like(qkv, device=dev)
    out, lse, dsum = torch.empty(B, T, H * 64, device=dev), torch.empty(B * H, T, device=dev), torch.empty(B * H, T, device=dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    L = lib.get()
    for bad_bias, pd in ((bias[:, :T].contiguous(), 0.0),                                   # Tp % 32 != 0
                         (bias, 1.0),                                                       # nothing would be kept
                         (bias[:, :32].contiguous(), 0.0)):                                 # Tp < T
        Tp = bad_bias.shape[1]
        rc = L.msmc_attn_fwd_f32(lib.ptr(x), lib.ptr(bad_bias), lib.ptr(out), lib.ptr(lse), B, T, H, Tp, SCALE, pd, lib.ptr(seed), 1,
                                 lib.stream(x))
        assert rc == E_SHAPE, rc
        rc = L.msmc_attn_bwd_f32(lib.ptr(x), lib.ptr(bad_bias), lib.ptr(out), lib.ptr(lse), lib.ptr(g), lib.ptr(dx), lib.ptr(dsum), B,
                                 T, H, Tp, SCALE, pd, lib.ptr(seed), 1, lib.stream(x))
        assert rc == E_SHAPE, rc
        with _raises(RuntimeError, 'msmc_attn_fwd_f32 failed with code -2'):
            attn.attention(x, bad_bias, H, SCALE, pd, 1)
    o = attn.attention(x.clone().requires_grad_(True), bias, H, SCALE)                     # ... and raised by the backward wrapper too
    o.grad_fn.args = (H, SCALE, 1.0, 1)
    with _raises(RuntimeError, 'msmc_attn_bwd_f32 failed with code -2'):
        o.grad_fn.apply(g)


def check_gradient_casts(dev):
    """an fp32 call keeps an fp32 gradient, widens a bf16 one and takes a non-contiguous one"""
    from msmctts_amd.hip import attn
    B, T, H = 2, 45, 2
    qkv, go, pos = inputs(B, T, H, 1.0, (45, 32), seed=701)
    go = go.bfloat16().float()                          # (representable in bf16: the widened gradient is the same gradient)
    bias = attn.pad_key_bias(pos.to(dev))
    _, want = run(dev, qkv, go, pos, H)
    strided = go.transpose(1, 2).contiguous().transpose(1, 2)
    assert not strided.is_contiguous()
    for g in (go.bfloat16(), strided, strided.bfloat16()):
        x = qkv.clone().to(dev).requires_grad_(True)
        out = attn.attention(x, bias, H, SCALE)
        direct = out.grad_fn.apply(g.to(dev))[0]
        assert direct.dtype == torch.float32 and torch.equal(direct.cpu(), want), (g.dtype, g.is_contiguous())


# ---- 6: the block stack against the oracle ---------------------------------------------------------------------------------------
def check_block_stack(dev, T, prologue, kernels):
    """FFTBlocks (2 blocks, 2 heads of 64, d_model 128, FFN 256) in fp32, eval mode, ragged lengths, against oracle/model.py's
    restatement of the stack on the same weights: output, input gradient and every parameter gradient within 1e-3 of the tensor's
    largest magnitude.  ``kernels``: the attention core must have run on the kernels once per block; otherwise (the
    MSMC_ATTN_FP32=0 switch, set on the module attribute) the same comparison through the stock operator, which the kernels
    never see."""
    from msmctts_amd.hip import attn as hipattn
    from msmctts_amd.networks.acoustic_models import transformer as tfm
    from oracle import model as omodel
    torch.manual_seed(11)
    net = tfm.FFTBlocks(name='enc', **STACK_CFG).to(dev)
    net.hip_dtype = torch.float32
    net.eval()
    B = 2
    lengths = torch.tensor(STACK_LENGTHS[T])
    pos = omodel.position_ids(lengths, T)
    gen = torch.Generator().manual_seed(12 + T)
    x_cpu = torch.randn(B, T, 128, generator=gen) * pos.ne(0).unsqueeze(-1)
    go = torch.randn(B, T, 128, generator=gen)
    calls = []
    real, keep_flag, keep_fp32 = hipattn.attention, tfm.FFT_PROLOGUE, hipattn.ATTN_FP32
    try:
        hipattn.attention = lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1]
        tfm.FFT_PROLOGUE = prologue
        hipattn.ATTN_FP32 = kernels
        x = x_cpu.clone().to(dev).requires_grad_(True)
        out, _ = net(x, None if prologue else pos.to(dev), lengths=lengths.to(dev) if prologue else None)
        (out * go.to(dev)).sum().backward()
    finally:
        hipattn.attention, tfm.FFT_PROLOGUE, hipattn.ATTN_FP32 = real, keep_flag, keep_fp32
    if kernels:
        assert calls == [torch.float32] * STACK_CFG['n_layers'], 'the attention core did not run on the fp32 kernels: %s' % calls
    else:
        assert not calls, 'MSMC_ATTN_FP32=0 must keep the stock operator'
    P = {'enc.' + k: v.detach().float().cpu().clone().requires_grad_(v.requires_grad) for k, v in net.named_parameters()}
    P.update({'enc.' + k: v.detach().cpu() for k, v in net.state_dict().items() if 'enc.' + k not in P})
    xo = x_cpu.clone().requires_grad_(True)
    want = omodel.fft_blocks(P, 'enc', xo, pos, STACK_CFG, training=False)
    (want * go).sum().backward()
    pairs = [('out', out.detach(), want.detach()), ('grad x', x.grad, xo.grad)]
    pairs += [(k, v.grad, P['enc.' + k].grad) for k, v in net.named_parameters() if v.requires_grad]
    assert len(pairs) > 2 + 10 * STACK_CFG['n_layers']
    failed = []
    for name, a, b in pairs:
        assert a is not None and b is not None, name
        err, mag = float((a.cpu().double() - b.double()).abs().max()), float(b.abs().max())
        if not err <= FP32_BAR * mag:
            failed.append('%s: max abs err %.3e, scale %.3e' % (name, err, mag))
    worst = max(float((a.cpu().double() - b.double()).abs().max()) / float(b.abs().max()) for _, a, b in pairs)
    print('attention fp32 stack T=%d prologue=%s kernels=%s: worst err / scale %.3e over %d tensors' % (T, prologue, kernels, worst,
                                                                                                       len(pairs)))
    assert not failed, failed


# ---- 7: what the parent commit lacks -----------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import attn, lib
    assert attn.supported(torch.float32, 64, 64) and attn.supported(torch.bfloat16, 64, 64)
    assert not attn.supported(torch.float32, 32, 32) and not attn.supported(torch.float16, 64, 64)
    assert {'msmc_attn_fwd_f32', 'msmc_attn_bwd_f32'} <= set(lib.exported_symbols())
    keep = attn.ATTN_FP32
    try:
        attn.ATTN_FP32 = False
        assert not attn.supported(torch.float32, 64, 64) and attn.supported(torch.bfloat16, 64, 64)
    finally:
        attn.ATTN_FP32 = keep
