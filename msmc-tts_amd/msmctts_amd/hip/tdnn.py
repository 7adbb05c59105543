"""Autograd functions over the speaker reference encoder's kernels (csrc/tdnn.hip, reference vqgantts/tdnn.py):

    relu_batch_norm(x, bn)                    bn(F.relu(x)) for an affine nn.BatchNorm1d on channels-last x [..., C]
    se_residual(x, res, linear1, linear2)     res + x * sigmoid(linear2(relu(linear1(mean_t(x)))))      x [B, T, C]
    attentive_stats_pool(x, a)                (sum_t alpha x | sqrt(clamp(sum_t alpha x^2 - mean^2, 1e-9))), alpha = softmax_t(a)

Activations fp32 or bf16; parameters, statistics and their gradients fp32.  The ``*_usable`` predicates say whether a call is
inside what the kernels take; the functions themselves never fall back -- a refused shape raises.
"""
import torch

from . import lib

_DT = {torch.float32: 0, torch.bfloat16: 1}


def _workspace(holder, name, nbytes, device):
    """scratch of a multi-launch pass, kept on the module that owns the operator: consumed before the call returns"""
    have = getattr(holder, name, None)
    ws = lib.workspace(nbytes, device, have if have is not None and have.device == device else None, floor=4)
    if ws is not have:
        setattr(holder, name, ws)
    return ws


def _device_ok(x):
    return x.dtype in _DT and (x.is_cuda or lib._host_pointers_ok)


def _rows(x):
    """(N, C, row stride) of a channels-last tensor whose rows are evenly spaced: contiguous, or a channel slice of such rows"""
    C = x.shape[-1]
    N = x.numel() // C
    if x.is_contiguous() or x.dim() < 2:
        return N, C, C
    ld = x.stride(-2)
    even = x.stride(-1) == 1 and all(x.stride(i) == x.stride(i + 1) * x.shape[i + 1] for i in range(x.dim() - 2))
    if not even or ld < C:
        raise ValueError('relu_batch_norm takes contiguous rows or a channel slice of contiguous rows, got strides %s' % (x.stride(),))
    return N, C, ld


def _raw(t):
    """pointer of a tensor that may be a channel slice (lib.ptr insists on contiguity)"""
    import ctypes
    if not t.is_cuda and not lib._host_pointers_ok:
        raise RuntimeError('msmc HIP ops run on the GPU only (got a %s tensor); there is no CPU path' % t.device)
    return ctypes.c_void_p(t.data_ptr())


# ---- ReLU + affine BatchNorm -------------------------------------------------------------------------------------------------
class _ReluBatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, bn):
        N, C, ldx = _rows(x)
        L = lib.get()
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        rstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ctx.training, ctx.bn = bn.training, bn
        if bn.training:
            if N < 2:
                raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(x.shape),))
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            ws = _workspace(bn, '_hip_ws', int(L.msmc_relu_bn_workspace(N, C)), x.device)
            lib.call('msmc_relu_bn_fwd', _raw(x), ldx, lib.ptr(gamma, torch.float32), lib.ptr(beta, torch.float32), lib.ptr(y), C,
                     lib.ptr(mean), lib.ptr(rstd), lib.ptr(bn.running_mean, torch.float32), lib.ptr(bn.running_var, torch.float32),
                     lib.ptr(bn.num_batches_tracked, torch.int64), lib.ptr(ws), ws.numel() * 4, N, C, float(bn.eps),
                     float(bn.momentum), _DT[x.dtype], lib.stream(x))
            ctx.save_for_backward(x, gamma, mean, rstd)
        else:
            lib.call('msmc_relu_bn_eval_fwd', _raw(x), ldx, lib.ptr(gamma, torch.float32), lib.ptr(beta, torch.float32),
                     lib.ptr(bn.running_mean, torch.float32), lib.ptr(bn.running_var, torch.float32), lib.ptr(y), C, lib.ptr(rstd),
                     N, C, float(bn.eps), _DT[x.dtype], lib.stream(x))
            # (the running mean as it was in the forward pass: a later training step may move the buffer)
            ctx.save_for_backward(x, gamma, bn.running_mean.clone() if any(ctx.needs_input_grad) else bn.running_mean, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, rstd = ctx.saved_tensors
        g = g.contiguous()
        if g.dtype != x.dtype:
            g = g.to(x.dtype)
        N, C, ldx = _rows(x)
        L = lib.get()
        gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = _workspace(ctx.bn, '_hip_ws', int(L.msmc_relu_bn_workspace(N, C)), x.device)
        lib.call('msmc_relu_bn_bwd' if ctx.training else 'msmc_relu_bn_eval_bwd', lib.ptr(g), C, _raw(x), ldx, lib.ptr(mean),
                 lib.ptr(rstd), lib.ptr(gamma), lib.ptr(gx), C, lib.ptr(dgamma), lib.ptr(dbeta), lib.ptr(ws), ws.numel() * 4, N, C,
                 _DT[x.dtype], lib.stream(x))
        return gx, dgamma, dbeta, None


def relu_batch_norm_usable(x, bn):
    """fp32 / bf16 rows (contiguous or a channel slice with a row stride % 8 == 0), C % 8 == 0 and <= 1024, and the module the
    reference builds: nn.BatchNorm1d defaults -- affine, a float momentum, fp32 parameters and running statistics on x's device"""
    C = x.shape[-1]
    if not (_device_ok(x) and C % 8 == 0 and 0 < C <= 1024 and C == bn.num_features):
        return False
    if not bn.affine or not bn.track_running_stats or not isinstance(bn.momentum, float):
        return False
    if x.stride(-1) != 1 or (x.dim() > 1 and x.stride(-2) % 8) or x.data_ptr() % 16:
        return False
    return all(t is not None and t.dtype == dt and t.device == x.device and t.is_contiguous() and t.data_ptr() % 16 == 0
               for t, dt in ((bn.weight, torch.float32), (bn.bias, torch.float32), (bn.running_mean, torch.float32),
                             (bn.running_var, torch.float32), (bn.num_batches_tracked, torch.int64)))


def relu_batch_norm(x, bn):
    """``bn(F.relu(x))`` for channels-last x [..., C] -- what the reference computes on [B, C, T]: batch statistics over every
    frame and the module's buffers advanced in training, the running statistics in evaluation.  x may be a channel slice
    ``wide[..., c0:c0 + C]`` of contiguous rows; y is contiguous."""
    if not relu_batch_norm_usable(x, bn):
        raise RuntimeError('relu_batch_norm: outside what msmc_relu_bn_* takes (C %% 8 == 0, C <= 1024, fp32 / bf16, an affine '
                           'BatchNorm1d with running statistics): x %s %s' % (tuple(x.shape), x.dtype))
    return _ReluBatchNorm.apply(x, bn.weight, bn.bias, bn)


# ---- squeeze-excitation + residual ------------------------------------------------------------------------------------------------
class _SEResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, W1, b1, W2, b2, holder):
        B, T, C = x.shape
        L = lib.get()
        y = torch.empty_like(x)
        gate = torch.empty(B, C, dtype=torch.float32, device=x.device)
        mean = torch.empty(B, C, dtype=torch.float32, device=x.device)
        hidden = torch.empty(B, C // 2, dtype=torch.float32, device=x.device)
        ws = _workspace(holder, '_hip_ws', int(L.msmc_se_workspace(B, T, C)), x.device)
        lib.call('msmc_se_fwd', lib.ptr(x), lib.ptr(res, x.dtype), lib.ptr(W1, torch.float32), lib.ptr(b1, torch.float32),
                 lib.ptr(W2, torch.float32), lib.ptr(b2, torch.float32), lib.ptr(y), lib.ptr(gate), lib.ptr(mean), lib.ptr(hidden),
                 lib.ptr(ws), ws.numel() * 4, B, T, C, _DT[x.dtype], lib.stream(x))
        ctx.save_for_backward(x, W1, W2, gate, mean, hidden)
        ctx.holder = holder
        return y

    @staticmethod
    def backward(ctx, g):
        x, W1, W2, gate, mean, hidden = ctx.saved_tensors
        B, T, C = x.shape
        g = g.contiguous()
        if g.dtype != x.dtype:
            g = g.to(x.dtype)
        L = lib.get()
        dgate = torch.empty_like(gate)
        ws = _workspace(ctx.holder, '_hip_ws', int(L.msmc_se_workspace(B, T, C)), x.device)
        lib.call('msmc_se_bwd_gate', lib.ptr(g), lib.ptr(x), lib.ptr(dgate), lib.ptr(ws), ws.numel() * 4, B, T, C, _DT[x.dtype],
                 lib.stream(x))
        # the two small layers, on [B, C] / [B, C/2] quantities (a few KB: stock matrix products)
        dz2 = dgate * gate * (1.0 - gate)
        dz1 = (dz2 @ W2) * (hidden > 0).to(dz2.dtype)
        dmean = ((dz1 @ W1) / T).contiguous()
        gx = torch.empty_like(x)
        lib.call('msmc_se_bwd_apply', lib.ptr(g), lib.ptr(gate), lib.ptr(dmean), lib.ptr(gx), B, T, C, _DT[x.dtype], lib.stream(x))
        return gx, g, dz1.t() @ mean, dz1.sum(0), dz2.t() @ hidden, dz2.sum(0), None


def se_residual_usable(x, linear1, linear2):
    """contiguous fp32 / bf16 x [B, T, C], C % 8 == 0 and <= 1024, the reference's SE_Connect layers (C -> C/2 -> C, fp32)"""
    if not (x.dim() == 3 and _device_ok(x) and x.is_contiguous() and x.data_ptr() % 16 == 0):
        return False
    B, T, C = x.shape
    if not (C % 8 == 0 and 0 < C <= 1024 and T >= 1 and 0 < B < 65536):
        return False
    return (tuple(linear1.weight.shape) == (C // 2, C) and tuple(linear2.weight.shape) == (C, C // 2) and
            all(p is not None and p.dtype == torch.float32 and p.device == x.device and p.is_contiguous()
                for p in (linear1.weight, linear1.bias, linear2.weight, linear2.bias)))


def se_residual(x, res, linear1, linear2, holder=None):
    """``res + x * sigmoid(linear2(relu(linear1(x.mean(1))))).unsqueeze(1)`` on channels-last x, res [B, T, C]"""
    if not se_residual_usable(x, linear1, linear2) or res.shape != x.shape:
        raise RuntimeError('se_residual: outside what msmc_se_* takes (contiguous [B, T, C], C %% 8 == 0, C <= 1024, fp32 / bf16): '
                           'x %s %s' % (tuple(x.shape), x.dtype))
    return _SEResidual.apply(x, res.contiguous(), linear1.weight, linear1.bias, linear2.weight, linear2.bias,
                             linear1 if holder is None else holder)


# ---- attentive statistics pooling -------------------------------------------------------------------------------------------------
class _AttentiveStatsPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, holder):
        B, T, C = x.shape
        L = lib.get()
        out = torch.empty(B, 2 * C, dtype=torch.float32, device=x.device)
        stats = torch.empty(B, 4, C, dtype=torch.float32, device=x.device)
        ws = _workspace(holder, '_hip_ws', int(L.msmc_asp_workspace(B, T, C)), x.device)
        lib.call('msmc_asp_fwd', lib.ptr(x), lib.ptr(a, x.dtype), lib.ptr(out), lib.ptr(stats), lib.ptr(ws), ws.numel() * 4, B, T, C,
                 _DT[x.dtype], lib.stream(x))
        ctx.save_for_backward(x, a, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        x, a, stats = ctx.saved_tensors
        B, T, C = x.shape
        g = g.contiguous().float()
        gx, ga = torch.empty_like(x), torch.empty_like(a)
        lib.call('msmc_asp_bwd', lib.ptr(g), lib.ptr(x), lib.ptr(a), lib.ptr(stats), lib.ptr(gx), lib.ptr(ga), B, T, C, _DT[x.dtype],
                 lib.stream(x))
        return gx, ga, None


class _Holder(object):
    """workspace owner for callers without a module"""


_DEFAULT_HOLDER = _Holder()


def attentive_stats_pool_usable(x, a):
    """contiguous x and logits a [B, T, C] of one fp32 / bf16 dtype, C % 8 == 0 and <= 1536"""
    if not (x.dim() == 3 and a.shape == x.shape and a.dtype == x.dtype and _device_ok(x) and x.is_contiguous() and a.is_contiguous()):
        return False
    B, T, C = x.shape
    return C % 8 == 0 and 0 < C <= 1536 and T >= 1 and 0 < B < 65536 and x.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0


def attentive_stats_pool(x, a, holder=None):
    """(mean | std) [B, 2C] in fp32 of x [B, T, C] under softmax_t(a): the softmax runs over all T frames, as in the reference"""
    if not attentive_stats_pool_usable(x, a):
        raise RuntimeError('attentive_stats_pool: outside what msmc_asp_* takes (contiguous [B, T, C], C %% 8 == 0, C <= 1536, '
                           'fp32 / bf16): x %s %s' % (tuple(x.shape), x.dtype))
    return _AttentiveStatsPool.apply(x, a, _DEFAULT_HOLDER if holder is None else holder)
