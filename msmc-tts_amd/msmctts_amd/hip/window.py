"""Fixed-length windows of a subset of utterances on the gfx950 kernels (csrc/window.hip): autograd function.

``window_gather(x, win, W, out_dtype)``: x [B, T, C] fp32 or bf16, ``win`` the (utterance, first row) pairs of n <= B windows
-> [n, W, C] in ``out_dtype`` (default: x's), ``out[j, t] = x[u_j, s_j + t]`` rounded once (the bits of ``Tensor.to``), zeros for
rows outside [0, T).  [n, W, C] is the channels-last image the vocoder's first convolution reads, in its compute dtype: no
transpose / contiguous / cast chain behind it.  Backward, one launch writes every element of the gradient of x -- the
gradient row of the window covering it, zero elsewhere.

``win`` is an int32 [n, 2] tensor on x's device (its contents cannot be checked from the host; the kernels are safe for any,
and the contract is strictly increasing utterance indices) or a Python list of (u, s) pairs, which IS checked: ``ValueError``
unless the utterance indices are strictly increasing.  Shapes the kernels refuse (W < 1, n < 1, n > B ...) raise the
``RuntimeError`` of every failed launch."""
import torch

from . import lib

_DT = {torch.float32: 0, torch.bfloat16: 1}


def as_windows(win, device):
    """``win`` as the kernels' [n, 2] int32 table on ``device``; a Python list is validated on the way"""
    if torch.is_tensor(win):
        if win.dtype != torch.int32 or win.dim() != 2 or win.shape[1] != 2:
            raise TypeError('window table: int32 [n, 2], got %s %s' % (win.dtype, tuple(win.shape)))
        if win.device != torch.device(device):
            raise ValueError('window table on %s, tensor on %s' % (win.device, device))
        return win.contiguous()
    pairs = [(int(u), int(s)) for u, s in win]
    if any(b[0] <= a[0] for a, b in zip(pairs, pairs[1:])):
        raise ValueError('utterance indices of the windows must be strictly increasing, got %s' % [u for u, _ in pairs])
    return torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(device)


class _WindowGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, win, W, out_dtype):
        B, T, C = x.shape
        n = win.shape[0]
        out = torch.empty((n, max(W, 0), C), dtype=out_dtype, device=x.device)
        lib.call('msmc_window_gather_fwd', lib.ptr(x), _DT[x.dtype], lib.ptr(win), lib.ptr(out), _DT[out_dtype], B, T, C, n, W,
                 lib.stream(x))
        ctx.save_for_backward(win)
        ctx.args = (B, T, C, W, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        win, = ctx.saved_tensors
        B, T, C, W, dtype = ctx.args
        g = g.contiguous()
        if g.dtype not in _DT:
            g = g.float()
        gx = torch.empty((B, T, C), dtype=dtype, device=g.device)
        lib.call('msmc_window_gather_bwd', lib.ptr(g), _DT[g.dtype], lib.ptr(win), lib.ptr(gx), _DT[dtype], B, T, C, win.shape[0],
                 W, lib.stream(g))
        return gx, None, None, None


def usable(x):
    """the kernels take this tensor: fp32 / bf16 [B, T, C] on the GPU (or on the host with the interpreter build bound)"""
    return torch.is_tensor(x) and x.dim() == 3 and x.dtype in _DT and (x.is_cuda or lib._host_pointers_ok)


def window_gather(x, win, W, out_dtype=None):
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if x.dim() != 3 or x.dtype not in _DT or out_dtype not in _DT:
        raise TypeError('window_gather: fp32 / bf16 [B, T, C] in, fp32 / bf16 out; got %s %s -> %s' % (x.dtype, tuple(x.shape),
                                                                                                    out_dtype))
    return _WindowGather.apply(x.contiguous(), as_windows(win, x.device), int(W), out_dtype)
