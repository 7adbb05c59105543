"""The pitch / energy side encoder of ``MAMSEncoder`` on the gfx950 kernels (csrc/side_enc.hip): autograd functions.

``side_front(pitch, energy, weight, bias, out_dtype)``: the first layer of the side encoder with its Tanh.  pitch [B, T, P] and
energy [B, T, E] fp32 (either may be None where its width is 0) are read where they are -- no ``torch.cat``, no transposes;
``weight`` [C, P + E, taps] and ``bias`` [C] are ``nn.Conv1d``'s own parameters.  Returns y [B, T, C] channels-last, fp32 or bf16.
Differentiable in ``weight`` and ``bias`` only: the tracks are data (``front_usable`` is False when either requires a gradient,
and the caller keeps the stock chain).

``pool_add(side, feat, scale)``: ``(pooled, out)`` with ``pooled = avg_pool1d(side, scale, scale, ceil_mode=True)`` along the
frames of the channels-last side [B, Tin, C] fp32 and ``out = feat + pooled.to(feat.dtype)`` for feat [B, ceil(Tin / scale), C]
fp32 or bf16 -- one launch forward, one backward.  ``scale == 1``: ``pooled`` is ``side`` itself.

There is no CPU path and no fallback: without the library, or with host tensors on the product build, the calls raise; shapes
the launchers refuse raise with the launcher's code.  ``front_usable`` / ``pool_usable`` tell a caller beforehand."""
import torch

from . import lib

_DT = {torch.float32: 0, torch.bfloat16: 1}
MAX_CIN, MAX_TAPS, MAX_WEIGHT = 8, 15, 12288


def _on_kernels(t):
    return t.is_cuda or lib._host_pointers_ok


def front_usable(pitch, energy, weight):
    """the front kernel takes these operands: fp32 tracks [B, T, P] / [B, T, E] that need no gradient, on the GPU (or on the host
    with the interpreter build bound), and a weight [C, P + E, taps] inside its limits"""
    tracks = [t for t in (pitch, energy) if t is not None]
    if not tracks or weight.dim() != 3 or weight.dtype != torch.float32:
        return False
    if any(t.dim() != 3 or t.dtype != torch.float32 or t.requires_grad or t.shape[:2] != tracks[0].shape[:2] or
           t.device != weight.device for t in tracks):
        return False
    C, cin, taps = weight.shape
    return (_on_kernels(weight) and sum(t.shape[2] for t in tracks) == cin and 1 <= cin <= MAX_CIN and taps % 2 == 1 and
            taps <= MAX_TAPS and C % 8 == 0 and C * cin * taps + C <= MAX_WEIGHT and tracks[0].shape[0] >= 1 and tracks[0].shape[1] >= 1)


def pool_usable(side, feat, scale):
    return (side.dim() == 3 and feat.dim() == 3 and side.dtype == torch.float32 and feat.dtype in _DT and scale >= 1 and
            side.device == feat.device and _on_kernels(side) and
            tuple(feat.shape) == (side.shape[0], -(-side.shape[1] // scale), side.shape[2]) and side.numel() > 0)


class _SideFront(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pitch, energy, weight, bias, out_dtype):
        ref = pitch if pitch is not None else energy
        B, T = ref.shape[:2]
        P = 0 if pitch is None else pitch.shape[2]
        E = 0 if energy is None else energy.shape[2]
        C, _, taps = weight.shape
        y = torch.empty((B, T, C), dtype=out_dtype, device=ref.device)
        lib.call('msmc_side_front_fwd', lib.ptr(pitch, torch.float32), lib.ptr(energy, torch.float32), lib.ptr(weight), lib.ptr(bias),
                 lib.ptr(y), _DT[out_dtype], B, T, P, E, C, taps, lib.stream(y))
        ctx.save_for_backward(pitch, energy, y)
        ctx.args = (B, T, P, E, C, taps)
        return y

    @staticmethod
    def backward(ctx, gy):
        pitch, energy, y = ctx.saved_tensors
        B, T, P, E, C, taps = ctx.args
        gy = gy.contiguous()
        if gy.dtype != y.dtype:
            gy = gy.to(y.dtype)
        dw = torch.empty((C, P + E, taps), dtype=torch.float32, device=y.device)
        db = torch.empty((C,), dtype=torch.float32, device=y.device)
        ws = lib.workspace(int(lib.get().msmc_side_front_bwd_workspace(B, T, P, E, C, taps)), y.device, floor=4)
        lib.call('msmc_side_front_bwd', lib.ptr(pitch), lib.ptr(energy), lib.ptr(y), lib.ptr(gy), _DT[y.dtype], lib.ptr(dw), lib.ptr(db),
                 lib.ptr(ws), ws.numel() * ws.element_size(), B, T, P, E, C, taps, lib.stream(y))
        return None, None, dw, db, None


def side_front(pitch, energy, weight, bias, out_dtype=torch.float32):
    if out_dtype not in _DT:
        raise TypeError('side_front: fp32 or bf16 out, got %s' % out_dtype)
    pitch = None if pitch is None or pitch.shape[-1] == 0 else pitch.detach().contiguous()
    energy = None if energy is None or energy.shape[-1] == 0 else energy.detach().contiguous()
    if pitch is None and energy is None:
        raise ValueError('side_front: no input track')
    return _SideFront.apply(pitch, energy, weight.contiguous(), bias.contiguous(), out_dtype)


class _PoolAdd(torch.autograd.Function):
    """scale > 1: (pooled, out); scale == 1: out alone"""

    @staticmethod
    def forward(ctx, side, feat, scale):
        B, Tin, C = side.shape
        Tout = feat.shape[1]
        out = torch.empty_like(feat)
        pooled = torch.empty((B, Tout, C), dtype=torch.float32, device=side.device) if scale > 1 else None
        lib.call('msmc_pool_add_fwd', lib.ptr(side), lib.ptr(feat), _DT[feat.dtype], lib.ptr(pooled), lib.ptr(out), B, Tin, Tout, C, scale,
                 lib.stream(side))
        ctx.args = (B, Tin, Tout, C, scale)
        ctx.set_materialize_grads(False)
        return (pooled, out) if scale > 1 else out

    @staticmethod
    def backward(ctx, *grads):
        B, Tin, Tout, C, scale = ctx.args
        gpooled, gout = grads if scale > 1 else (None, grads[0])
        if gpooled is None and gout is None:
            return None, None, None
        gside = None
        if ctx.needs_input_grad[0]:
            if scale == 1 and gout.dtype == torch.float32:
                gside = gout
            else:
                go = None if gout is None else gout.contiguous()
                if go is not None and go.dtype not in _DT:
                    go = go.float()
                gp = None if gpooled is None else gpooled.contiguous().float()
                gside = torch.empty((B, Tin, C), dtype=torch.float32, device=(go if go is not None else gp).device)
                lib.call('msmc_pool_add_bwd', lib.ptr(go), 0 if go is None else _DT[go.dtype], lib.ptr(gp), lib.ptr(gside), B, Tin, Tout, C,
                         scale, lib.stream(gside))
        return gside, (gout if ctx.needs_input_grad[1] else None), None


def pool_add(side, feat, scale):
    scale = int(scale)
    if side.dtype != torch.float32 or feat.dtype not in _DT or side.dim() != 3 or feat.dim() != 3:
        raise TypeError('pool_add: fp32 [B, Tin, C] and fp32 / bf16 [B, Tout, C]; got %s %s, %s %s' % (
            side.dtype, tuple(side.shape), feat.dtype, tuple(feat.shape)))
    side, feat = side.contiguous(), feat.contiguous()
    if scale > 1:
        return _PoolAdd.apply(side, feat, scale)
    return side, _PoolAdd.apply(side, feat, scale)
