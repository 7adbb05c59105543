"""Stage targets of the multi-stage quantiser from stored code indices on the gfx950 kernel (csrc/code_embed.hip).

``code_gather(ind, length, embed_t, out_dtype)``: ind [B, T, H] int32 / int64, length [B], embed_t [H, K, d] fp32 (what
``vq_prepare`` returns: every codeword one contiguous row) -> [B, T, H * d] in ``out_dtype`` (fp32 or bf16, one rounding: the
bits of ``Tensor.to``) with ``out[b, t, h d + c] = embed_t[h, ind[b, t, h], c]`` where ``t < length[b]``; a head whose label is
outside [0, K) gives zeros for its d channels, rows at or beyond ``length[b]`` are zeros.  One launch (``msmc_code_gather``), no
zero-fill.  Forward only: the codebook behind it is frozen, the result carries no gradient.

Operands the kernel cannot take -- host tensors without the interpreter build bound, another label or codebook dtype -- run the
stock chain ``code_gather_stock`` (``F.embedding`` per head, masks): the same values, bit for bit.  ``usable`` says which way a
call goes.  On the GPU a launch the kernel refuses raises the ``RuntimeError`` of every failed launch."""
import torch
import torch.nn.functional as F

from . import lib

_DT = {torch.float32: 0, torch.bfloat16: 1}
_IT = {torch.int32: 0, torch.int64: 1}


def usable(ind, embed_t, out_dtype=torch.float32):
    """the kernel takes these operands: int32 / int64 labels and an fp32 codebook on one GPU (or on the host with the interpreter
    build bound), fp32 / bf16 out"""
    return (torch.is_tensor(ind) and torch.is_tensor(embed_t) and ind.dtype in _IT and embed_t.dtype == torch.float32
            and embed_t.dim() == 3 and out_dtype in _DT and ind.device == embed_t.device
            and (ind.is_cuda or lib._host_pointers_ok))


def code_gather_stock(ind, length, embed_t, out_dtype=torch.float32):
    """``code_gather`` on stock operators: the definition, and the path of operands the kernel does not take"""
    H, K, d = embed_t.shape
    B, T = ind.shape[:2]
    ind = ind.long()
    ok = (ind >= 0) & (ind < K) & (torch.arange(T, device=ind.device)[None, :] < length.to(ind.device).reshape(B, 1))[..., None]
    rows = [F.embedding(ind[..., h].clamp(0, K - 1), embed_t[h]) for h in range(H)]
    out = torch.where(ok[..., None], torch.stack(rows, dim=2), torch.zeros((), dtype=embed_t.dtype, device=ind.device))
    return out.reshape(B, T, H * d).to(out_dtype)


def code_gather(ind, length, embed_t, out_dtype=torch.float32):
    if not torch.is_tensor(embed_t) or embed_t.dim() != 3:
        raise ValueError('embed_t: expected [H, K, d]')
    H, K, d = embed_t.shape
    if ind.dim() == 2 and H == 1:
        ind = ind.unsqueeze(-1)
    if ind.dim() != 3 or ind.shape[2] != H:
        raise ValueError('ind: expected [B, T, %d], got %s' % (H, tuple(ind.shape)))
    if ind.dtype.is_floating_point or ind.dtype == torch.bool:
        raise TypeError('ind: integer labels expected, got %s' % ind.dtype)
    if out_dtype not in _DT:
        raise TypeError('code_gather: fp32 / bf16 out, got %s' % (out_dtype,))
    B, T = ind.shape[:2]
    length = torch.as_tensor(length).reshape(-1)
    if length.numel() != B:
        raise ValueError('%d lengths for %d utterances' % (length.numel(), B))
    with torch.no_grad():
        if not usable(ind, embed_t, out_dtype):
            return code_gather_stock(ind, length, embed_t.detach().float(), out_dtype)
        indc = ind.detach().contiguous()
        lenc = length.to(device=indc.device, dtype=torch.int32).contiguous()
        embc = embed_t.detach().contiguous()
        out = torch.empty((B, T, H * d), dtype=out_dtype, device=indc.device)
        lib.call('msmc_code_gather', lib.ptr(indc), _IT[indc.dtype], lib.ptr(lenc, torch.int32), lib.ptr(embc, torch.float32),
                 lib.ptr(out), _DT[out_dtype], B, T, H, d, K, lib.stream(indc))
    return out
