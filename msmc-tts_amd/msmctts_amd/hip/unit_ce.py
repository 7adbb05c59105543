"""The unit predictor's loss and label decoding on the gfx950 kernels (csrc/unit_ce.hip): text -> units is a classifier over the
K centroids of a k-means codebook, trained on stored labels with -1 padding.

``masked_cross_entropy`` is the reference's ``'softmax'`` embedding loss (msmc_vqgan.py:254-258: cross-entropy per frame, padded
frames masked, summed, divided by the sum of the lengths) in two forward launches and one backward launch: the forward reads
the logits once and keeps 4 bytes per frame (the log-sum-exp), where the stock chain stores [N, K] fp32 log-probabilities and
their gradient.  ``unit_argmax`` turns logits into labels with -1 padding, the form ``collapse_units`` and
``KMeansVQGANEmb.synthesis_units`` take.

There is no CPU path and no fallback: without the library, or with host tensors on the product build, the calls raise; shapes
the launchers refuse raise with the launcher's code.
"""
import torch

from . import lib

_DT = {torch.float32: 0, torch.bfloat16: 1}


def _operands(logits, lengths, classes):
    if logits.dim() != 3:
        raise ValueError('logits: expected [B, T, width], got %s' % (tuple(logits.shape),))
    if logits.dtype not in _DT:
        raise TypeError('logits: float32 or bfloat16 expected, got %s' % logits.dtype)
    if not torch.is_tensor(lengths) or lengths.dtype not in (torch.int32, torch.int64) or lengths.device != logits.device:
        raise TypeError('lengths: an int32 or int64 tensor on the device of the logits expected')
    lengths = lengths.reshape(-1).contiguous()
    if lengths.numel() != logits.shape[0]:
        raise ValueError('%d lengths for %d utterances' % (lengths.numel(), logits.shape[0]))
    return logits.contiguous(), lengths, logits.shape[-1] if classes is None else int(classes)


class _MaskedCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, lengths, K):
        B, T, ld = logits.shape
        dev = logits.device
        lse = torch.empty((B, T), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        correct = torch.empty(1, dtype=torch.int64, device=dev)
        ws = lib.workspace(int(lib.get().msmc_unit_ce_workspace(B, T)), dev, floor=4)
        lib.call('msmc_unit_ce_fwd', lib.ptr(logits), _DT[logits.dtype], lib.ptr(target, torch.int64), lib.ptr(lengths),
                 int(lengths.dtype == torch.int64), lib.ptr(lse), None, lib.ptr(out), lib.ptr(correct), lib.ptr(ws),
                 ws.numel() * ws.element_size(), B, T, K, ld, lib.stream(logits))
        ctx.save_for_backward(logits, target, lengths, lse, out)
        ctx.K = K
        ctx.mark_non_differentiable(correct)
        return out[0], correct[0]

    @staticmethod
    def backward(ctx, gout, _gcorrect):
        logits, target, lengths, lse, out = ctx.saved_tensors
        B, T, ld = logits.shape
        g = gout.reshape(1).float().contiguous()
        glogits = torch.empty_like(logits)
        lib.call('msmc_unit_ce_bwd', lib.ptr(logits), _DT[logits.dtype], lib.ptr(target), lib.ptr(lengths),
                 int(lengths.dtype == torch.int64), lib.ptr(lse), lib.ptr(out), lib.ptr(g), lib.ptr(glogits), B, T, ctx.K, ld,
                 lib.stream(logits))
        return glogits, None, None, None


def masked_cross_entropy(logits, target, lengths, classes=None, return_correct=False):
    """logits [B, T, width] fp32 or bf16, target [B, T] int64, lengths [B] int32 / int64 on the device -> the 0-dim fp32 loss
    ``sum over frames t < lengths[b] of -log softmax(logits[b, t, :classes])[target[b, t]] / lengths.sum()``.  ``classes``
    (default: the width) is the number of leading columns that are classes -- a projection built wider than the codebook passes
    the codebook's K; the other columns get a zero gradient.  A frame whose target is outside [0, classes) -- the -1 padding of
    unit labels -- adds no loss and gets a zero gradient; the denominator stays the sum of the lengths (all lengths zero: the loss
    is 0).  ``return_correct``: also the 0-dim int64 count of frames whose arg-max is the target.  Nothing is read back from the
    device.  Differentiable in ``logits`` (the gradient comes in their dtype)."""
    logits, lengths, K = _operands(logits, lengths, classes)
    if tuple(target.shape) != tuple(logits.shape[:2]):
        raise ValueError('target: expected %s, got %s' % (tuple(logits.shape[:2]), tuple(target.shape)))
    loss, correct = _MaskedCrossEntropy.apply(logits, target.detach().contiguous(), lengths, K)
    return (loss, correct) if return_correct else loss


def unit_argmax(logits, lengths, classes=None):
    """logits [B, T, width] fp32 or bf16, lengths [B] -> labels [B, T] int64: the arg-max over the first ``classes`` columns
    (lowest index on ties) where ``t < lengths[b]``, -1 elsewhere -- the forward's arg-max (``msmc_unit_argmax``)."""
    logits, lengths, K = _operands(logits.detach(), lengths, classes)
    B, T, ld = logits.shape
    pred = torch.empty((B, T), dtype=torch.int64, device=logits.device)
    lib.call('msmc_unit_argmax', lib.ptr(logits), _DT[logits.dtype], lib.ptr(lengths), int(lengths.dtype == torch.int64), lib.ptr(pred),
             B, T, K, ld, lib.stream(logits))
    return pred
