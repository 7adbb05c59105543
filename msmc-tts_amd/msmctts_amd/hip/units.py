"""From frames to discrete units on the gfx950 kernels: the step between fitting a k-means codebook (``fit_kmeans``) and training
on it.

``assign_units`` labels frames [N, d] with their nearest centre through ``msmc_vq_assign_wide`` (csrc/vq_assign.inc): the wide
search's labels, bit for bit, and the squared distance to the winner -- 12 bytes stored per frame where ``vq_search(...,
wide=True)`` stores 2 d 4 of quant and diff.  ``collapse_units`` cuts label sequences into (unit, duration) runs and
``unit_usage`` counts the frames per code (csrc/units.hip); ``usage_summary`` turns the counts into the two numbers the
reference prints (examples/qs-tts/scripts/vq_analysis.py ``compute_codebook_complexity``): codes used and their entropy in bits.

The way back: ``expand_units`` turns (unit, duration) runs into frame labels again (csrc/units.hip) and ``unit_embed`` turns
frame labels into the synthesiser's decoder input -- rows of the projected codebook plus the utterance's global embedding, with
its gradient (csrc/unit_embed.hip): what ``KMeansVQGANEmb.forward_units`` / ``synthesis_units`` run.

There is no CPU path and no fallback: shapes the kernels refuse raise with the launcher's code, host frames are uploaded block
by block, and without the library (or with a host ``device`` on the product build) the calls raise.
"""
import numpy as np
import torch

from . import lib
from . import vq as hipvq
from .kmeans import _Frames, default_block_frames


def _centers(centers):
    """[K, d] float32 host or device tensor from a tensor, an array, a ``.npy`` path or what ``fit_kmeans`` returns"""
    if hasattr(centers, 'cluster_centers_'):
        centers = centers.cluster_centers_
    if isinstance(centers, (str, bytes)) or hasattr(centers, '__fspath__'):
        if not str(centers).endswith('.npy'):
            raise ValueError('%s: the centroid file is recognised by its .npy suffix' % (centers,))
        centers = np.load(centers, allow_pickle=False)
    if not torch.is_tensor(centers):
        centers = torch.from_numpy(np.ascontiguousarray(np.asarray(centers, dtype=np.float32)))
    if centers.dim() != 2:
        raise ValueError('centers: expected [K, d], got %s' % (tuple(centers.shape),))
    return centers


def assign_wide(x, embed_t, enorm, want_dist=True):
    """``msmc_vq_assign_wide`` on prepared centres: x [N, d] fp32 on the device, embed_t [1, K, d] / enorm [1, K] from
    ``vq_prepare`` -> (labels [N] int64, dist [N] float32 or None)"""
    _, K, d = embed_t.shape
    if embed_t.shape[0] != 1:
        raise RuntimeError('msmc_vq_assign_wide takes one head (got %d)' % embed_t.shape[0])
    if x.dim() != 2 or x.shape[1] != d:
        raise ValueError('frames [N, %d] expected, got %s' % (d, tuple(x.shape)))
    xc = x.detach().contiguous()
    N = xc.shape[0]
    ind = torch.empty((N,), dtype=torch.int64, device=xc.device)
    dist = torch.empty((N,), dtype=torch.float32, device=xc.device) if want_dist else None
    lib.call('msmc_vq_assign_wide', lib.ptr(xc, torch.float32), lib.ptr(embed_t, torch.float32), lib.ptr(enorm, torch.float32),
             lib.ptr(ind), lib.ptr(dist), N, d, K, lib.stream(xc))
    return ind, dist


def assign_units(frames, centers, block=None, want_dist=True, device=None):
    """Nearest-centre labels of ``frames`` [N, d] -> ``(labels [N] int64, dist [N] float32 or None)`` on the device.

    ``frames``: a device tensor, host tensor or numpy array; host frames are uploaded ``block`` frames at a time (default: the
    largest block with block * d * 4 < 2^31) to ``device`` (default: the current GPU; a device tensor stays where it is).
    ``centers`` [K, d]: a tensor, an array, a ``.npy`` path or the object ``fit_kmeans`` returns; prepared once
    (``vq_prepare``).  ``labels`` are the wide search's (``vq_search(..., wide=True)``), ``dist`` the squared distance to the
    winner as direct fp32 differences in the order documented at ``msmc_vq_assign_wide`` (include/msmc_hip.h): a frame that
    equals its centre gets exactly 0.  A frame's result depends on its own row only, so ``block`` does not show in the bits."""
    frames = _Frames(frames, device)
    N, d, device = frames.N, frames.d, frames.device
    centers = _centers(centers)
    if centers.shape[1] != d:
        raise ValueError('centers [K, %d] for frames [N, %d]' % (centers.shape[1], d))
    block = default_block_frames(d) if block is None else int(block)
    if block < 1:
        raise ValueError('block must be positive')
    with torch.no_grad():
        embed = centers.detach().to(device=device, dtype=torch.float32).t().unsqueeze(0).contiguous()       # [1, d, K]
        embed_t, enorm = hipvq.vq_prepare(embed, frames=0)
        labels = torch.empty((N,), dtype=torch.int64, device=device)
        dist = torch.empty((N,), dtype=torch.float32, device=device) if want_dist else None
        for s in range(0, N, block):
            e = min(N, s + block)
            ind, dd = assign_wide(frames.rows(s, e), embed_t, enorm, want_dist)
            labels[s:e] = ind
            if want_dist:
                dist[s:e] = dd
        if N == 0:          # (no block ran: the launcher still refuses a shape it does not take)
            assign_wide(torch.empty((0, d), dtype=torch.float32, device=device), embed_t, enorm, False)
    return labels, dist


def _labels_and_lengths(ind, length):
    if ind.dim() != 2:
        raise ValueError('ind: expected [B, T], got %s' % (tuple(ind.shape),))
    indc = ind.detach().contiguous()
    length = torch.as_tensor(length).to(device=indc.device, dtype=torch.int64).reshape(-1).contiguous()
    if length.numel() != indc.shape[0]:
        raise ValueError('%d lengths for %d utterances' % (length.numel(), indc.shape[0]))
    return indc, length


def collapse_units(ind, length):
    """ind [B, T] int64, length [B] -> ``(units [B, T] int64, dur [B, T] int32, ulen [B] int64)``: the maximal runs of equal
    labels in the valid prefix ``ind[b, :min(length[b], T)]`` -- run r is ``units[b, r]`` for ``dur[b, r]`` frames,
    ``ulen[b]`` runs; the slots beyond them hold -1 / 0.  ``repeat_interleave(units[b, :ulen[b]], dur[b, :ulen[b]])`` is the
    prefix again."""
    indc, length = _labels_and_lengths(ind, length)
    B, T = indc.shape
    units = torch.empty((B, T), dtype=torch.int64, device=indc.device)
    dur = torch.empty((B, T), dtype=torch.int32, device=indc.device)
    ulen = torch.empty((B,), dtype=torch.int64, device=indc.device)
    lib.call('msmc_units_collapse', lib.ptr(indc, torch.int64), lib.ptr(length), lib.ptr(units), lib.ptr(dur), lib.ptr(ulen), B, T,
             lib.stream(indc))
    return units, dur, ulen


def unit_usage(ind, length, K, counts=None):
    """counts [K] int64: the valid frames of ind [B, T] (t < length[b]) per label; labels outside [0, K) are skipped.
    ``counts``: a [K] int64 device tensor to add onto (a corpus, batch by batch); None starts from zero."""
    indc, length = _labels_and_lengths(ind, length)
    B, T = indc.shape
    K = int(K)
    accumulate = counts is not None
    if counts is None:
        counts = torch.empty((max(K, 0),), dtype=torch.int64, device=indc.device)
    elif K >= 1 and tuple(counts.shape) != (K,):
        raise ValueError('counts: expected [%d], got %s' % (K, tuple(counts.shape)))
    lib.call('msmc_units_usage', lib.ptr(indc, torch.int64), lib.ptr(length), lib.ptr(counts, torch.int64), B, T, K,
             int(accumulate), lib.stream(indc))
    return counts


def expand_units(units, dur, ulen, T=None):
    """The inverse of ``collapse_units``: units [B, R] int64, dur [B, R] (int32), ulen [B] -> ``(ind [B, T] int64, length [B]
    int64)``.  Run r < ulen[b] covers ``max(dur[b, r], 0)`` frames; ``ind[b, t]`` is the unit of the run that covers frame t,
    -1 behind the last run; ``length[b]`` the frames of utterance b, at most T (a longer sequence is cut).  ``T=None`` sizes the
    output by the longest utterance (at least one frame): ``msmc_units_total`` and ONE read-back of its maximum, a
    synchronisation -- pass T where it is known."""
    if units.dim() != 2:
        raise ValueError('units: expected [B, R], got %s' % (tuple(units.shape),))
    unitsc = units.detach().contiguous()
    B, R = unitsc.shape
    durc = torch.as_tensor(dur).detach().to(device=unitsc.device, dtype=torch.int32).contiguous()
    if tuple(durc.shape) != (B, R):
        raise ValueError('dur: expected %s, got %s' % ((B, R), tuple(durc.shape)))
    ulen = torch.as_tensor(ulen).to(device=unitsc.device, dtype=torch.int64).reshape(-1).contiguous()
    if ulen.numel() != B:
        raise ValueError('%d run counts for %d utterances' % (ulen.numel(), B))
    if T is None:
        total = torch.empty((max(B, 0),), dtype=torch.int64, device=unitsc.device)
        lib.call('msmc_units_total', lib.ptr(durc), lib.ptr(ulen), lib.ptr(total), B, R, lib.stream(unitsc))
        T = max(int(total.max()), 1)
    T = int(T)
    ind = torch.empty((B, max(T, 0)), dtype=torch.int64, device=unitsc.device)
    length = torch.empty((B,), dtype=torch.int64, device=unitsc.device)
    lib.call('msmc_units_expand', lib.ptr(unitsc, torch.int64), lib.ptr(durc), lib.ptr(ulen), lib.ptr(ind), lib.ptr(length), B, R, T,
             lib.stream(unitsc))
    return ind, length


class _UnitEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ind, length, table, glob):
        B, T = ind.shape
        K, C = table.shape
        tablec = table.detach().contiguous()
        globc = None if glob is None else glob.detach().contiguous()
        out = torch.empty((B, T, C), dtype=torch.float32, device=tablec.device)
        lib.call('msmc_units_embed_fwd', lib.ptr(ind, torch.int64), lib.ptr(length, torch.int64), lib.ptr(tablec, torch.float32),
                 lib.ptr(globc, torch.float32), lib.ptr(out), B, T, C, K, lib.stream(tablec))
        ctx.save_for_backward(ind, length)
        ctx.sizes = (B, T, C, K, glob is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        ind, length = ctx.saved_tensors
        B, T, C, K, with_glob = ctx.sizes
        goutc = gout.contiguous()
        gtable = torch.empty((K, C), dtype=torch.float32, device=goutc.device)
        gglob = torch.empty((B, C), dtype=torch.float32, device=goutc.device) if with_glob and ctx.needs_input_grad[3] else None
        ws = lib.workspace(int(lib.get().msmc_units_embed_workspace(B * T, C, K)), goutc.device)
        lib.call('msmc_units_embed_bwd', lib.ptr(goutc, torch.float32), lib.ptr(ind), lib.ptr(length), lib.ptr(gtable), lib.ptr(gglob),
                 lib.ptr(ws), ws.numel() * ws.element_size(), B, T, C, K, lib.stream(goutc))
        return None, None, gtable, gglob


def unit_embed(ind, length, table, glob=None):
    """The decoder input from unit labels: ind [B, T] int64, length [B], table [K, C] fp32, glob [B, C] fp32 or None ->
    out [B, T, C] fp32 with ``out[b, t] = table[ind[b, t]] + glob[b]`` where ``t < length[b]`` and ``0 <= ind[b, t] < K``, zeros
    in every other row (``msmc_units_embed_fwd``, csrc/unit_embed.hip).  Differentiable in ``table`` and ``glob``
    (``msmc_units_embed_bwd``: per-label and per-utterance sums of the incoming gradient in the fixed order of the k-means
    statistics pass, no atomics, same inputs same bits); ``ind`` and ``length`` get no gradient."""
    indc, length = _labels_and_lengths(ind, length)
    if table.dim() != 2:
        raise ValueError('table: expected [K, C], got %s' % (tuple(table.shape),))
    if glob is not None and tuple(glob.shape) != (indc.shape[0], table.shape[1]):
        raise ValueError('glob: expected %s, got %s' % ((indc.shape[0], table.shape[1]), tuple(glob.shape)))
    return _UnitEmbed.apply(indc, length, table, glob)


def usage_summary(counts):
    """(codes used, entropy in bits) of usage counts [K], in float64 on the host: the number of codes with a non-zero count and
    ``-sum p log2 p`` over them, p = count / total -- the two numbers of the reference's ``compute_codebook_complexity``"""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    used = c[c > 0].astype(np.float64)
    if used.size == 0:
        return 0, 0.0
    probs = used / used.sum()
    return int(used.size), float(-(probs * np.log2(probs)).sum())
