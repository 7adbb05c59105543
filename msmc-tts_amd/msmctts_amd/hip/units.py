"""From frames to discrete units on the gfx950 kernels: the step between fitting a k-means codebook (``fit_kmeans``) and training
on it.

``assign_units`` labels frames [N, d] with their nearest centre through ``msmc_vq_assign_wide`` (csrc/vq_assign.inc): the wide
search's labels, bit for bit, and the squared distance to the winner -- 12 bytes stored per frame where ``vq_search(...,
wide=True)`` stores 2 d 4 of quant and diff.  ``collapse_units`` cuts label sequences into (unit, duration) runs and
``unit_usage`` counts the frames per code (csrc/units.hip); ``usage_summary`` turns the counts into the two numbers the
reference prints (examples/qs-tts/scripts/vq_analysis.py ``compute_codebook_complexity``): codes used and their entropy in bits.

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


def usage_summary(counts):
    """(codes used, entropy in bits) of usage counts [K], in float64 on the host: the number of codes with a non-zero count and
    ``-sum p log2 p`` over them, p = count / total -- the two numbers of the reference's ``compute_codebook_complexity``"""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    used = c[c > 0].astype(np.float64)
    if used.size == 0:
        return 0, 0.0
    probs = used / used.sum()
    return int(used.size), float(-(probs * np.log2(probs)).sum())
