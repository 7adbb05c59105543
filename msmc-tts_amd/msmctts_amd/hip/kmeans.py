"""Fitting the k-means unit codebook of ``KMeansVQGANEmb`` on the gfx950 kernels: Lloyd's algorithm over frames [N, d].

The E step is the search the model itself runs (``vq.vq_prepare`` + ``vq.vq_search``: at unit widths ``msmc_vq_search_wide``,
csrc/vq_wide.inc); the M step is csrc/kmeans.hip: ``msmc_kmeans_stats`` (per-centroid sums and counts in a fixed summation
order, no floating-point atomics) and ``msmc_kmeans_update`` (the division and each centre's squared movement).  The reference
has no counterpart: it loads a model somebody fitted elsewhere (msmc_vqgan_emb.py:294-336).  ``fit_kmeans(...).save(path)``
writes the ``.npy`` of centres [K, d] that ``KMeansQuantizer`` reads.

There is no CPU path and no fallback: shapes the kernels refuse raise with the launcher's code, host tensors are uploaded
block by block, and without the library (or with a host ``device`` on the product build) the calls raise.
"""
import numpy as np
import torch

from . import lib
from . import vq as hipvq


class _Frames(object):
    """The frames [N, d] of a fit or a seeding -- a device tensor, a host tensor or a numpy array -- behind one way to read them:
    ``rows`` and ``take`` return fp32, contiguous rows on ``device``: where a device tensor lies, else ``device`` (default: the
    current GPU), uploaded by the call that asks for them"""

    def __init__(self, frames, device=None):
        if not torch.is_tensor(frames):
            frames = np.asarray(frames)
        if len(frames.shape) != 2:
            raise ValueError('frames: expected [N, d], got %s' % (tuple(frames.shape),))
        self.frames = frames
        self.N, self.d = int(frames.shape[0]), int(frames.shape[1])
        self.on_device = torch.is_tensor(frames) and frames.is_cuda
        self.device = frames.device if self.on_device else torch.device('cuda' if device is None else device)

    def _on_device(self, part):
        if not torch.is_tensor(part):
            part = torch.from_numpy(np.ascontiguousarray(part))
        return part.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def rows(self, s, e):
        return self._on_device(self.frames[s:e])

    def take(self, index):
        """the rows whose frame numbers a CPU int64 tensor lists, in its order"""
        if torch.is_tensor(self.frames):
            return self._on_device(self.frames[index.to(self.frames.device)])
        return self._on_device(self.frames[index.numpy()])


def _workspace(N, d, K, device, workspace=None):
    return lib.workspace(int(lib.get().msmc_kmeans_stats_workspace(N, d, K)), device, workspace)


def centroid_stats(x, ind, K, out=None, accumulate=False, workspace=None):
    """x [N, d] fp32, ind [N] int64 -> (sums [K, d], counts [K]) of the rows of every centroid; entries of ``ind`` outside
    [0, K) are skipped.  ``out``: a (sums, counts) pair to write, or with ``accumulate`` to add this call's totals onto (one add
    per element).  Deterministic; the summation order is documented at ``msmc_kmeans_stats`` (include/msmc_hip.h)."""
    N, d = x.shape
    K = int(K)
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs the (sums, counts) pair to add onto')
        out = (torch.empty((max(K, 0), d), dtype=torch.float32, device=x.device),
               torch.empty((max(K, 0),), dtype=torch.float32, device=x.device))
    sums, counts = out
    if K >= 1 and (tuple(sums.shape) != (K, d) or tuple(counts.shape) != (K,)):
        raise ValueError('out: sums [%d, %d] and counts [%d], got %s and %s' % (K, d, K, tuple(sums.shape), tuple(counts.shape)))
    xc = x.detach().contiguous()
    indc = ind.reshape(-1).contiguous()
    if indc.numel() != N:
        raise ValueError('%d labels for %d frames' % (indc.numel(), N))
    workspace = _workspace(N, d, K, x.device, workspace)
    lib.call('msmc_kmeans_stats', lib.ptr(xc, torch.float32), lib.ptr(indc, torch.int64), lib.ptr(sums, torch.float32),
             lib.ptr(counts, torch.float32), lib.ptr(workspace), workspace.numel() * workspace.element_size(), N, d, K,
             int(bool(accumulate)), lib.stream(xc))
    return sums, counts


def centroid_update(sums, counts, centers):
    """centers [K, d] in place: ``sums[k] / counts[k]`` where ``counts[k] > 0``, an empty centroid keeps its row; returns
    shift2 [K], the squared movement of every row (zero for an empty centroid)"""
    K, d = centers.shape
    shift2 = torch.empty((K,), dtype=torch.float32, device=centers.device)
    lib.call('msmc_kmeans_update', lib.ptr(sums, torch.float32), lib.ptr(counts, torch.float32), lib.ptr(centers, torch.float32),
             lib.ptr(shift2), d, K, lib.stream(centers))
    return shift2


MAX_LOCAL_TRIALS = 16                       # KPP_MAX_L of csrc/kmeans_pp.hip


def default_local_trials(K):
    """scikit-learn's ``2 + floor(ln K)`` candidates per seeding step, capped at what the kernel takes"""
    return min(MAX_LOCAL_TRIALS, 2 + int(np.log(K)))


def kmeans_plusplus(frames, n_clusters, seed=0, n_local_trials=None, first=None, uniforms=None, device=None):
    """Greedy k-means++ seeding on the gfx950 kernels (``msmc_kmeanspp_seed``, csrc/kmeans_pp.hip) -> ``(centers [K, d]
    float32, chosen [K] int64, potential [K] float64)``, tensors on the device: the chosen rows of ``frames``, their frame
    numbers, and the summed squared distance of every frame to its nearest centre after each pick.

    Centre 0 is frame ``first``; every further step draws ``n_local_trials`` candidates (default ``2 + floor(ln K)``, at most
    16) with probability proportional to the squared distance to the nearest centre so far -- candidate j of step i is the
    first frame whose running sum of those distances exceeds ``uniforms[i - 1, j]`` times their total -- and keeps the one
    that lowers the total most.  ``first`` and ``uniforms`` [K - 1, n_local_trials] float64 in [0, 1) default to
    ``randint(N)`` and ``rand(K - 1, n_local_trials, dtype=float64)`` drawn in that order from
    ``torch.Generator().manual_seed(seed)`` on the host.  A device tensor is seeded over all its frames where it lies; host
    frames are uploaded once, whole.  The whole seeding is enqueued without a read-back; every sum runs in a fixed order
    (include/msmc_hip.h), so the same inputs give the same bits."""
    frames = _Frames(frames, device)
    N, d, device = frames.N, frames.d, frames.device
    K = int(n_clusters)
    if N < 1 or K < 1:
        raise ValueError('kmeans_plusplus needs at least one frame and one cluster (got N = %d, n_clusters = %d)' % (N, K))
    L = default_local_trials(K) if n_local_trials is None else int(n_local_trials)
    gen = torch.Generator().manual_seed(int(seed))
    drawn = int(torch.randint(N, (1,), generator=gen))
    first = drawn if first is None else int(first)
    if uniforms is None:
        uniforms = torch.rand(max(K - 1, 0), max(L, 0), dtype=torch.float64, generator=gen)
    uniforms = torch.as_tensor(uniforms, dtype=torch.float64)
    if tuple(uniforms.shape) != (K - 1, L):
        raise ValueError('uniforms: expected [%d, %d], got %s' % (K - 1, L, tuple(uniforms.shape)))
    x = frames.rows(0, N)
    u = uniforms.to(device).contiguous()
    centers = torch.empty((K, d), dtype=torch.float32, device=device)
    chosen = torch.empty((K,), dtype=torch.int64, device=device)
    potential = torch.empty((K,), dtype=torch.float64, device=device)
    need = int(lib.get().msmc_kmeanspp_workspace(N, d, K, L))
    workspace = lib.workspace(need, device)
    lib.call('msmc_kmeanspp_seed', lib.ptr(x, torch.float32), N, d, K, L, first, lib.ptr(u, torch.float64), lib.ptr(centers),
             lib.ptr(chosen), lib.ptr(potential), lib.ptr(workspace), need, lib.stream(x))
    return centers, chosen, potential


class KMeansFit(object):
    """what ``fit_kmeans`` returns.  ``cluster_centers_`` [K, d] float32, ``labels_`` [N] int64 and ``inertia_``: the
    assignment of the frames to the RETURNED centres (a final search) and its summed squared error; ``n_iter_``: Lloyd
    iterations run; ``counts_`` [K] int64 and ``step_labels_`` [N] int64: the rows per centroid and the labels of the last M
    step, the one the returned centres are the means of (where the fit stopped because no label changed they are ``labels_``);
    ``history_``: per iteration ``{'inertia', 'empty', 'shift', 'changed'}`` -- the E step's summed squared error, the
    number of empty centroids, the summed squared movement of the centres and whether a label changed; ``init_indices_`` [K]
    int64: the frame numbers in ``frames`` of the first centres, None where ``init`` was an array."""

    def __init__(self, centers, labels, inertia, n_iter, counts, step_labels, history, init_indices=None):
        self.cluster_centers_, self.labels_, self.inertia_, self.n_iter_ = centers, labels, inertia, n_iter
        self.counts_, self.step_labels_, self.history_, self.init_indices_ = counts, step_labels, history, init_indices

    def save(self, path):
        """the centres as the ``.npy`` [K, d] that ``KMeansQuantizer`` / ``KMeansVQGANEmb(quantizer_path=...)`` load"""
        path = str(path)
        if not path.endswith('.npy'):
            raise ValueError('%s: the centroid file is recognised by its .npy suffix' % path)
        with open(path, 'wb') as fout:
            np.save(fout, self.cluster_centers_, allow_pickle=False)
        return path


def default_block_frames(d):
    """the largest block with block * d * 4 < 2^31 (the search kernels address a block's frames with 32-bit byte offsets)"""
    return max(1, ((1 << 31) - 1) // (4 * d))


def _mean_variance(frames, spans):
    """mean over the channels of the per-channel (population) variance of the frames, float64 sums over slabs of a block"""
    s1 = torch.zeros(frames.d, dtype=torch.float64, device=frames.device)
    s2 = torch.zeros(frames.d, dtype=torch.float64, device=frames.device)
    for s, e in spans:
        for slab in frames.rows(s, e).split(1 << 16):
            v = slab.double()
            s1 += v.sum(0)
            s2 += (v * v).sum(0)
    mean = s1 / frames.N
    return float((s2 / frames.N - mean * mean).clamp_(min=0).mean())


def _seed_plusplus(frames, K, seed, n_local_trials, seed_frames):
    """the first centres of ``fit_kmeans(init='k-means++')`` -> (centres [K, d] on the device, frame numbers [K] int64 numpy)"""
    N = frames.N
    if seed_frames is None:
        M = N if frames.on_device else min(N, 256 * K)
    else:
        M = min(N, int(seed_frames))
        if M < 1:
            raise ValueError('seed_frames must be positive')
    rows, sample = None, frames.frames
    if M < N:
        rows = torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:M]).values
        sample = frames.take(rows)
    centers, chosen, _ = kmeans_plusplus(sample, K, seed=seed, n_local_trials=n_local_trials, device=frames.device)
    chosen = chosen.cpu()
    return centers, (chosen if rows is None else rows[chosen]).numpy()


def fit_kmeans(frames, n_clusters, max_iter=100, tol=1e-4, seed=0, init=None, block_frames=None, device=None, callback=None,
               n_local_trials=None, seed_frames=None):
    """Lloyd's algorithm on the gfx950 kernels -> ``KMeansFit``.

    ``frames``: a device tensor, host tensor or numpy array [N, d] fp32, processed in blocks of ``block_frames`` frames
    (default: the largest block with block * d * 4 < 2^31); host data is uploaded block by block in every iteration, to
    ``device`` (default: the current GPU; a device tensor stays where it is).  ``init``: the first centres [K, d]; None draws K
    distinct frames with ``torch.Generator().manual_seed(seed)`` on the host; ``'k-means++'`` seeds them on the card
    (``kmeans_plusplus`` with ``seed`` and ``n_local_trials``) -- a device tensor over all its frames; host frames over a
    sample of ``seed_frames`` rows (drawn as the first ``seed_frames`` of ``randperm(N)`` from
    ``torch.Generator().manual_seed(seed)``, kept in frame order), uploaded once, so that K seeding passes do not upload
    the data K times.  ``seed_frames`` defaults to ``min(N, 256 * n_clusters)`` for host frames: 256 frames per centre is a
    stated choice, not a measurement (at K = 2000, d = 1024 it is 2 GB on the card); given explicitly it also samples a device
    tensor.  Any other string raises.  Every iteration prepares the centres (``vq_prepare``), then per block, in block order, searches
    (``vq_search``: labels and squared error) and accumulates the centroid statistics, then updates the centres
    (``msmc_kmeans_update``; an empty centroid keeps its row -- it is not relocated) and reads back, once, the summed squared
    movement of the centres, the inertia (the search's squared error summed in float64), whether a label changed and the
    number of empty centroids.  It stops when no label changed, when the movement is at most ``tol`` times the mean per-channel
    variance of the frames (scikit-learn's meaning of ``tol``), or after ``max_iter`` iterations.  Same inputs, same bits:
    every sum runs in a fixed order.  ``callback(iteration, record)`` is called with every ``history_`` record."""
    frames = _Frames(frames, device)
    N, d, device = frames.N, frames.d, frames.device
    K = int(n_clusters)
    if max_iter < 1:
        raise ValueError('max_iter must be at least 1')
    if N < 1 or K < 1:
        raise ValueError('fit_kmeans needs at least one frame and one cluster (got N = %d, n_clusters = %d)' % (N, K))
    block = default_block_frames(d) if block_frames is None else int(block_frames)
    if block < 1:
        raise ValueError('block_frames must be positive')
    spans = [(s, min(N, s + block)) for s in range(0, N, block)]

    init_indices = None
    if isinstance(init, str):
        if init != 'k-means++':
            raise ValueError("init: the first centres [K, d], None or 'k-means++', got %r" % (init,))
        centers, init_indices = _seed_plusplus(frames, K, seed, n_local_trials, seed_frames)
    elif init is None:
        if not 1 <= K <= N:
            raise ValueError('n_clusters = %d: cannot draw that many distinct frames from %d' % (K, N))
        pick = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:K]
        init_indices = pick.numpy()
        centers = frames.take(pick)
    else:
        centers = torch.as_tensor(np.asarray(init) if not torch.is_tensor(init) else init)
        if tuple(centers.shape) != (K, d):
            raise ValueError('init: expected [%d, %d], got %s' % (K, d, tuple(centers.shape)))
    centers = centers.detach().to(device=device, dtype=torch.float32).contiguous().clone()

    with torch.no_grad():
        limit = float(tol) * _mean_variance(frames, spans) if tol > 0 else 0.0
        sums = torch.empty((K, d), dtype=torch.float32, device=device)
        counts = torch.empty((K,), dtype=torch.float32, device=device)
        workspace = _workspace(min(N, block), d, K, device)

        def prepared():
            return hipvq.vq_prepare(centers.t().unsqueeze(0).contiguous(), frames=min(N, block))

        def e_step(embed_t, enorm, labels, stats):
            inertia = torch.zeros((), dtype=torch.float64, device=device)
            for b, (s, e) in enumerate(spans):
                xb = frames.rows(s, e)
                _, diff, ind = hipvq.vq_search(xb, embed_t, enorm)
                ind = ind.reshape(-1)
                inertia += diff.sum(dtype=torch.float64)
                labels[s:e] = ind
                if stats:
                    centroid_stats(xb, ind, K, out=(sums, counts), accumulate=b > 0, workspace=workspace)
            return inertia

        labels = torch.full((N,), -1, dtype=torch.int64, device=device)
        previous = torch.full((N,), -1, dtype=torch.int64, device=device)
        history, changed, n_iter = [], True, 0
        for it in range(int(max_iter)):
            labels, previous = previous, labels
            inertia = e_step(*prepared(), labels, True)
            shift2 = centroid_update(sums, counts, centers)
            back = torch.stack([shift2.sum(dtype=torch.float64), inertia, (labels != previous).any().double(),
                                (counts == 0).sum().double()]).cpu()           # the iteration's one read-back
            shift, changed = float(back[0]), bool(back[2] != 0)
            history.append({'inertia': float(back[1]), 'empty': int(back[3]), 'shift': shift, 'changed': changed})
            n_iter = it + 1
            if callback is not None:
                callback(n_iter, history[-1])
            if not changed or shift <= limit:
                break
        step_labels = labels
        if changed:             # the centres moved after the last search: the assignment to the returned centres
            final = torch.empty_like(labels)
            inertia = float(e_step(*prepared(), final, False))
        else:                   # the same labels gave the same sums, hence the same centres, bit for bit: that search stands
            final, inertia = labels, history[-1]['inertia']
        return KMeansFit(centers.cpu().numpy(), final.cpu().numpy(), inertia, n_iter, counts.cpu().numpy().astype(np.int64),
                         step_labels.cpu().numpy(), history, init_indices)
