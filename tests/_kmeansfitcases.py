"""Shared cases of the k-means fit on the gfx950 kernels: the centroid statistics and update kernels (csrc/kmeans.hip:
msmc_kmeans_stats, msmc_kmeans_update), ``centroid_stats`` / ``fit_kmeans`` (msmctts_amd/hip/kmeans.py) and the file they write
for ``KMeansQuantizer``.  tests/test_kmeans_fit_emu.py runs them on the kernel interpreter, tests/test_gpu_kmeans_fit.py on the GPU.

Statistics reference.  ``restated_stats`` is the kernel's documented summation order in numpy fp32 -- the rows of a centroid in
ascending n, in runs of 64, every run summed from +0 in ascending n, the run partials added from +0 in ascending order, with
``accumulate`` one more add onto what the buffers hold -- and must match BIT FOR BIT (both builds compile with
-ffp-contract=off: plain IEEE adds on either side).  Independently, every element of ``sums`` must lie within
``n_k 2^-24 sum|x|`` of the float64 sum: the recursive-summation bound, which holds for any order of n_k - 1 adds (the run
structure adds only exact +0 terms), so no number in it is measured.  ``counts`` must be exact.

Update reference.  ``sums / counts`` in float64: IEEE fp32 division is correctly rounded, so the kernel's quotient is within
``2^-24 |q|`` (half an ulp) of it; normal numbers only (N(0, 1) data).  ``shift2`` against the restated order: lane l of 64 adds
``(new - old)^2`` of the 4-channel pieces l, l + 64, ... in ascending channel order from +0, then the butterfly
``v = v + v[lane ^ m]``, m = 1, 2, 4, 8, 16, 32 -- bit for bit.

Fit references.  ``lloyd_numpy`` is Lloyd's algorithm in numpy, in float64 and in float32, from the same init and with the same
empty-centroid rule (an empty centroid keeps its row) and stopping rule as ``fit_kmeans``.  The blob cases have first-to-second
distance margins down to 2e-6 relative, so fp32 may flip a few assignments: labels and centres of two runs are never compared
one for one, only the final inertia, whose allowed relative gap is ten times the gap observed between the two numpy runs,
floored at 1e-6 (``inertia_gap_allowed``; the observed values are in profiles/kmeans_fit.md).
"""
import ctypes
import functools
import os

import numpy as np
import torch

from _vqstreamcases import E_SHAPE, _raises, same_bits

E_WORKSPACE = -3
RUN = 64                                                    # rows per run (KM_RUN of csrc/kmeans.hip)

# ---- (a) statistics kernel -----------------------------------------------------------------------------------------------------
# d, K, N; the last: four parts of the counting sort with two placement tiles each, every centroid in several of them
STATS_SHAPES = ((4, 1, 1), (16, 5, 257), (272, 24, 300), (1024, 100, 300), (2048, 40, 64), (768, 2000, 300), (64, 3, 1031),
                (8, 300, 2000))
STATS_IDS = ['d%d K%d N%d' % s for s in STATS_SHAPES]
ONE_CENTROID = 6                                            # every frame on centroid 1: one centroid spans 17 runs


@functools.lru_cache(maxsize=None)
def stats_problem(s):
    """seeded N(0, 1) frames [N, d] and labels [N] (host tensors, computed once, never modified)"""
    d, K, N = STATS_SHAPES[s]
    gen = torch.Generator().manual_seed(5100 + s)
    x = torch.randn(N, d, generator=gen)
    ind = torch.randint(0, K, (N,), generator=gen)
    if s == ONE_CENTROID:
        ind = torch.ones(N, dtype=torch.int64)
    return x.contiguous(), ind.contiguous()


def restated_stats(x, ind, K, sums=None, counts=None):
    """the summation order of msmc_kmeans_stats in numpy fp32 -> (sums [K, d], counts [K]); ``sums`` / ``counts`` given: accumulate"""
    x, ind = np.asarray(x, dtype=np.float32), np.asarray(ind)
    d = x.shape[1]
    out_s, out_c = np.empty((K, d), dtype=np.float32), np.empty((K,), dtype=np.float32)
    for k in range(K):
        rows = np.flatnonzero(ind == k)
        total = np.zeros(d, dtype=np.float32)
        for r0 in range(0, len(rows), RUN):
            part = np.zeros(d, dtype=np.float32)
            for n in rows[r0:r0 + RUN]:
                part = part + x[n]
            total = total + part
        n = np.float32(len(rows))
        out_s[k] = total if sums is None else sums[k] + total
        out_c[k] = n if counts is None else counts[k] + n
    return out_s, out_c


def float64_stats(x, ind, K):
    """-> (float64 sums [K, d], sum of |x| [K, d], rows per centroid [K])"""
    x, ind = np.asarray(x, dtype=np.float64), np.asarray(ind)
    ok = (ind >= 0) & (ind < K)
    s, a = np.zeros((K, x.shape[1])), np.zeros((K, x.shape[1]))
    np.add.at(s, ind[ok], x[ok])
    np.add.at(a, ind[ok], np.abs(x[ok]))
    return s, a, np.bincount(ind[ok], minlength=K)


def run_stats(dev, x, ind, K, N=None, sums=None, counts=None, accumulate=0, extra_rows=0, ws_bytes=None):
    """msmc_kmeans_stats directly -> (rc, sums, counts) on the host.  Without ``sums`` / ``counts`` the output buffers are
    ``extra_rows`` rows longer than K, NaN / -7 filled; ``N``: the frame count passed (default: all of x)"""
    from msmctts_amd.hip import lib
    d = x.shape[1]
    N = x.shape[0] if N is None else N
    L = lib.get()
    rows = max(K, 0) + extra_rows
    sums = torch.full((rows, d), float('nan')) if sums is None else sums.clone()
    counts = torch.full((rows,), -7.0) if counts is None else counts.clone()
    xd, indd, sums, counts = x.to(dev), ind.to(dev), sums.to(dev), counts.to(dev)
    need = int(L.msmc_kmeans_stats_workspace(N, d, K))
    have = int(L.msmc_kmeans_stats_workspace(max(0, min(N, x.shape[0])), d, K))        # (a refused N is never allocated for)
    ws = torch.empty(have // 4 + 4, dtype=torch.float32).to(dev)
    rc = L.msmc_kmeans_stats(lib.ptr(xd), lib.ptr(indd), lib.ptr(sums), lib.ptr(counts), lib.ptr(ws),
                             need if ws_bytes is None else ws_bytes, N, d, K, accumulate, lib.stream(xd))
    return rc, sums.cpu(), counts.cpu()


def assert_stats(got_s, got_c, x, ind, K, want=None, what=''):
    """bit identity with the restated order, exact counts, and the float64 bound of the module docstring"""
    want_s, want_c = restated_stats(x, ind, K) if want is None else want
    assert torch.equal(got_c, torch.from_numpy(want_c)), '%s counts' % what
    s64, a64, n = float64_stats(x, ind, K)
    if want is None:
        assert np.array_equal(want_c, n.astype(np.float32))
    err = np.abs(got_s.double().numpy() - s64)
    bound = n[:, None] * 2.0 ** -24 * a64
    worst = float((err - bound).max())
    print('%s sums: largest error %.3g, largest error / bound %.3g' % (what, float(err.max()), float((err / np.maximum(bound, 1e-300)).max())))
    assert worst <= 0.0, '%s sums beyond n_k 2^-24 sum|x| of the float64 sums by %.3g' % (what, worst)
    assert same_bits(got_s, torch.from_numpy(want_s)), '%s sums are not the bits of the restated order (%d elements differ)' % (
        what, int((got_s.view(torch.int32) != torch.from_numpy(want_s).view(torch.int32)).sum()))


def check_stats_shape(dev, s):
    d, K, N = STATS_SHAPES[s]
    x, ind = stats_problem(s)
    rc, sums, counts = run_stats(dev, x, ind, K)
    assert rc == 0, rc
    assert_stats(sums, counts, x, ind, K, what='d=%d K=%d N=%d' % (d, K, N))
    if s == ONE_CENTROID:
        assert counts.tolist() == [0.0, float(N), 0.0] and N > 16 * RUN
        assert not bool(sums[0].any()) and not bool(sums[2].any())
    # the host wrapper, same bits
    from msmctts_amd.hip import kmeans
    s2, c2 = kmeans.centroid_stats(x.to(dev), ind.to(dev), K)
    assert same_bits(s2.cpu(), sums) and same_bits(c2.cpu(), counts)


def check_skipped_labels(dev):
    """labels -1 and K (and far outside) are the padding mask: skipped by the counts and by the sums"""
    s = 2
    d, K, N = STATS_SHAPES[s]
    x, ind = stats_problem(s)
    ind = ind.clone()
    ind[::7] = -1
    ind[3::11] = K
    ind[5] = -(1 << 40)
    ind[6] = 1 << 40
    rc, sums, counts = run_stats(dev, x, ind, K)
    assert rc == 0
    keep = (ind >= 0) & (ind < K)
    assert float(counts.sum()) == float(keep.sum()) and int(keep.sum()) < N - 60
    assert_stats(sums, counts, x, ind, K, what='masked')
    # ... and every frame masked: zeros
    rc, sums, counts = run_stats(dev, x, torch.full((N,), -1, dtype=torch.int64), K)
    assert rc == 0 and not bool(sums.any()) and not bool(counts.any())


def check_no_frames(dev):
    """N = 0: returns 0; without accumulate zeros, with accumulate the buffers as they were (no workspace in either case)"""
    d, K = 16, 5
    x, ind = torch.zeros(0, d), torch.zeros(0, dtype=torch.int64)
    rc, sums, counts = run_stats(dev, x, ind, K, extra_rows=3, ws_bytes=0)
    assert rc == 0
    assert not bool(sums[:K].any()) and not bool(counts[:K].any())
    assert bool(torch.isnan(sums[K:]).all()) and bool((counts[K:] == -7).all())
    s0, c0 = torch.full((K, d), 2.5), torch.full((K,), 3.0)
    rc, sums, counts = run_stats(dev, x, ind, K, sums=s0, counts=c0, accumulate=1, ws_bytes=0)
    assert rc == 0 and torch.equal(sums, s0) and torch.equal(counts, c0)


def check_oversized_buffers(dev):
    """rows of sums / counts beyond K stay untouched; frames and labels beyond N are not read into any sum"""
    s = 1
    d, K, N = STATS_SHAPES[s]
    x, ind = stats_problem(s)
    n = N - 57
    rc, sums, counts = run_stats(dev, x, ind, K, N=n, extra_rows=9)
    assert rc == 0
    assert bool(torch.isnan(sums[K:]).all()) and bool((counts[K:] == -7).all())
    assert_stats(sums[:K].contiguous(), counts[:K].contiguous(), x[:n], ind[:n], K, what='first %d of %d frames' % (n, N))


def check_accumulate(dev):
    """300 frames folded in blocks of 97, in block order, against the same order in numpy; and through ``centroid_stats``"""
    s = 3
    d, K, N = STATS_SHAPES[s]
    x, ind = stats_problem(s)
    sums = counts = want_s = want_c = None
    for b, s0 in enumerate(range(0, N, 97)):
        xb, ib = x[s0:s0 + 97].contiguous(), ind[s0:s0 + 97].contiguous()
        rc, sums, counts = run_stats(dev, xb, ib, K, sums=sums, counts=counts, accumulate=int(b > 0))
        assert rc == 0
        want_s, want_c = restated_stats(xb, ib, K, want_s, want_c)
    assert_stats(sums, counts, x, ind, K, want=(want_s, want_c), what='accumulated')
    assert float(counts.sum()) == N
    from msmctts_amd.hip import kmeans
    out = None
    for b, s0 in enumerate(range(0, N, 97)):
        out = kmeans.centroid_stats(x[s0:s0 + 97].to(dev), ind[s0:s0 + 97].to(dev), K, out=out, accumulate=b > 0)
    assert same_bits(out[0].cpu(), sums) and same_bits(out[1].cpu(), counts)
    with _raises(ValueError, 'accumulate needs'):
        kmeans.centroid_stats(x.to(dev), ind.to(dev), K, accumulate=True)


def check_refusals(dev):
    """d = 6, d = 2052, K = 0, N * d * 4 >= 2^32: MSMC_E_SHAPE; a short workspace: MSMC_E_WORKSPACE; guard values intact"""
    from msmctts_amd.hip import kmeans, lib
    gen = torch.Generator().manual_seed(5190)

    def intact(sums, counts):
        return bool(torch.isnan(sums).all()) and bool((counts == -7).all())

    for d, K in ((6, 5), (2052, 5), (16, 0)):
        x, ind = torch.randn(9, d, generator=gen), torch.zeros(9, dtype=torch.int64)
        rc, sums, counts = run_stats(dev, x, ind, K, extra_rows=5)
        assert rc == E_SHAPE and intact(sums, counts), (d, K, rc)
        assert int(lib.get().msmc_kmeans_stats_workspace(9, d, K)) == 0
    # N * d * 4 >= 2^32 is refused before anything is read
    x, ind = torch.randn(9, 64, generator=gen), torch.zeros(9, dtype=torch.int64)
    rc, sums, counts = run_stats(dev, x, ind, 5, N=1 << 24, ws_bytes=1 << 40)
    assert rc == E_SHAPE and intact(sums, counts), rc
    rc, sums, counts = run_stats(dev, x, ind, 5, N=-1, ws_bytes=1 << 40)
    assert rc == E_SHAPE and intact(sums, counts), rc
    # a workspace one byte short
    s = 1
    d, K, N = STATS_SHAPES[s]
    x, ind = stats_problem(s)
    need = int(lib.get().msmc_kmeans_stats_workspace(N, d, K))
    assert need >= 4 * N + 4 * d * (N // RUN)
    rc, sums, counts = run_stats(dev, x, ind, K, ws_bytes=need - 1)
    assert rc == E_WORKSPACE and intact(sums, counts), rc
    # the wrappers raise with the launcher's code
    with _raises(RuntimeError, 'msmc_kmeans_stats failed with code -2'):
        kmeans.centroid_stats(torch.zeros(9, 6).to(dev), torch.zeros(9, dtype=torch.int64).to(dev), 5)
    with _raises(RuntimeError, 'msmc_kmeans_update failed with code -2'):
        kmeans.centroid_update(torch.zeros(5, 6).to(dev), torch.zeros(5).to(dev), torch.zeros(5, 6).to(dev))
    with _raises(RuntimeError, 'failed with code -2'):
        kmeans.fit_kmeans(torch.randn(40, 6, generator=gen), 3, device=dev)


def check_workspace_size():
    """O(N + K + runs * d), never a [K][d] partial per tile: at the sizes of the issue the EMA kernel's layout would be 8 MB per
    16-frame tile"""
    from msmctts_amd.hip import lib
    L = lib.get()
    N, d, K = 1 << 20, 1024, 2000
    need = int(L.msmc_kmeans_stats_workspace(N, d, K))
    runs = N // RUN + K
    assert need <= 4 * (N + 258 * (K + 1)) + 16 + 4 * d * runs, need
    assert need < (4 * N * d) // 32                         # a small fraction of x itself


# ---- (b) update kernel ---------------------------------------------------------------------------------------------------------
def restated_update(sums, counts, centers):
    """-> (new centres, shift2) in the order of msmc_kmeans_update, numpy fp32"""
    sums, counts, centers = (np.asarray(a, dtype=np.float32) for a in (sums, counts, centers))
    K, d = centers.shape
    new, shift2 = centers.copy(), np.zeros(K, dtype=np.float32)
    lanes = np.arange(64)
    for k in range(K):
        if not counts[k] > 0:
            continue
        new[k] = sums[k] / counts[k]
        df = new[k] - centers[k]
        sq = (df * df).reshape(d // 4, 4)
        v = np.zeros(64, dtype=np.float32)
        for q in range(d // 4):
            for j in range(4):
                v[q % 64] = v[q % 64] + sq[q, j]
        for m in (1, 2, 4, 8, 16, 32):
            v = v + v[lanes ^ m]
        shift2[k] = v[0]
    return new, shift2


def check_update(dev, d, K):
    from msmctts_amd.hip import kmeans
    gen = torch.Generator().manual_seed(5200 + d)
    sums = torch.randn(K, d, generator=gen) * 7.0
    counts = torch.randint(0, 40, (K,), generator=gen).float()
    counts[0], counts[K - 1] = 0.0, 3.0
    if K > 2:
        counts[K // 2] = 0.0
    centers = torch.randn(K, d, generator=gen)
    got = centers.clone().to(dev)
    shift2 = kmeans.centroid_update(sums.to(dev), counts.to(dev), got).cpu()
    got = got.cpu()
    empty = counts == 0
    assert int(empty.sum()) >= 1 and same_bits(got[empty], centers[empty]), 'an empty centroid must keep the bits of its row'
    assert not bool(shift2[empty].any())
    q = sums.double() / counts.double().unsqueeze(1)
    err = (got.double() - q).abs()[~empty]
    # (1 + 2^-20: the float64 quotient is itself rounded)
    assert bool((err <= 2.0 ** -24 * (1 + 2.0 ** -20) * q.abs()[~empty]).all()), 'sums / counts beyond half an ulp of the float64 quotient: %.3g' % float(err.max())
    new, want = restated_update(sums, counts, centers)
    assert same_bits(got, torch.from_numpy(new))
    assert same_bits(shift2, torch.from_numpy(want)), (shift2[:4].tolist(), want[:4].tolist())
    moved = ((got.double() - centers.double()) ** 2).sum(1)
    # all terms positive: one rounding of the difference (counted twice in the square), one of the square, d / 64 adds in a
    # lane's chain, 6 butterfly adds -> relative error below (d / 64 + 10) 2^-24 of the float64 sum of the same differences
    assert torch.allclose(shift2.double(), moved, rtol=(d / 64 + 10) * 2.0 ** -24, atol=0.0)


# ---- (c) blob problems and the numpy Lloyd references ------------------------------------------------------------------------------
FIT_SHAPES = ((16, 5, 257), (272, 24, 1500), (1024, 100, 3000))                   # d, K, N
FIT_IDS = ['d%d K%d N%d' % s for s in FIT_SHAPES]
FIT_SEED = 7
TOL = 1e-4
MAX_ITER = 100


@functools.lru_cache(maxsize=None)
def blobs(i):
    """K true centres N(0, 1), noise 0.25, frames rounded to fp32; init: K distinct frames drawn as ``fit_kmeans(seed=FIT_SEED)``
    draws them -> (frames [N, d] float32 numpy, init [K, d] float32 numpy), never modified"""
    d, K, N = FIT_SHAPES[i]
    rng = np.random.default_rng(5300 + i)
    true = rng.standard_normal((K, d))
    x = (true[rng.integers(0, K, N)] + 0.25 * rng.standard_normal((N, d))).astype(np.float32)
    pick = torch.randperm(N, generator=torch.Generator().manual_seed(FIT_SEED))[:K].numpy()
    return x, x[pick].copy()


def assign_numpy(x, centers):
    """-> (labels: first minimum of |x|^2 - 2 x.c + |c|^2, inertia: sum of |x - c_label|^2) in the dtype of ``x``"""
    dist = ((x * x).sum(1, keepdims=True) - 2 * (x @ centers.T)) + (centers * centers).sum(1)[None, :]
    labels = dist.argmin(1)
    e = x - centers[labels]
    return labels, float((e.astype(np.float64) ** 2).sum())


def lloyd_numpy(x, init, dtype, max_iter=MAX_ITER, tol=TOL):
    """Lloyd's algorithm with the rules of ``fit_kmeans`` (an empty centroid keeps its row; stop when no label changed or the
    summed squared movement is at most tol * mean per-channel variance) -> dict of centres, labels, inertia, n_iter, history"""
    x, centers = np.asarray(x, dtype=dtype), np.array(init, dtype=dtype)
    K = centers.shape[0]
    limit = tol * float(np.asarray(x, dtype=np.float64).var(axis=0).mean())
    previous, history, changed = None, [], True
    for it in range(max_iter):
        labels, inertia = assign_numpy(x, centers)
        history.append(inertia)
        old = centers.copy()
        for k in range(K):
            rows = labels == k
            if rows.any():
                centers[k] = x[rows].sum(0, dtype=dtype) / dtype(rows.sum())
        changed = previous is None or bool((labels != previous).any())
        previous = labels
        shift = float(((centers.astype(np.float64) - old.astype(np.float64)) ** 2).sum())
        if not changed or shift <= limit:
            break
    if changed:
        labels, inertia = assign_numpy(x, centers)
    return {'centers': centers, 'labels': labels, 'inertia': inertia, 'n_iter': it + 1, 'history': history,
            'empty': K - len(np.unique(previous))}


@functools.lru_cache(maxsize=None)
def lloyd_reference(i, bits):
    x, init = blobs(i)
    return lloyd_numpy(x, init, np.float64 if bits == 64 else np.float32)


def inertia_gap_allowed(i):
    """ten times the relative inertia gap of the fp32 numpy Lloyd against the float64 one, floored at 1e-6 -> (allowed, observed)"""
    i64, i32 = lloyd_reference(i, 64)['inertia'], lloyd_reference(i, 32)['inertia']
    observed = abs(i32 - i64) / i64
    return max(10.0 * observed, 1e-6), observed


@functools.lru_cache(maxsize=None)
def fitted(dev, i):
    """the fit the tests of case i share (single block, explicit init); never modified"""
    from msmctts_amd.hip import kmeans
    x, init = blobs(i)
    return kmeans.fit_kmeans(x, FIT_SHAPES[i][1], max_iter=MAX_ITER, tol=TOL, init=init, device=dev)


def same_fit(a, b):
    return (same_bits(torch.from_numpy(a.cluster_centers_), torch.from_numpy(b.cluster_centers_))
            and np.array_equal(a.labels_, b.labels_) and a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_
            and np.array_equal(a.counts_, b.counts_) and np.array_equal(a.step_labels_, b.step_labels_) and a.history_ == b.history_)


# ---- (d) one Lloyd step ---------------------------------------------------------------------------------------------------------
def check_one_step(dev, i):
    """``fit_kmeans(max_iter=1)``: the labels it used are those of ``vq_search`` on the same centres, the new centres are the
    update of the statistics of those labels -- through the wrappers and against the numpy restatements, bit for bit"""
    from msmctts_amd.hip import kmeans, vq
    d, K, N = FIT_SHAPES[i]
    x, init = blobs(i)
    fit = kmeans.fit_kmeans(x, K, max_iter=1, init=init, device=dev)
    assert fit.n_iter_ == 1 and len(fit.history_) == 1
    xd, c0 = torch.from_numpy(x).to(dev), torch.from_numpy(init).to(dev)
    et, en = vq.vq_prepare(c0.t().unsqueeze(0).contiguous(), frames=N)
    _, diff, ind = vq.vq_search(xd, et, en)
    ind = ind.reshape(-1)
    assert torch.equal(torch.from_numpy(fit.step_labels_), ind.cpu()), 'the labels of the M step are not those of vq_search'
    assert fit.history_[0]['inertia'] == float(diff.sum(dtype=torch.float64))
    sums, counts = kmeans.centroid_stats(xd, ind, K)
    centers = c0.clone()
    shift2 = kmeans.centroid_update(sums, counts, centers)
    assert same_bits(torch.from_numpy(fit.cluster_centers_), centers.cpu()), 'the new centres are not the update of the statistics'
    assert fit.history_[0]['shift'] == float(shift2.sum(dtype=torch.float64))
    assert np.array_equal(fit.counts_, np.bincount(fit.step_labels_, minlength=K))
    empty = fit.counts_ == 0
    print('centroids without a frame in the first step: %d' % int(empty.sum()))
    assert np.array_equal(fit.cluster_centers_[empty].view(np.int32), init[empty].view(np.int32)), 'an empty centroid keeps its row'
    assert fit.history_[0]['empty'] == int(empty.sum())
    want_s, want_c = restated_stats(x, fit.step_labels_, K)
    new, _ = restated_update(want_s, want_c, init)
    assert same_bits(torch.from_numpy(fit.cluster_centers_), torch.from_numpy(new)), 'the new centres against the numpy restatement'
    # labels_ belong to the RETURNED centres
    et, en = vq.vq_prepare(centers.t().unsqueeze(0).contiguous(), frames=N)
    _, diff, ind = vq.vq_search(xd, et, en)
    assert np.array_equal(fit.labels_, ind.reshape(-1).cpu().numpy()) and fit.inertia_ == float(diff.sum(dtype=torch.float64))


# ---- (e) the fit ----------------------------------------------------------------------------------------------------------------
def check_fit_is_deterministic(dev, i):
    """two fits with the same seed are bit-identical in every returned array (the seed draws the init of ``blobs``)"""
    from msmctts_amd.hip import kmeans
    x, init = blobs(i)
    K = FIT_SHAPES[i][1]
    a = kmeans.fit_kmeans(x, K, max_iter=MAX_ITER, tol=TOL, seed=FIT_SEED, device=dev)
    b = kmeans.fit_kmeans(torch.from_numpy(x).to(dev), K, max_iter=MAX_ITER, tol=TOL, seed=FIT_SEED, device=dev)
    assert same_fit(a, b), 'two fits with the same seed differ'
    assert same_fit(a, fitted(dev, i)), 'the seeded draw is not K distinct frames of randperm(N, Generator(seed))[:K]'


def check_fit_in_blocks(dev, i):
    """blocks of 97 frames: the same labels and counts as the single-block fit"""
    from msmctts_amd.hip import kmeans
    x, init = blobs(i)
    one = fitted(dev, i)
    many = kmeans.fit_kmeans(x, FIT_SHAPES[i][1], max_iter=MAX_ITER, tol=TOL, init=init, block_frames=97, device=dev)
    assert np.array_equal(many.labels_, one.labels_) and np.array_equal(many.counts_, one.counts_)
    assert np.array_equal(many.step_labels_, one.step_labels_) and many.n_iter_ == one.n_iter_


def check_fit_properties(dev, i):
    d, K, N = FIT_SHAPES[i]
    x, init = blobs(i)
    fit = fitted(dev, i)
    assert fit.cluster_centers_.shape == (K, d) and fit.cluster_centers_.dtype == np.float32
    assert fit.labels_.shape == (N,) and fit.labels_.dtype == np.int64 and fit.counts_.dtype == np.int64
    assert 1 <= fit.n_iter_ == len(fit.history_) <= MAX_ITER
    assert int(fit.counts_.sum()) == N
    assert np.array_equal(fit.counts_, np.bincount(fit.step_labels_, minlength=K))
    assert fit.history_[-1]['empty'] == int((fit.counts_ == 0).sum())
    # every non-empty centre is the mean of its frames of the last M step: sums within n_k 2^-24 sum|x| of float64 (the bound of
    # the statistics), divided by n_k, plus half an ulp of the quotient for the division
    s64, a64, n = float64_stats(x, fit.step_labels_, K)
    full = n > 0
    mean = s64[full] / n[full, None]
    err = np.abs(fit.cluster_centers_[full].astype(np.float64) - mean)
    bound = 2.0 ** -24 * (1 + 2.0 ** -20) * (a64[full] + np.abs(mean))
    print('centres against the float64 means: largest error / bound %.3g' % float((err / bound).max()))
    assert bool((err <= bound).all())
    # inertia: never up by more than 2^-20 of itself from one iteration to the next, nor to the final assignment
    series = [h['inertia'] for h in fit.history_] + [fit.inertia_]
    print('inertia per iteration:', ' '.join('%.9g' % v for v in series))
    for a, b in zip(series, series[1:]):
        assert b <= a + 2.0 ** -20 * a, (a, b)
    e = x.astype(np.float64) - fit.cluster_centers_.astype(np.float64)[fit.labels_]
    assert abs(float((e * e).sum()) - fit.inertia_) <= 1e-5 * fit.inertia_


def check_saved_file_is_the_quantisers(dev, i, tmpdir):
    """``save()`` then ``KMeansQuantizer(path)`` on the same frames returns ``labels_`` exactly"""
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansQuantizer, fit_kmeans
    from msmctts_amd.hip import kmeans
    assert fit_kmeans is kmeans.fit_kmeans
    d, K, N = FIT_SHAPES[i]
    x, _ = blobs(i)
    fit = fitted(dev, i)
    path = fit.save(os.path.join(str(tmpdir), 'units.npy'))
    assert same_bits(torch.from_numpy(np.load(path)), torch.from_numpy(fit.cluster_centers_))
    q = KMeansQuantizer(path).to(dev).eval()
    with torch.no_grad():
        out = q([(torch.from_numpy(x).view(1, N, d).to(dev), torch.tensor([N]).to(dev))])
    assert np.array_equal(out['quantizer_indices'][0].reshape(-1).cpu().numpy(), fit.labels_)
    with _raises(ValueError, '.npy suffix'):
        fit.save(os.path.join(str(tmpdir), 'units.pkl'))


def check_final_inertia(dev, i):
    """against the float64 numpy Lloyd from the same init, gap allowed as ``inertia_gap_allowed`` derives it"""
    ref = lloyd_reference(i, 64)
    allowed, observed = inertia_gap_allowed(i)
    fit = fitted(dev, i)
    gap = abs(fit.inertia_ - ref['inertia']) / ref['inertia']
    print('d=%d K=%d N=%d: float64 Lloyd inertia %.12g in %d iterations (%d empty); fp32 numpy gap %.3g -> allowed %.3g; '
          'fit inertia %.12g in %d iterations (%d empty), gap %.3g'
          % (FIT_SHAPES[i] + (ref['inertia'], ref['n_iter'], ref['empty'], observed, allowed, fit.inertia_, fit.n_iter_,
                              int((fit.counts_ == 0).sum()), gap)))
    assert gap <= allowed, (gap, allowed)


# ---- (f) the float64 restatement against scikit-learn (CPU only, where it imports) --------------------------------------------------
def check_reference_against_sklearn(i):
    from sklearn.cluster import KMeans
    x, init = blobs(i)
    ref = lloyd_reference(i, 64)
    assert ref['empty'] == 0, 'scikit-learn relocates empty centroids: compare only where none occurs'
    km = KMeans(n_clusters=FIT_SHAPES[i][1], init=init.astype(np.float64), n_init=1, algorithm='lloyd', tol=TOL, max_iter=MAX_ITER)
    km.fit(x.astype(np.float64))
    assert np.array_equal(km.labels_, ref['labels'])
    assert abs(km.inertia_ - ref['inertia']) <= 1e-9 * ref['inertia']
    assert np.allclose(km.cluster_centers_, ref['centers'], rtol=0.0, atol=1e-9)


# ---- (g) the command-line tool ------------------------------------------------------------------------------------------------------
def check_tool(dev, tmpdir):
    """tools/fit_kmeans.py (in process) on the utterances of the model fixture: a seeded subsample of their frames, the fit of
    exactly those frames, and a file that ``KMeansVQGANEmb(quantizer_path=...)`` loads"""
    import importlib.util
    from _parity import json_field, load_npz
    from msmctts_amd.hip import kmeans
    from msmctts_amd.networks import find_modules
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('fit_kmeans_tool', os.path.join(root, 'tools', 'fit_kmeans.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    z = load_npz('small_kmeans.npz')
    emb, lengths = z['batch.emb'], [int(v) for v in z['batch.emb_length']]
    tmp = str(tmpdir)
    with open(os.path.join(tmp, 'train.list'), 'w') as f:
        for b, n in enumerate(lengths):
            np.save(os.path.join(tmp, 'utt%d_emb.npy' % b), emb[b, :n])
            f.write('utt%d emb\n' % b)
    ids, pattern, out = os.path.join(tmp, 'train.list'), os.path.join(tmp, '{0}_{1}.npy'), os.path.join(tmp, 'units.npy')
    K, M, d = 6, 40, emb.shape[2]
    fit = tool.main([ids, pattern, '--clusters', str(K), '--frames', str(M), '--seed', '3', '--iters', '5', '--device', dev, '-o', out])
    frames = tool.load_frames(ids, pattern, M, 3)
    every = np.concatenate([emb[b, :n] for b, n in enumerate(lengths)])
    assert frames.shape == (M, d) and frames.dtype == np.float32 and M < len(every)
    rows = [int(np.flatnonzero((every == f).all(1))[0]) for f in frames]
    assert rows == sorted(set(rows)), 'the subsample: distinct frames, in utterance order'
    assert tool.load_frames(ids, pattern).shape == every.shape and np.array_equal(tool.load_frames(ids, pattern), every)
    again = kmeans.fit_kmeans(frames, K, max_iter=5, seed=3, device=dev)
    centers = np.load(out)
    assert centers.shape == (K, d) and centers.dtype == np.float32
    assert np.array_equal(centers.view(np.int32), again.cluster_centers_.view(np.int32)) and fit.n_iter_ == again.n_iter_
    (_, m), = find_modules({'autoencoder': dict(json_field(z['cfg']), _name='KMeansVQGANEmb', quantizer_path=out)})
    assert torch.equal(m.quantizer.quantizer[0].embed, torch.from_numpy(centers).t())


# ---- (h) feature presence ----------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    for name in ('msmc_kmeans_stats_workspace', 'msmc_kmeans_stats', 'msmc_kmeans_update'):
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import fit_kmeans  # noqa: F401
