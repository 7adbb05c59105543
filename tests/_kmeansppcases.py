"""Shared cases of the k-means++ seeding on the gfx950 kernels (csrc/kmeans_pp.hip: msmc_kmeanspp_seed; msmctts_amd/hip/kmeans.py:
``kmeans_plusplus``, ``fit_kmeans(init='k-means++')``; tools/fit_kmeans.py ``--init k-means++``).  tests/test_kmeanspp_emu.py runs
them on the kernel interpreter, tests/test_gpu_kmeanspp.py on the GPU.

Reference.  ``restated_seeding`` is the documented order of the kernels in numpy and must match BIT FOR BIT (both builds compile
with -ffp-contract=off): distances in fp32 as the direct difference -- lane l of 64 adds (x - c)^2 of the 4-channel pieces l,
l + 64, ... in ascending channel order from +0, then the butterfly v = v + v[lane ^ m], m = 1, 2, 4, 8, 16, 32 --, the minimum
with mind, and in float64 per tile of 256 frames the running sum from +0 in ascending n (``np.cumsum``: sequential), the tile
prefixes pre[t + 1] = pre[t] + (the last running sum of tile t), cum = pre[t] + running sum, total = pot = pre[T].  Candidate
= first n with cum[n] > u * total (N - 1 for total == 0), winner = first minimum of pot.  The restatement asserts the two
invariants of cum on the way: it never decreases and ends at total bit for bit.

Its float64 twin (``dtype=np.float64``: the same frames, every distance in float64) must pick the same frames.  A near-tie between
two candidates' potentials that flips under fp32 would be a property of the input, not a kernel fault, so the case seeds below
were chosen on the CPU such that the twin agrees (every seed tried did: 5400 + s for case s, N(0, 1) frames; relative gaps
between candidate potentials are around 1e-3 there, fp32 distance errors around 1e-7).
"""
import concurrent.futures
import ctypes
import functools
import os

import numpy as np
import torch

from _vqstreamcases import E_SHAPE, _raises, same_bits
import _kmeansfitcases as fitcases

E_WORKSPACE = -3
TILE = 256                                                  # KPP_TILE of csrc/kmeans_pp.hip
ONE_MINUS = 1.0 - 2.0 ** -53                                # the largest float64 below 1
_POOL = concurrent.futures.ThreadPoolExecutor(6)            # (the restatement of the largest case is 600 passes over 12 MB)

# d, N, K, L
SHAPES = ((4, 1, 1, 1), (16, 257, 5, 3), (272, 1500, 24, 5), (64, 1031, 3, 16), (1024, 3000, 100, 6), (2048, 300, 7, 3),
          (768, 300, 8, 1), (1024, 600, 8, 3))
IDS = ['d%d N%d K%d L%d' % s for s in SHAPES]
GPU_CASES = (0, 1, 2, 3, 4, 5, 6)
EMU_CASES = (0, 1, 2, 3, 7, 5, 6)                           # (1024, 3000, 100, 6) takes minutes on the interpreter


def draws(seed, N, K, L):
    """first and uniforms as ``kmeans_plusplus(seed=...)`` draws them"""
    gen = torch.Generator().manual_seed(seed)
    first = int(torch.randint(N, (1,), generator=gen))
    return first, torch.rand(max(K - 1, 0), L, dtype=torch.float64, generator=gen)


@functools.lru_cache(maxsize=None)
def problem(s):
    """seeded N(0, 1) frames [N, d] (distinct rows) -> (x host tensor, first, uniforms [K - 1, L] float64); never modified"""
    d, N, K, L = SHAPES[s]
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(5400 + s)).contiguous()
    first, u = draws(5400 + s, N, K, L)
    return x, first, u


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def restated_distances(x, c):
    """|x[n] - c[j]|^2 [L, N] in the order of kpp_dist_kernel, in the dtype of x"""
    N, d = x.shape
    L, dv, lanes = c.shape[0], d // 4, np.arange(64)
    out = np.empty((L, N), dtype=x.dtype)

    def slab(n0):                                           # (slabs: the [n, L, d] differences stay small; numpy drops the GIL)
        df = x[n0:n0 + 512, None, :] - c[None, :, :]
        sq = (df * df).reshape(df.shape[0], L, dv, 4)
        v = np.zeros((df.shape[0], L, 64), dtype=x.dtype)
        for q0 in range(0, dv, 64):
            w = min(64, dv - q0)
            for k in range(4):
                v[:, :, :w] = v[:, :, :w] + sq[:, :, q0:q0 + w, k]
        for m in (1, 2, 4, 8, 16, 32):
            v = v + v[:, :, lanes ^ m]
        out[:, n0:n0 + 512] = v[:, :, 0].T

    list(_POOL.map(slab, range(0, N, 512)))
    return out


def float64_distances(x, c):
    """the twin's distances [L, N]: float64 throughout, in no particular order (a candidate's differences at a time)"""
    return np.stack(list(_POOL.map(lambda cj: ((x - cj) ** 2).sum(1), c)))


def running_sum(m):
    """-> (cum [N] float64, total) of the minima m [N] in the documented order; asserts the two invariants of cum"""
    m = m.astype(np.float64)
    cum, pre = np.empty(len(m)), 0.0
    for n0 in range(0, len(m), TILE):
        local = np.cumsum(m[n0:n0 + TILE])
        cum[n0:n0 + TILE] = pre + local
        pre = pre + local[-1]
    assert cum[-1] == pre and bool((np.diff(cum) >= 0).all())
    return cum, pre


def restated_seeding(x, K, L, first, u, dtype=np.float32):
    """-> (chosen [K] int64, potential [K] float64, candidates [K - 1, L]) in the order of msmc_kmeanspp_seed"""
    x = np.asarray(x, dtype=dtype)
    u = np.asarray(u, dtype=np.float64).reshape(max(K - 1, 0), L)
    N = x.shape[0]
    dist = restated_distances if dtype == np.float32 else float64_distances
    mind = dist(x, x[[first]])[0]
    cum, total = running_sum(mind)
    chosen, potential, cands = [first], [total], []
    for i in range(1, K):
        cand = []
        for j in range(L):
            n = N - 1
            if total > 0:
                n = min(int(np.searchsorted(cum, u[i - 1, j] * total, side='right')), N - 1)
            cand.append(n)
        dj = dist(x, x[cand])
        mins = np.where(mind[None, :] < dj, mind[None, :], dj)
        runs = [running_sum(mins[j]) for j in range(L)]
        best = int(np.argmin([r[1] for r in runs]))         # (the first of equal minima)
        mind, (cum, total) = mins[best], runs[best]
        chosen.append(cand[best])
        potential.append(total)
        cands.append(cand)
    return np.array(chosen, dtype=np.int64), np.array(potential, dtype=np.float64), np.array(cands, dtype=np.int64).reshape(-1, L)


@functools.lru_cache(maxsize=None)
def reference(s):
    """the restatement of case s, checked against its float64 twin; computed once, never modified"""
    d, N, K, L = SHAPES[s]
    x, first, u = problem(s)
    chosen, potential, cands = restated_seeding(x.numpy(), K, L, first, u.numpy())
    twin, pot64, _ = restated_seeding(x.numpy(), K, L, first, u.numpy(), dtype=np.float64)
    assert np.array_equal(chosen, twin), 'case %d: the float64 twin picks other frames -- choose another seed' % s
    assert np.allclose(potential, pot64, rtol=1e-5, atol=0.0)
    return chosen, potential


# ---- the launcher, directly ---------------------------------------------------------------------------------------------------------
def run_seed(dev, x, K, L, first, u, N=None, extra_rows=0, ws_bytes=None, ws_extra=64, x_offset=0):
    """msmc_kmeanspp_seed directly -> (rc, centers, chosen, potential, workspace as bytes, bytes the library asked for).  The
    outputs are ``extra_rows`` longer than K and the workspace ``ws_extra`` bytes longer than asked for, all guard-filled;
    ``x_offset``: floats by which the frames' pointer is moved off its alignment"""
    from msmctts_amd.hip import lib
    lb = lib.get()
    d = x.shape[1]
    N = x.shape[0] if N is None else N
    rows = max(K, 0) + extra_rows
    xd = torch.cat([torch.zeros(x_offset), x.reshape(-1)]).to(dev)[x_offset:] if x_offset else x.to(dev)
    ud = (u if u.numel() else torch.zeros(1, dtype=torch.float64)).to(dev).contiguous()
    centers = torch.full((rows, d), float('nan')).to(dev)
    chosen = torch.full((rows,), -7, dtype=torch.int64).to(dev)
    potential = torch.full((rows,), -7.0, dtype=torch.float64).to(dev)
    need = int(lb.msmc_kmeanspp_workspace(N, d, K, L))
    have = int(lb.msmc_kmeanspp_workspace(max(1, min(N, x.shape[0])), d, max(K, 1), min(max(L, 1), 16)))
    ws = torch.full((have + ws_extra,), 0x5a, dtype=torch.uint8).to(dev)
    rc = lb.msmc_kmeanspp_seed(lib.ptr(xd), N, d, K, L, first, lib.ptr(ud),
                               lib.ptr(centers), lib.ptr(chosen), lib.ptr(potential), lib.ptr(ws),
                               need if ws_bytes is None else ws_bytes, lib.stream(centers))
    if centers.is_cuda:
        torch.cuda.synchronize()
    return rc, centers.cpu(), chosen.cpu(), potential.cpu(), ws.cpu(), have


def intact(centers, chosen, potential, ws):
    return bool(torch.isnan(centers).all()) and bool((chosen == -7).all()) and bool((potential == -7).all()) and bool((ws == 0x5a).all())


def same_bits64(a, b):
    return torch.equal(torch.as_tensor(a).contiguous().view(torch.int64), torch.as_tensor(b).contiguous().view(torch.int64))


@functools.lru_cache(maxsize=None)
def seeded(dev, s):
    """the direct call the tests of case s share (guarded buffers); never modified"""
    d, N, K, L = SHAPES[s]
    x, first, u = problem(s)
    return run_seed(dev, x, K, L, first, u, extra_rows=3)


# ---- 1, 3: bit-exact restatement, no repeats ------------------------------------------------------------------------------------------
def check_shape(dev, s):
    d, N, K, L = SHAPES[s]
    x, first, u = problem(s)
    want_c, want_p = reference(s)
    rc, centers, chosen, potential, _, _ = seeded(dev, s)
    assert rc == 0, rc
    chosen, potential, centers = chosen[:K], potential[:K], centers[:K]
    print('%s: chosen %s ... potential %.9g -> %.9g' % (IDS[s], chosen[:6].tolist(), float(potential[0]), float(potential[-1])))
    assert np.array_equal(chosen.numpy(), want_c), (chosen.tolist(), want_c.tolist())
    assert same_bits64(potential, torch.from_numpy(want_p)), (potential.tolist(), want_p.tolist())
    assert same_bits(centers, x[chosen]), 'centers are not the chosen rows'
    assert int(chosen[0]) == first and bool((chosen >= 0).all()) and bool((chosen < N).all())
    if K <= N:
        assert len(set(chosen.tolist())) == K, 'a frame was chosen twice although the frames are distinct'
    assert bool((np.diff(potential.numpy()) <= 0).all()), 'the potential went up'


# ---- 2: edge uniforms -----------------------------------------------------------------------------------------------------------------
def check_edge_uniforms(dev):
    s = 1
    d, N, K, L = SHAPES[s]
    x, _, _ = problem(s)
    for first, value in ((3, 0.0), (0, 0.0), (N - 1, 0.0), (5, ONE_MINUS), (N - 1, ONE_MINUS)):
        u = torch.full((K - 1, L), value, dtype=torch.float64)
        rc, centers, chosen, potential, _, _ = run_seed(dev, x, K, L, first, u)
        assert rc == 0
        want_c, want_p, _ = restated_seeding(x.numpy(), K, L, first, u.numpy())
        assert np.array_equal(chosen.numpy(), want_c) and same_bits64(potential, torch.from_numpy(want_p)), (first, value)
        got = chosen.tolist()
        assert got[0] == first and len(set(got)) == K and all(0 <= n < N for n in got), got
        if value == 0.0:                                    # the first frame of non-zero weight: the lowest not chosen yet
            for i in range(1, K):
                assert got[i] == min(set(range(N)) - set(got[:i])), got
        assert same_bits(centers, x[chosen])


# ---- 4: duplicates ----------------------------------------------------------------------------------------------------------------------
def check_duplicates(dev):
    """three distinct rows repeated to N = 200, K = 5: terminates, in range, the three rows first, then potential 0"""
    d, N, K, L = 16, 200, 5, 3
    gen = torch.Generator().manual_seed(5480)
    rows = torch.randn(3, d, generator=gen)
    x = rows[torch.randint(0, 3, (N,), generator=gen)].contiguous()
    first, u = draws(5480, N, K, L)
    rc, centers, chosen, potential, _, _ = run_seed(dev, x, K, L, first, u)
    assert rc == 0
    assert bool((chosen >= 0).all()) and bool((chosen < N).all())
    assert sorted(map(tuple, centers[:3].tolist())) == sorted(map(tuple, rows.tolist())), 'the first three centres: the three distinct rows'
    assert potential[2:].tolist() == [0.0, 0.0, 0.0] and float(potential[1]) > 0
    assert chosen[3:].tolist() == [N - 1, N - 1], 'total == 0 picks frame N - 1'
    want_c, want_p, _ = restated_seeding(x.numpy(), K, L, first, u.numpy())
    assert np.array_equal(chosen.numpy(), want_c) and same_bits64(potential, torch.from_numpy(want_p))
    assert same_bits(centers, x[chosen])
    # more centres than frames
    x3 = torch.randn(3, d, generator=gen)
    first, u = draws(5481, 3, K, L)
    rc, centers, chosen, potential, _, _ = run_seed(dev, x3, K, L, first, u)
    assert rc == 0 and sorted(chosen[:3].tolist()) == [0, 1, 2] and chosen[3:].tolist() == [2, 2]
    assert potential[2:].tolist() == [0.0, 0.0, 0.0] and same_bits(centers, x3[chosen])


# ---- 5: determinism ---------------------------------------------------------------------------------------------------------------------
def check_determinism(dev, s):
    """two calls: the same bits; the ``seed`` path of ``kmeans_plusplus``: the explicit ``first`` / ``uniforms`` path; rows beyond
    K and workspace beyond the queried size: untouched"""
    from msmctts_amd.hip import kmeans
    d, N, K, L = SHAPES[s]
    x, first, u = problem(s)
    rc, centers, chosen, potential, ws, have = seeded(dev, s)
    assert rc == 0
    assert bool(torch.isnan(centers[K:]).all()) and bool((chosen[K:] == -7).all()) and bool((potential[K:] == -7).all())
    assert have > 0 and ws.numel() == have + 64 and bool((ws[have:] == 0x5a).all()), 'the workspace was written beyond its size'
    rc2, centers2, chosen2, potential2, _, _ = run_seed(dev, x, K, L, first, u)
    assert rc2 == 0 and same_bits(centers2, centers[:K]) and torch.equal(chosen2, chosen[:K]) and same_bits64(potential2, potential[:K])
    by_seed = kmeans.kmeans_plusplus(x, K, seed=5400 + s, n_local_trials=L, device=dev)
    explicit = kmeans.kmeans_plusplus(x.to(dev), K, seed=1, n_local_trials=L, first=first, uniforms=u, device=dev)
    for got in (by_seed, explicit):
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.float64
        assert same_bits(got[0].cpu(), centers[:K]) and torch.equal(got[1].cpu(), chosen[:K]) and same_bits64(got[2].cpu(), potential[:K])


def check_default_local_trials():
    from msmctts_amd.hip import kmeans
    assert [kmeans.default_local_trials(K) for K in (1, 2, 8, 100, 500, 2000, 10 ** 7)] == [2, 2, 4, 6, 8, 9, 16]


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    """d = 6, d = 2052, L = 0, L = 17, first = N, first = -1, K = 0, N = 0, a misaligned x: MSMC_E_SHAPE; a workspace one byte
    short: MSMC_E_WORKSPACE; every buffer keeps its guard values"""
    from msmctts_amd.hip import kmeans, lib
    gen = torch.Generator().manual_seed(5490)
    N = 9
    for d, K, L, first in ((6, 3, 2, 0), (2052, 3, 2, 0), (16, 3, 0, 0), (16, 3, 17, 0), (16, 3, 2, N), (16, 3, 2, -1), (16, 0, 2, 0)):
        x = torch.randn(N, d, generator=gen)
        u = torch.rand(max(K - 1, 1), min(max(L, 1), 16), dtype=torch.float64, generator=gen)
        rc, centers, chosen, potential, ws, _ = run_seed(dev, x, K, L, first, u, extra_rows=4)
        assert rc == E_SHAPE and intact(centers, chosen, potential, ws), (d, K, L, first, rc)
    for d, K, L in ((6, 3, 2), (2052, 3, 2), (16, 3, 0), (16, 3, 17), (16, 0, 2)):
        assert int(lib.get().msmc_kmeanspp_workspace(N, d, K, L)) == 0
    assert int(lib.get().msmc_kmeanspp_workspace(0, 16, 3, 2)) == 0
    x, u = torch.randn(N, 16, generator=gen), torch.rand(2, 2, dtype=torch.float64, generator=gen)
    rc, centers, chosen, potential, ws, _ = run_seed(dev, x, 3, 2, 0, u, N=0, extra_rows=4)
    assert rc == E_SHAPE and intact(centers, chosen, potential, ws)
    rc, centers, chosen, potential, ws, _ = run_seed(dev, x, 3, 2, 0, u, extra_rows=4, x_offset=1)
    assert rc == E_SHAPE and intact(centers, chosen, potential, ws), 'a misaligned x'
    # a workspace one byte short
    s = 1
    d, N, K, L = SHAPES[s]
    x, first, u = problem(s)
    need = int(lib.get().msmc_kmeanspp_workspace(N, d, K, L))
    assert need >= 8 * L * N
    rc, centers, chosen, potential, ws, _ = run_seed(dev, x, K, L, first, u, extra_rows=4, ws_bytes=need - 1)
    assert rc == E_WORKSPACE and intact(centers, chosen, potential, ws), rc
    # the wrapper raises with the launcher's code
    with _raises(RuntimeError, 'msmc_kmeanspp_seed failed with code -2'):
        kmeans.kmeans_plusplus(torch.zeros(9, 6), 3, device=dev)
    with _raises(RuntimeError, 'msmc_kmeanspp_seed failed with code -2'):
        kmeans.kmeans_plusplus(torch.zeros(9, 16), 3, n_local_trials=17, device=dev)
    with _raises(ValueError, 'uniforms: expected'):
        kmeans.kmeans_plusplus(torch.zeros(9, 16), 3, n_local_trials=2, uniforms=torch.zeros(3, 2, dtype=torch.float64), device=dev)


# ---- 7: through fit_kmeans --------------------------------------------------------------------------------------------------------------
def check_fit(dev, i):
    from msmctts_amd.hip import kmeans
    d, K, N = fitcases.FIT_SHAPES[i]
    x, init = fitcases.blobs(i)
    kw = dict(max_iter=fitcases.MAX_ITER, tol=fitcases.TOL, device=dev)
    fit = kmeans.fit_kmeans(x, K, init='k-means++', seed=fitcases.FIT_SEED, **kw)
    centers, chosen, _ = kmeans.kmeans_plusplus(x, K, seed=fitcases.FIT_SEED, device=dev)
    chosen = chosen.cpu().numpy()
    assert np.array_equal(fit.init_indices_, chosen) and fit.init_indices_.dtype == np.int64
    assert same_bits(centers.cpu(), torch.from_numpy(x[chosen]))
    by_array = kmeans.fit_kmeans(x, K, init=x[chosen], **kw)
    assert fitcases.same_fit(fit, by_array), "init='k-means++' is not the fit from x[chosen]"
    assert by_array.init_indices_ is None
    on_device = kmeans.fit_kmeans(torch.from_numpy(x).to(dev), K, init='k-means++', seed=fitcases.FIT_SEED, **kw)
    assert fitcases.same_fit(fit, on_device) and np.array_equal(on_device.init_indices_, chosen)
    print('%s: k-means++ init: inertia %.9g in %d iterations, %d empty; uniform init: inertia %.9g in %d iterations, %d empty' % (
        fitcases.FIT_IDS[i], fit.inertia_, fit.n_iter_, int((fit.counts_ == 0).sum()), fitcases.fitted(dev, i).inertia_,
        fitcases.fitted(dev, i).n_iter_, int((fitcases.fitted(dev, i).counts_ == 0).sum())))


def check_fit_seeds_from_a_sample(dev, i):
    """host frames, ``seed_frames`` < N: one upload of the sampled rows, seeded over them alone; ``init_indices_`` index ``frames``"""
    from msmctts_amd.hip import kmeans
    d, K, N = fitcases.FIT_SHAPES[i]
    x, _ = fitcases.blobs(i)
    M = N // 2
    rows = np.sort(torch.randperm(N, generator=torch.Generator().manual_seed(11))[:M].numpy())
    fit = kmeans.fit_kmeans(x, K, init='k-means++', seed=11, seed_frames=M, max_iter=3, device=dev)
    assert fit.init_indices_.shape == (K,) and set(fit.init_indices_.tolist()) <= set(rows.tolist())
    centers, chosen, _ = kmeans.kmeans_plusplus(x[rows], K, seed=11, device=dev)
    assert np.array_equal(fit.init_indices_, rows[chosen.cpu().numpy()])
    assert same_bits(centers.cpu(), torch.from_numpy(x[fit.init_indices_]))
    assert fitcases.same_fit(fit, kmeans.fit_kmeans(x, K, init=x[fit.init_indices_], max_iter=3, device=dev))


def check_fit_without_seeding_is_unchanged(dev, i):
    from msmctts_amd.hip import kmeans
    d, K, N = fitcases.FIT_SHAPES[i]
    x, init = fitcases.blobs(i)
    fit = kmeans.fit_kmeans(x, K, max_iter=fitcases.MAX_ITER, tol=fitcases.TOL, seed=fitcases.FIT_SEED, device=dev)
    assert fitcases.same_fit(fit, fitcases.fitted(dev, i)), 'init=None changed'
    assert same_bits(torch.from_numpy(x[fit.init_indices_]), torch.from_numpy(init)) and fitcases.fitted(dev, i).init_indices_ is None
    with _raises(ValueError, "None or 'k-means++'"):
        kmeans.fit_kmeans(x, K, init='nonsense', device=dev)


# ---- 8: the command-line tool -------------------------------------------------------------------------------------------------------------
def check_tool(dev, tmpdir):
    """tools/fit_kmeans.py --init k-means++ (in process) on the utterances of the model fixture: the fit of the same frames with
    ``init='k-means++'``, and a file ``KMeansQuantizer`` loads"""
    import importlib.util
    from _parity import load_npz
    from msmctts_amd.hip import kmeans
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansQuantizer, kmeans_plusplus
    assert kmeans_plusplus is kmeans.kmeans_plusplus
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
    fit = tool.main([ids, pattern, '--clusters', str(K), '--frames', str(M), '--seed', '3', '--iters', '5', '--device', dev,
                     '--init', 'k-means++', '--local-trials', '2', '-o', out])
    frames = tool.load_frames(ids, pattern, M, 3)
    again = kmeans.fit_kmeans(frames, K, max_iter=5, seed=3, init='k-means++', n_local_trials=2, device=dev)
    centers = np.load(out)
    assert centers.shape == (K, d) and centers.dtype == np.float32
    assert np.array_equal(centers.view(np.int32), again.cluster_centers_.view(np.int32)) and fit.n_iter_ == again.n_iter_
    assert np.array_equal(fit.init_indices_, again.init_indices_) and len(set(fit.init_indices_.tolist())) == K
    q = KMeansQuantizer(out).to(dev).eval()
    with torch.no_grad():
        got = q([(torch.from_numpy(frames).view(1, M, d).to(dev), torch.tensor([M]).to(dev))])
    assert np.array_equal(got['quantizer_indices'][0].reshape(-1).cpu().numpy(), fit.labels_)
    # the default stays the uniform draw
    plain = tool.main([ids, pattern, '--clusters', str(K), '--frames', str(M), '--seed', '3', '--iters', '5', '--device', dev, '-o', out])
    assert fitcases.same_fit(plain, kmeans.fit_kmeans(frames, K, max_iter=5, seed=3, device=dev))


# ---- 9: the float64 restatement against scikit-learn (CPU only, where it imports) -------------------------------------------------------
def check_reference_against_sklearn():
    """blob case 1, 32 seeds each: the mean log seeding potential of the float64 restatement and of
    ``sklearn.cluster.kmeans_plusplus`` agree within three standard errors of the difference (the two consume their random
    numbers differently: only the distributions can be compared)"""
    from sklearn.cluster import kmeans_plusplus
    from msmctts_amd.hip import kmeans
    d, K, N = fitcases.FIT_SHAPES[1]
    x = fitcases.blobs(1)[0].astype(np.float64)
    L = kmeans.default_local_trials(K)
    ours, theirs = [], []
    for seed in range(32):
        first, u = draws(seed, N, K, L)
        ours.append(np.log(restated_seeding(x, K, L, first, u.numpy(), dtype=np.float64)[1][-1]))
        c, _ = kmeans_plusplus(x, K, random_state=seed)
        theirs.append(np.log(float64_distances(x, c).min(0).sum()))
    ours, theirs = np.array(ours), np.array(theirs)
    se = np.sqrt(ours.var(ddof=1) / len(ours) + theirs.var(ddof=1) / len(theirs))
    print('mean log potential: restatement %.6f (sd %.4f), scikit-learn %.6f (sd %.4f), difference %.4f = %.2f standard errors' % (
        ours.mean(), ours.std(ddof=1), theirs.mean(), theirs.std(ddof=1), ours.mean() - theirs.mean(), (ours.mean() - theirs.mean()) / se))
    assert abs(ours.mean() - theirs.mean()) <= 3.0 * se


# ---- feature presence ---------------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import kmeans, lib
    for name in ('msmc_kmeanspp_workspace', 'msmc_kmeanspp_seed'):
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
    assert callable(kmeans.kmeans_plusplus)
