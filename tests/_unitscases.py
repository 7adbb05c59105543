"""Shared cases of unit extraction: the labels-only wide assignment (csrc/vq_assign.inc, msmc_vq_assign_wide), run collapse and
code usage (csrc/units.hip, msmc_units_collapse / msmc_units_usage), their host side (msmctts_amd/hip/units.py),
``KMeansQuantizer.units`` and tools/extract_units.py.  tests/test_units_emu.py runs them on the kernel interpreter,
tests/test_gpu_units.py on the GPU.

References.
* Labels: ``msmc_vq_search_wide`` on the same inputs, BIT FOR BIT, in every instantiation (``msmc_vq_wide_set_split`` 0 / 1 / 2 /
  4) -- the shipped kernel pins the new one -- and float64 under the near-tie rule of tests/_vqstreamcases.py (``MAX_LEFT_OUT``,
  a cap asserted on the reference alone) with the inputs of tests/_kmeanscases.py (``problem`` / ``reference_of``: the generator
  for which the float64 reference stays inside that cap at these widths; N(0, 1) frames alone do not, see its docstring).
* Distance: ``restated_dist`` is the documented order in numpy (include/msmc_hip.h: piece c4 of the row to partial c4 % 16,
  every partial in ascending piece and channel order from +0, the 16 partials added in order from +0) and must match BIT FOR
  BIT; against float64 ``sum (x - e)^2`` the bound is the one tests/_kmeansppcases.py holds the fp32 distances of the same
  convention to: ``np.allclose(fp32, float64, rtol=1e-5, atol=0.0)``.
* Collapse / usage: ``restated_collapse`` and ``np.bincount``; exact.
"""
import contextlib
import ctypes
import functools
import importlib.util
import io
import os

import numpy as np
import torch

import _kmeanscases as kc
from _kmeanscases import SPLITS, forced_split
from _vqstreamcases import E_SHAPE, MAX_LEFT_OUT, _raises, last_kernel, same_bits

ASSIGN = 'vq_assign_wide_kernel'
# d, K: a K tail inside a centroid tile, d that is no multiple of the 32-channel slice, K = 1, the 16-row prepare tile (d > 1279)
SHAPES = ((1024, 100), (768, 500), (1040, 17), (272, 24), (64, 1), (2048, 40))
IDS = ['d%d K%d' % s for s in SHAPES]
FRAMES = (256, 37)
# Seeds are those of tests/_kmeanscases.py (4800 + its shape number: its cached problems and references are shared).  At N = 37
# the cap of 2 % allows no undecided frame at all; d = 1024, K = 100 with seed 4800 has one among its nine N(0, 1) frames, so
# that case draws from 5800 -- chosen on the float64 reference alone, before any kernel ran.
SEED_OVERRIDE = {(0, 37): 5800}
GUARD_I, EXTRA = -7, 70


def _problem(s, N):
    """the frames, centroids and float64 decision of tests/_kmeanscases.py for shape s (shared, cached there, never modified)"""
    d, K = SHAPES[s]
    seed = SEED_OVERRIDE.get((s, N), 4800 + kc.WIDE_SHAPES.index((d, K)))
    x, embed = kc.problem(d, K, N, seed)
    return x, embed, kc.reference_of(d, K, N, seed)


def assign(dev, x, embed, N=None, want_dist=True, extra_rows=0, x_offset=0):
    """msmc_vq_assign_wide directly -> (rc, ind [rows], dist [rows] or None) on the host; the outputs are ``extra_rows`` longer
    than N (GUARD_I / NaN filled); ``x_offset``: x starts that many floats into its buffer"""
    from msmctts_amd.hip import lib, vq
    _, d, K = embed.shape
    N = x.shape[0] if N is None else N
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    buf = torch.zeros(x.numel() + 4).to(dev)
    xd = buf[x_offset:x_offset + x.numel()].view(x.shape)
    xd.copy_(x)
    rows = max(N, 0) + extra_rows
    ind = torch.full((rows,), GUARD_I, dtype=torch.int64).to(dev)
    dist = torch.full((rows,), float('nan')).to(dev) if want_dist else None
    rc = lib.get().msmc_vq_assign_wide(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(ind), lib.ptr(dist), N, d, K, lib.stream(xd))
    return rc, ind.cpu(), None if dist is None else dist.cpu()


def restated_dist(x, rows):
    """the documented summation order of dist in numpy fp32: x [N, d] frames, rows [N, d] the winners' rows"""
    x, rows = np.asarray(x, dtype=np.float32), np.asarray(rows, dtype=np.float32)
    N, d = x.shape
    df = x - rows
    sq = (df * df).reshape(N, d // 4, 4)
    part = np.zeros((N, 16), dtype=np.float32)
    for c0 in range(0, d // 4, 16):
        w = min(16, d // 4 - c0)
        for jj in range(4):
            part[:, :w] = part[:, :w] + sq[:, c0:c0 + w, jj]
    total = np.zeros(N, dtype=np.float32)
    for p in range(16):
        total = total + part[:, p]
    return total


def check_dist(x, embed, ind, dist, what):
    rows = embed[0].t()[ind]
    want = restated_dist(x.numpy(), rows.numpy())
    assert same_bits(dist, torch.from_numpy(want)), '%s: dist is not the documented sum, first %s' % (
        what, (dist != torch.from_numpy(want)).nonzero()[:4].flatten().tolist())
    want64 = ((x.double() - rows.double()) ** 2).sum(-1).numpy()
    assert np.allclose(dist.numpy(), want64, rtol=1e-5, atol=0.0), '%s: dist against float64, worst relative %.3g' % (
        what, float(np.max(np.abs(dist.numpy() - want64) / np.maximum(want64, 1e-300))))


# ---- (a) labels: the wide search's, and float64's; dist: the documented sum ---------------------------------------------------------
def check_labels_and_dist(dev, s, N, splits=SPLITS):
    x, embed, (want, decided) = _problem(s, N)
    left_out = 1.0 - decided.double().mean().item()
    print('assign d=%d K=%d N=%d: the float64 reference leaves %.4f of the frames undecided' % (SHAPES[s] + (N, left_out)))
    assert left_out <= MAX_LEFT_OUT, 'the float64 reference leaves %.3f of the frames undecided' % left_out
    K = embed.shape[2]
    dists = []
    for wc in splits:
        with forced_split(wc):
            rc, _, _, i0 = kc.search(dev, x, embed)
            assert rc == 0 and last_kernel() == kc.WIDE, (wc, rc, last_kernel())
            rc, ind, dist = assign(dev, x, embed, extra_rows=EXTRA)
            assert rc == 0 and last_kernel() == ASSIGN, (wc, rc, last_kernel())
        assert bool((ind[N:] == GUARD_I).all()) and bool(torch.isnan(dist[N:]).all()), 'split %d: rows beyond N were written' % wc
        ind, dist = ind[:N], dist[:N]
        assert torch.equal(ind, i0[:, 0]), 'split %d: labels differ from msmc_vq_search_wide on %d frames' % (wc, int((ind != i0[:, 0]).sum()))
        assert int(ind.min()) >= 0 and int(ind.max()) < K
        wrong = (ind != want) & decided
        assert not bool(wrong.any()), 'split %d: label differs from float64 on %d decided frames' % (wc, int(wrong.sum()))
        check_dist(x, embed, ind, dist, 'split %d' % wc)
        dists.append(dist)
    assert all(same_bits(dists[0], other) for other in dists[1:]), 'dist depends on the split'


# ---- (b) exact zeros, ties ------------------------------------------------------------------------------------------------------------
def check_exact_zeros(dev):
    """a frame that is a copy of a centroid gets that centroid and weighs exactly 0 (the expanded form would leave rounding noise)"""
    for d, K, N in ((1024, 100, 48), (272, 24, 37)):
        embed = kc.problem(d, K, 16, 4800 + kc.WIDE_SHAPES.index((d, K)))[1]
        which = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(5900 + d))
        x = embed[0][:, which].t().contiguous()
        for wc in SPLITS:
            with forced_split(wc):
                rc, ind, dist = assign(dev, x, embed)
            assert rc == 0 and torch.equal(ind, which), (d, wc)
            assert bool((dist == 0).all()) and not bool(torch.signbit(dist).any()), (d, wc, dist.tolist())


def check_ties(dev):
    """identical centroid rows -- next to each other, in other tiles of every instantiation, in the partial last tile: the
    lowest index wins (the copies are the same bits, so a frame is at exactly the same fp32 distance from all of them)"""
    d, K, N = 64, 600, 48
    gen = torch.Generator().manual_seed(5910)
    embed = torch.randn(1, d, K, generator=gen)
    for k in (6, 69, 261, 330, K - 1):
        embed[0, :, k] = embed[0, :, 5]
    embed[0, :, 64] = embed[0, :, 63]
    embed[0, :, 256] = embed[0, :, 255]
    which = torch.tensor([5, 63, 255] * (N // 3))
    x = (embed[0][:, which].t() + 1e-3 * torch.randn(N, d, generator=gen)).contiguous()
    for wc in SPLITS:
        with forced_split(wc):
            rc, ind, dist = assign(dev, x, embed)
        assert rc == 0 and torch.equal(ind, which), (wc, ind.tolist())
        check_dist(x, embed, ind, dist, 'ties, split %d' % wc)


# ---- (c) dist = NULL -------------------------------------------------------------------------------------------------------------------
def check_null_distance(dev):
    """without a distance buffer the labels are the same and nothing but ind [N] is written: ind sits between guard rows"""
    from msmctts_amd.hip import lib, vq
    s, N, G = 3, 37, 64
    x, embed, _ = _problem(s, N)
    d, K = SHAPES[s]
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    xd = x.clone().to(dev)
    for wc in SPLITS:
        with forced_split(wc):
            rc, want, _ = assign(dev, x, embed)
            buf = torch.full((G + N + G,), GUARD_I, dtype=torch.int64).to(dev)
            ind = buf[G:G + N]
            rc2 = lib.get().msmc_vq_assign_wide(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(ind), None, N, d, K, lib.stream(xd))
        assert rc == 0 and rc2 == 0, (wc, rc, rc2)
        got = buf.cpu()
        assert torch.equal(got[G:G + N], want), wc
        assert bool((got[:G] == GUARD_I).all()) and bool((got[G + N:] == GUARD_I).all()), wc
        assert same_bits(xd.cpu(), x), 'x was written'


# ---- (d) refusals -----------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    from msmctts_amd.hip import lib, vq
    gen = torch.Generator().manual_seed(5920)

    def untouched(ind, dist):
        return bool((ind.cpu() == GUARD_I).all()) and bool(torch.isnan(dist.cpu()).all())

    for d, K, N in ((40, 24, 5), (2064, 24, 5), (64, 0, 5), (64, 24, -1)):
        # (a refused call reads nothing: plain buffers of the operands' sizes -- msmc_vq_prepare itself does not take d = 2064)
        xd = torch.randn(5, d, generator=gen).to(dev)
        et, en = torch.randn(max(K, 1), d, generator=gen).to(dev), torch.ones(max(K, 1)).to(dev)
        ind, dist = torch.full((5,), GUARD_I, dtype=torch.int64).to(dev), torch.full((5,), float('nan')).to(dev)
        rc = lib.get().msmc_vq_assign_wide(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(ind), lib.ptr(dist), N, d, K, lib.stream(xd))
        assert rc == E_SHAPE and untouched(ind, dist), (d, K, N, rc)
    x, embed = kc.problem(64, 1, kc.WIDE_N, 4805)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    guard = torch.full((2, 64), 7.0).to(dev)
    ind, dist = torch.full((2,), GUARD_I, dtype=torch.int64).to(dev), torch.full((2,), float('nan')).to(dev)
    L = lib.get()
    # N * d * 4 >= 2^32 is refused before anything is read (the pointers are never touched)
    rc = L.msmc_vq_assign_wide(lib.ptr(guard), lib.ptr(et), lib.ptr(en), lib.ptr(ind), lib.ptr(dist), 1 << 24, 64, 1, lib.stream(guard))
    assert rc == E_SHAPE and untouched(ind, dist), rc
    # N = 0: returns 0, nothing written
    rc = L.msmc_vq_assign_wide(lib.ptr(guard), lib.ptr(et), lib.ptr(en), lib.ptr(ind), lib.ptr(dist), 0, 64, 1, lib.stream(guard))
    assert rc == 0 and untouched(ind, dist) and bool((guard.cpu() == 7).all()), rc
    # x four bytes off a 16-byte boundary
    rc, ind, dist = assign(dev, x[:5], embed, extra_rows=0, x_offset=1)
    assert rc == E_SHAPE and untouched(ind, dist), rc
    rc, ind, dist = assign(dev, x[:5], embed, x_offset=4)             # (the same buffer, 16 bytes in: taken)
    assert rc == 0 and bool((ind == 0).all())
    # the wrapper raises with the launcher's code
    et, en = vq.vq_prepare(torch.randn(1, 40, 24, generator=gen).to(dev), frames=0)
    from msmctts_amd.hip import units
    with _raises(RuntimeError, 'msmc_vq_assign_wide failed with code -2'):
        units.assign_wide(torch.zeros(4, 40).to(dev), et, en)
    with _raises(RuntimeError, 'msmc_vq_assign_wide failed with code -2'):
        units.assign_units(torch.zeros(4, 40).to(dev), torch.randn(24, 40, generator=gen), device=dev)


# ---- (e) collapse -----------------------------------------------------------------------------------------------------------------------
COLLAPSE_T = (1, 7, 256, 257, 1000)
POISON = -99


def restated_collapse(ind, length):
    B, T = ind.shape
    units, dur, ulen = np.full((B, T), -1, dtype=np.int64), np.zeros((B, T), dtype=np.int32), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = min(max(int(length[b]), 0), T)
        row = ind[b, :n]
        if n:
            starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
            ulen[b] = len(starts)
            units[b, :len(starts)] = row[starts]
            dur[b, :len(starts)] = np.diff(np.r_[starts, n])
    return units, dur, ulen


@functools.lru_cache(maxsize=None)
def collapse_problem(T):
    """every label pattern at every length -> (ind [B, T], length [B]); beyond ``length`` even rows hold other labels, odd rows
    the last valid label again (read by mistake, the one adds runs and the other lengthens the last)"""
    t = np.arange(T, dtype=np.int64)
    rng = np.random.default_rng(5930 + T)
    patterns = [np.full(T, 3, dtype=np.int64), t.copy(), t % 2, rng.integers(0, 3, T)]
    if T > 270:
        p = t.copy()
        p[250:271] = 5000                       # a run across the 256-frame chunk boundary
        patterns.append(p)
    if T >= 1000:
        p = t.copy()
        p[100:901] = 6000                       # a run that covers whole chunks
        patterns.append(p)
    rows, lengths = [], []
    for p in patterns:
        for n in (0, 1, T, max(T - 3, 0), -2, T + 5):
            row = p.copy()
            valid = min(max(n, 0), T)
            row[valid:] = (7000 + t[valid:]) if len(rows) % 2 == 0 or valid == 0 else row[valid - 1]
            rows.append(row)
            lengths.append(n)
    return np.stack(rows), np.array(lengths, dtype=np.int64)


def check_collapse(dev, T):
    from msmctts_amd.hip import lib, units as hipunits
    ind, length = collapse_problem(T)
    B = ind.shape[0]
    wu, wd, wl = restated_collapse(ind, length)
    indd, lend = torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
    units = torch.full((B, T), POISON, dtype=torch.int64).to(dev)
    dur = torch.full((B, T), POISON, dtype=torch.int32).to(dev)
    ulen = torch.full((B,), POISON, dtype=torch.int64).to(dev)
    rc = lib.get().msmc_units_collapse(lib.ptr(indd), lib.ptr(lend), lib.ptr(units), lib.ptr(dur), lib.ptr(ulen), B, T, lib.stream(indd))
    assert rc == 0
    units, dur, ulen = units.cpu().numpy(), dur.cpu().numpy(), ulen.cpu().numpy()
    assert np.array_equal(ulen, wl), (ulen.tolist(), wl.tolist())
    assert np.array_equal(units, wu) and np.array_equal(dur, wd)
    for b in range(B):
        n = int(ulen[b])
        assert bool((units[b, n:] == -1).all()) and bool((dur[b, n:] == 0).all())
        assert int(dur[b, :n].sum()) == min(max(int(length[b]), 0), T)
    assert np.array_equal(indd.cpu().numpy(), ind), 'ind was written'
    got = hipunits.collapse_units(indd, lend)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int64
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, (wu, wd, wl)))


def check_collapse_refusals(dev):
    from msmctts_amd.hip import lib
    g = torch.full((4,), POISON, dtype=torch.int64).to(dev)
    g32 = torch.full((4,), POISON, dtype=torch.int32).to(dev)
    for B, T in ((0, 4), (4, 0), (-1, 4), (1, -4)):
        rc = lib.get().msmc_units_collapse(lib.ptr(g), lib.ptr(g), lib.ptr(g), lib.ptr(g32), lib.ptr(g), B, T, lib.stream(g))
        assert rc == E_SHAPE, (B, T, rc)
    for B, T, K in ((0, 4, 3), (1, 0, 3), (1, 4, 0), (1, 4, -2)):
        rc = lib.get().msmc_units_usage(lib.ptr(g), lib.ptr(g), lib.ptr(g), B, T, K, 0, lib.stream(g))
        assert rc == E_SHAPE, (B, T, K, rc)
    assert bool((g.cpu() == POISON).all()) and bool((g32.cpu() == POISON).all())


# ---- (f) usage ---------------------------------------------------------------------------------------------------------------------------
def check_usage(dev, K):
    """B = 5, T = 1000: two workgroups; K = 5000: two passes over the LDS counters"""
    from msmctts_amd.hip import units as hipunits
    B, T = 5, 1000
    rng = np.random.default_rng(5940 + K)
    ind = rng.integers(0, K, (B, T)).astype(np.int64)
    ind[rng.random((B, T)) < 0.05] = -1
    ind[rng.random((B, T)) < 0.05] = K
    ind[0, :8] = K - 1
    length = np.array([T, 0, 613, T + 9, -4], dtype=np.int64)
    valid = np.concatenate([ind[b, :min(max(int(length[b]), 0), T)] for b in range(B)])
    assert (valid == -1).any() and (valid == K).any()
    want = np.bincount(valid[(valid >= 0) & (valid < K)], minlength=K).astype(np.int64)
    indd, lend = torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
    got = hipunits.unit_usage(indd, lend, K)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    counts = torch.full((K,), POISON, dtype=torch.int64).to(dev)          # accumulate = 0 overwrites
    from msmctts_amd.hip import lib
    lib.call('msmc_units_usage', lib.ptr(indd), lib.ptr(lend), lib.ptr(counts), B, T, K, 0, lib.stream(indd))
    assert np.array_equal(counts.cpu().numpy(), want)
    again = hipunits.unit_usage(indd, lend, K, counts)                    # accumulate = 1, twice
    assert again is counts and np.array_equal(counts.cpu().numpy(), 2 * want)
    hipunits.unit_usage(indd, lend, K, counts)
    assert np.array_equal(counts.cpu().numpy(), 3 * want)


def reference_complexity(all_indices):
    """``compute_codebook_complexity`` of the reference's vq_analysis.py, restated: a dictionary of counts in order of first
    appearance -> (codes used, -sum p log2 p)"""
    codebook = {}
    for indices in all_indices:
        for code in indices.tolist():
            codebook[code] = codebook.get(code, 0) + 1
    num_used = np.asarray(list(codebook.values()))
    probs = num_used / num_used.sum()
    return len(codebook), float(-(probs * np.log2(probs)).sum())


def check_usage_summary():
    from msmctts_amd.hip.units import usage_summary
    assert usage_summary(np.array([4, 0, 2, 2, 0])) == (3, 1.5)
    assert usage_summary(torch.tensor([0, 0, 9])) == (1, 0.0)
    assert usage_summary(np.zeros(4, dtype=np.int64)) == (0, 0.0)
    seqs = [np.array([5, 5, 1, 0, 5, 3]), np.array([3, 3, 3, 7]), np.array([1])]
    counts = np.bincount(np.concatenate(seqs), minlength=9)
    used, bits = usage_summary(counts)
    want_used, want_bits = reference_complexity(seqs)
    assert used == want_used and abs(bits - want_bits) <= 1e-12


# ---- (g) host side ---------------------------------------------------------------------------------------------------------------------
def check_assign_units_inputs(dev):
    from msmctts_amd.hip import units
    d, K, N = 64, 24, 200
    x, embed = kc.problem(d, K, N, 5950)
    centers = embed[0].t().contiguous()
    rc, want_i, want_d = assign(dev, x, embed)
    assert rc == 0
    results = {'numpy': units.assign_units(x.numpy(), centers.numpy(), device=dev),
               'host tensor': units.assign_units(x, centers, device=dev),
               'device tensor': units.assign_units(x.to(dev), centers.to(dev), device=dev),
               'block 64': units.assign_units(x.numpy(), centers, block=64, device=dev),
               'block 1': units.assign_units(x[:5], centers, block=1, device=dev)}
    for name, (ind, dist) in results.items():
        n = 5 if name == 'block 1' else N
        assert ind.dtype == torch.int64 and dist.dtype == torch.float32 and tuple(ind.shape) == (n,) == tuple(dist.shape), name
        assert torch.equal(ind.cpu(), want_i[:n]) and same_bits(dist.cpu(), want_d[:n]), name
    ind, dist = units.assign_units(x, centers, want_dist=False, device=dev)
    assert dist is None and torch.equal(ind.cpu(), want_i)
    ind, dist = units.assign_units(x[:0], centers, device=dev)
    assert tuple(ind.shape) == (0,) and tuple(dist.shape) == (0,)


def check_assign_units_centres(dev, tmpdir):
    """the forms ``centers`` takes: an array, a ``.npy`` path, what ``fit_kmeans`` returns"""
    from msmctts_amd.hip import kmeans, units
    d, K, N = 64, 24, 40
    x, embed = kc.problem(d, K, N, 5950)
    centers = embed[0].t().contiguous().numpy()
    want = units.assign_units(x, centers, device=dev)
    path = os.path.join(str(tmpdir), 'centres.npy')
    np.save(path, centers)
    fit = kmeans.KMeansFit(centers, None, 0.0, 0, None, None, [])
    for form in (path, fit, torch.from_numpy(centers)):
        ind, dist = units.assign_units(x, form, device=dev)
        assert torch.equal(ind, want[0]) and same_bits(dist, want[1])
    with _raises(ValueError, '.npy'):
        units.assign_units(x, os.path.join(str(tmpdir), 'centres.pkl'), device=dev)
    with _raises(ValueError, 'centers [K, 32]'):
        units.assign_units(x, centers[:, :32], device=dev)


def check_quantizer_units(dev, tmpdir):
    """``KMeansQuantizer.units`` on a codebook file the test writes (d = 64, K = 24: ``forward`` runs the wide search): the
    labels are ``forward``'s ``quantizer_indices``; collapsed, ``repeat_interleave(units, dur)`` is the valid prefix again"""
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansQuantizer
    d, K, B, T = 64, 24, 3, 12
    x, embed = kc.problem(d, K, B * T, 5960)
    path = os.path.join(str(tmpdir), 'units.npy')
    np.save(path, embed[0].t().contiguous().numpy())
    q = KMeansQuantizer(path).to(dev).eval()
    emb = x.view(B, T, d).clone()
    emb[1, 2:6] = emb[1, 2]                     # repeated frames: runs longer than one
    emb[0, 9:] = emb[0, 9]
    emb = emb.to(dev)
    lengths = torch.tensor([12, 7, 0], dtype=torch.int64).to(dev)
    with torch.no_grad():
        qs = q([(emb, lengths)])
    assert last_kernel() == kc.WIDE, last_kernel()
    labels = q.units(emb, lengths)
    assert last_kernel() == ASSIGN, last_kernel()
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (B, T) and not labels.requires_grad
    assert torch.equal(labels, qs['quantizer_indices'][0])
    same, units, dur, ulen = q.units(emb, lengths, collapse=True)
    assert torch.equal(same, labels) and dur.dtype == torch.int32
    assert ulen.tolist()[2] == 0 and int(ulen[1]) < 7 and int(ulen[0]) < 12
    for b in range(B):
        n = int(ulen[b])
        again = torch.repeat_interleave(units[b, :n], dur[b, :n].long())
        assert torch.equal(again, labels[b, :int(lengths[b])]), b


def check_tool(dev, tmpdir, capsys=None):
    """tools/extract_units.py (in process) on three tiny feature files: the files it writes and the line it prints"""
    from msmctts_amd.hip import units
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('extract_units_tool', os.path.join(root, 'tools', 'extract_units.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    d, K = 64, 24
    x, embed = kc.problem(d, K, 40, 5970)
    centers = embed[0].t().contiguous().numpy()
    tmp = str(tmpdir)
    np.save(os.path.join(tmp, 'centres.npy'), centers)
    feats = {'a': x[:17].numpy(), 'b': x[17:18].numpy(), 'c': x[18:].repeat_interleave(2, dim=0).numpy()}
    with open(os.path.join(tmp, 'ids.list'), 'w') as f:
        for name, v in feats.items():
            np.save(os.path.join(tmp, 'feat_%s.npy' % name), v)
            f.write('%s spk0\n' % name)
    want = {name: units.assign_units(v, centers, want_dist=False, device=dev)[0].cpu().numpy() for name, v in feats.items()}
    bins = np.bincount(np.concatenate(list(want.values())), minlength=K).astype(np.int64)
    for jobs, collapse in ((1, False), (2, True)):
        out = os.path.join(tmp, 'out%d' % jobs)
        stdout = io.StringIO()
        with contextlib.redirect_stdout(stdout):
            counts = tool.main([os.path.join(tmp, 'ids.list'), os.path.join(tmp, 'feat_{0}.npy'), '-c', os.path.join(tmp, 'centres.npy'),
                                '-o', out, '--jobs', str(jobs), '--device', dev] + (['--collapse'] if collapse else []))
        used, bits = units.usage_summary(bins)
        assert stdout.getvalue().strip().splitlines()[-1] == '%d %s' % (used, bits), stdout.getvalue()
        ref_used, ref_bits = reference_complexity(list(want.values()))
        assert used == ref_used and abs(bits - ref_bits) <= 1e-12
        assert np.array_equal(counts, bins) and np.array_equal(np.load(os.path.join(out, 'usage.npy')), bins)
        assert sorted(os.listdir(out)) == sorted(['indices', 'usage.npy'] + (['units', 'durations'] if collapse else []))
        for name, labels in want.items():
            got = np.load(os.path.join(out, 'indices', name + '.npy'))
            assert got.dtype == np.int64 and np.array_equal(got, labels), name
            if collapse:
                u, du = np.load(os.path.join(out, 'units', name + '.npy')), np.load(os.path.join(out, 'durations', name + '.npy'))
                assert u.dtype == np.int64 and du.dtype == np.int32 and np.array_equal(np.repeat(u, du), labels), name
                assert bool((u[1:] != u[:-1]).all())
        if collapse:
            assert len(np.load(os.path.join(out, 'units', 'c.npy'))) <= 22


# ---- (h) feature presence ---------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    for name in ('msmc_vq_assign_wide', 'msmc_units_collapse', 'msmc_units_usage'):
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import (KMeansQuantizer, assign_units, collapse_units, unit_usage,  # noqa: F401
                                                              usage_summary)
    assert callable(KMeansQuantizer.units)
