"""Shared cases of the EMA codebook update of one wide head (csrc/ema_wide.hip: msmc_vq_ema_wide_workspace / _stats / _apply /
_update; ``vq_ema_update(wide=True)`` and ``CodebookSync(wide=True)`` of msmctts_amd/hip/vq.py; ``Quantize.ema_wide`` and
``VQGANTrainer(wide_codebook_update=True)``).  tests/test_ema_wide_emu.py runs them on the kernel interpreter,
tests/test_gpu_ema_wide.py on the GPU.

Primary reference: ``restated_update``, the order documented in include/msmc_hip.h in numpy fp32, compared BIT FOR BIT (both
builds compile with -ffp-contract=off; the two fused multiply-adds are restated exactly by ``fma32``).  The sums are
``restated_stats`` of tests/_kmeansfitcases.py on the masked labels.

Secondary reference: ``float64_update``, the reference's own arithmetic (modules.py:35-57: one-hot sums over the valid frames,
``mul_(decay).add_(., alpha=1 - decay)``, Laplace smoothing, division) in float64, on the parameter values the kernel receives
(decay and eps rounded to fp32).  The bound is derived, not measured.  With u = 2^-24 and first-order error terms:

  * a sum s[k][j] of m rows: a run is a chain of at most 64 adds onto +0 (63 roundings), the centroid's total a chain of
    ceil(m / 64) adds of run partials, all bounded by u * (the sum of |x| over the rows) each:
        E_s = (63 + ceil(m / 64)) u sum|x|
  * n, a sum of K non-negative terms: a chain of ceil(K / 256) adds per strided partial and 8 levels of the halving tree:
        R_n = ceil(K / 256) + 8 roundings, relative (all terms have one sign)
  * the rest: R = 8 single roundings, relative to the magnitude A = |embed_avg| decay + |s| (1 - decay) of the new embed_avg
    before cancellation (for cluster_size: to the new cluster_size, whose terms are non-negative).
        cluster_size : R u cs
        embed_avg    : (1 - decay) E_s + R u A
        embed        : ((1 - decay) E_s + (R_n + R) u A) / sm,      sm = (cs + eps) / (n + K eps) n
  Allowed: twice these values (``ALLOW``).  A worst-case count of the single roundings stays inside that allowance: embed_avg
  takes 3 (1 - decay, embed_avg decay, the fma); cluster_size 3 (1 - decay, cluster_size decay, the fma); embed takes the 3 of
  embed_avg, the 3 of cs_new[k], +eps, K eps, n + K eps, the division, the multiplication by n (n itself enters sm with
  sensitivity K eps / (n + K eps) <= 1: R_n and the 3 roundings of every term of n once) and the final division: 15 + R_n
  <= 2 (8 + R_n) because R_n >= 9.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from _kmeansfitcases import E_WORKSPACE, RUN, float64_stats, restated_stats
from _vqstreamcases import E_SHAPE, _raises, same_bits

U = 2.0 ** -24
R_REST = 8
ALLOW = 2.0
DECAY, EPS = 0.99, 1e-5
GUARD = 7                                                   # sentinel elements behind every output buffer

# d, K, B, T, lengths
SHAPES = ((16, 1, 1, 1, (1,)), (16, 5, 2, 130, (130, 7)), (272, 100, 3, 100, (100, 0, 37)), (528, 24, 2, 40, (40, 9)),
          (1024, 300, 2, 200, (200, 63)), (2048, 17, 1, 70, (70,)), (768, 2000, 2, 150, (150, 150)), (64, 3, 1, 1031, (1031,)))
IDS = ['d%d K%d B%d T%d' % s[:4] for s in SHAPES]
ONE_CENTROID = 7                                            # every frame on centroid 1: it spans 17 runs
LARGE = (5, 6)                                              # one update on the interpreter
BOTH = (2, 7)                                               # shapes msmc_vq_ema_update takes as well
UPDATES = 3


@functools.lru_cache(maxsize=None)
def problem(s):
    """seeded host tensors, computed once and never modified: x [UPDATES, B, T, d], ind [UPDATES, B, T], length [B], and the
    initial buffers embed [d, K], cluster_size [K] (> 0, so n > 0), embed_avg [d, K]"""
    d, K, B, T, lengths = SHAPES[s]
    gen = torch.Generator().manual_seed(6100 + s)
    x = torch.randn(UPDATES, B, T, d, generator=gen)
    ind = torch.randint(0, K, (UPDATES, B, T), generator=gen)
    if s == ONE_CENTROID:
        ind = torch.ones(UPDATES, B, T, dtype=torch.int64)
    embed = torch.randn(d, K, generator=gen)
    cs = torch.rand(K, generator=gen) * 4.0 + 0.25
    ea = embed * cs.unsqueeze(0) + 0.1 * torch.randn(d, K, generator=gen)
    return x.contiguous(), ind.contiguous(), torch.tensor(lengths, dtype=torch.int64), embed, cs, ea.contiguous()


# ---- references -----------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 arrays, correctly rounded: the product of two fp32 numbers is exact in float64; the float64 sum is
    formed with its exact error (two-sum) and, where inexact, moved to the neighbour with an odd last bit (round to odd, 53 >=
    24 + 2 bits), so that the rounding to fp32 is the single rounding of the exact a b + c"""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def masked_labels(ind, length):
    B, T = ind.shape
    valid = np.arange(T)[None, :] < np.asarray(length)[:, None]
    return np.where(valid, np.asarray(ind), -1).reshape(-1), valid.reshape(-1)


def restated_n(cs_new):
    """the sum of vq_ema_kernel: 256 strided partials in ascending k from +0, then the halving tree"""
    p = np.zeros(256, dtype=np.float32)
    for k0 in range(0, len(cs_new), 256):
        part = cs_new[k0:k0 + 256]
        p[:len(part)] = p[:len(part)] + part
    s = 128
    while s > 0:
        p[:s] = p[:s] + p[s:2 * s]
        s >>= 1
    return p[0]


def restated_apply(sums, counts, embed, cs, ea, decay=DECAY, eps=EPS):
    """the update of the header from [K][d] sums and [K] counts, numpy fp32 -> (embed, cluster_size, embed_avg)"""
    ea, cs = np.asarray(ea, dtype=np.float32), np.asarray(cs, dtype=np.float32)
    K = cs.shape[0]
    decay, eps = np.float32(decay), np.float32(eps)
    omd = np.float32(1.0 - np.float64(decay))
    keps = np.float32(np.float64(K) * np.float64(eps))
    cs_new = fma32(np.float32(0) + counts, omd, cs * decay)
    n = restated_n(cs_new)
    sm = (cs_new + eps) / (n + keps) * n
    ea_new = fma32(np.ascontiguousarray(sums.T), omd, ea * decay)
    return ea_new / sm[None, :], cs_new, ea_new


def restated_update(x, ind, length, embed, cs, ea, decay=DECAY, eps=EPS):
    K = np.asarray(cs).shape[0]
    lab, _ = masked_labels(ind, length)
    xf = np.asarray(x, dtype=np.float32).reshape(len(lab), -1)
    xf = np.where((lab >= 0)[:, None], xf, np.float32(0))           # (padded rows are never part of a sum: NaN there is allowed)
    sums, counts = restated_stats(xf, lab, K)
    return restated_apply(sums, counts, embed, cs, ea, decay, eps)


def float64_update(x, ind, length, embed, cs, ea, decay=DECAY, eps=EPS, generic_sums=False):
    """modules.py:35-57 in float64 -> ((embed, cluster_size, embed_avg), (their bounds as the module docstring derives them));
    ``generic_sums``: E_s = m u sum|x|, the bound of m - 1 adds in ANY order (the resident kernels' sums)"""
    cs, ea = np.asarray(cs, dtype=np.float64), np.asarray(ea, dtype=np.float64)
    K = cs.shape[0]
    decay, eps = float(np.float32(decay)), float(np.float32(eps))
    lab, valid = masked_labels(ind, length)
    xf = np.asarray(x, dtype=np.float64).reshape(len(lab), -1)
    xf = np.where(valid[:, None], xf, 0.0)
    s64, a64, m = float64_stats(xf, lab, K)
    cs_new = cs * decay + (1 - decay) * m
    ea_new = ea * decay + (1 - decay) * s64.T
    n = cs_new.sum()
    sm = (cs_new + eps) / (n + K * eps) * n
    embed_new = ea_new / sm[None, :]
    chain = m if generic_sums else 63 + np.ceil(m / RUN)
    e_s = (chain[:, None] * U * a64).T                                        # [d, K]
    mag = np.abs(ea) * decay + np.abs(s64.T) * (1 - decay)
    r_n = math.ceil(K / 256) + 8
    b_cs = ALLOW * R_REST * U * cs_new
    b_ea = ALLOW * ((1 - decay) * e_s + R_REST * U * mag)
    b_embed = ALLOW * ((1 - decay) * e_s + (r_n + R_REST) * U * mag) / sm[None, :]
    assert n > 0
    return (embed_new, cs_new, ea_new), (b_embed, b_cs, b_ea)


def within(got, want, bound, what):
    err = np.abs(got.double().numpy() - want)
    print('%s: largest error %.3g, largest error / allowed %.3g' % (what, float(err.max()), float((err / np.maximum(bound, 1e-300)).max())))
    assert bool((err <= bound).all()), '%s beyond the derived float64 bound by %.3g' % (what, float((err - bound).max()))


# ---- direct calls -----------------------------------------------------------------------------------------------------------------
def guarded(t):
    """a flat device-bound copy of ``t`` with GUARD NaN elements behind it"""
    return torch.cat([t.reshape(-1).float(), torch.full((GUARD,), float('nan'))])


def intact(buf, n):
    return bool(torch.isnan(buf[n:]).all()) and buf.numel() == n + GUARD


def run_update(dev, x, ind, length, embed, cs, ea, split=False, decay=DECAY, eps=EPS, ws_bytes=None, sizes=None):
    """msmc_vq_ema_wide_update (``split``: _stats then _apply) on copies of the buffers, GUARD sentinels behind each of them (and
    behind the stats block) checked -> (rc, embed, cluster_size, embed_avg, stats or None) on the host.  ``sizes`` = (B, T, d, K)
    passed in place of the tensors' own; ``ws_bytes``: the size passed in place of the workspace's own"""
    from msmctts_amd.hip import lib
    L = lib.get()
    d0, K0 = embed.shape
    B, T, d, K = sizes if sizes is not None else (x.shape[0], x.shape[1], d0, K0)
    e, c, a = guarded(embed).to(dev), guarded(cs).to(dev), guarded(ea).to(dev)
    xd, indd, ln = x.contiguous().to(dev), ind.contiguous().to(dev), length.to(dev)
    need = int(L.msmc_vq_ema_wide_workspace(B * T, d, K))
    have = int(L.msmc_vq_ema_wide_workspace(x.shape[0] * x.shape[1], d0, K0))          # (a refused size is never allocated for)
    ws = torch.full((have // 4 + GUARD,), float('nan')).to(dev)
    nbytes = need if ws_bytes is None else ws_bytes
    stats = None
    if split:
        stats = torch.full((K0 * (d0 + 2) + GUARD,), float('nan')).to(dev)
        rc = L.msmc_vq_ema_wide_stats(lib.ptr(xd), lib.ptr(indd), lib.ptr(ln), lib.ptr(stats), lib.ptr(ws), nbytes, B, T, d, K,
                                      lib.stream(xd))
        if rc == 0:
            rc = L.msmc_vq_ema_wide_apply(lib.ptr(stats), lib.ptr(e), lib.ptr(c), lib.ptr(a), d, K, decay, eps, lib.stream(xd))
        stats = stats.cpu()
        assert intact(stats, K0 * (d0 + 2)), 'the stats block was written beyond K (d + 2) floats'
    else:
        rc = L.msmc_vq_ema_wide_update(lib.ptr(xd), lib.ptr(indd), lib.ptr(ln), lib.ptr(e), lib.ptr(c), lib.ptr(a), lib.ptr(ws),
                                       nbytes, B, T, d, K, decay, eps, lib.stream(xd))
    e, c, a, ws = e.cpu(), c.cpu(), a.cpu(), ws.cpu()
    assert intact(e, d0 * K0) and intact(c, K0) and intact(a, d0 * K0), 'a buffer was written beyond its size'
    assert bool(torch.isnan(ws[have // 4:]).all()), 'the workspace was written beyond msmc_vq_ema_wide_workspace'
    return rc, e[:d0 * K0].view(d0, K0), c[:K0], a[:d0 * K0].view(d0, K0), stats


def bits(t):
    return torch.from_numpy(np.ascontiguousarray(t))


# ---- 1. every shape, three successive updates --------------------------------------------------------------------------------------
def check_shape(dev, s, updates=UPDATES):
    d, K, B, T, lengths = SHAPES[s]
    x, ind, length, embed, cs, ea = problem(s)
    want = (embed.numpy(), cs.numpy(), ea.numpy())
    for u in range(updates):
        rc, e, c, a, _ = run_update(dev, x[u], ind[u], length, embed, cs, ea)
        assert rc == 0, rc
        want = restated_update(x[u], ind[u], length, *want)
        ref, bound = float64_update(x[u], ind[u], length, embed, cs, ea)
        what = 'd=%d K=%d update %d' % (d, K, u)
        within(e, ref[0], bound[0], what + ' embed')
        within(c, ref[1], bound[1], what + ' cluster_size')
        within(a, ref[2], bound[2], what + ' embed_avg')
        assert same_bits(c, bits(want[1])), what + ': cluster_size is not the restated bits'
        assert same_bits(a, bits(want[2])), what + ': embed_avg is not the restated bits (%d elements)' % int(
            (a.view(torch.int32) != bits(want[2]).view(torch.int32)).sum())
        assert same_bits(e, bits(want[0])), what + ': embed is not the restated bits (%d elements)' % int(
            (e.view(torch.int32) != bits(want[0]).view(torch.int32)).sum())
        assert bool(torch.isfinite(e).all()) and float(c.sum()) > 0
        embed, cs, ea = e, c, a
    if s == ONE_CENTROID:
        assert T > 16 * RUN


# ---- 2. padded frames are never read -----------------------------------------------------------------------------------------------
def check_padding_is_never_read(dev, s):
    d, K, B, T, lengths = SHAPES[s]
    x, ind, length, embed, cs, ea = problem(s)
    pad = torch.arange(T)[None, :] >= length[:, None]
    assert bool(pad.any())
    zeroed, poisoned = x[0].clone(), x[0].clone()
    zeroed[pad] = 0.0
    poisoned[pad] = float('nan')
    rc0, e0, c0, a0, _ = run_update(dev, zeroed, ind[0], length, embed, cs, ea)
    rc1, e1, c1, a1, _ = run_update(dev, poisoned, ind[0], length, embed, cs, ea)
    assert rc0 == 0 and rc1 == 0
    assert bool(torch.isfinite(e1).all()) and bool(torch.isfinite(c1).all()) and bool(torch.isfinite(a1).all())
    assert same_bits(e0, e1) and same_bits(c0, c1) and same_bits(a0, a1)


# ---- 3. the two halves are the fused call; a call repeats its bits ---------------------------------------------------------------------
def check_halves_and_repeat(dev, s):
    d, K, B, T, lengths = SHAPES[s]
    x, ind, length, embed, cs, ea = problem(s)
    rc0, e0, c0, a0, _ = run_update(dev, x[0], ind[0], length, embed, cs, ea)
    rc1, e1, c1, a1, _ = run_update(dev, x[0], ind[0], length, embed, cs, ea)
    rc2, e2, c2, a2, stats = run_update(dev, x[0], ind[0], length, embed, cs, ea, split=True)
    assert rc0 == 0 and rc1 == 0 and rc2 == 0
    assert same_bits(e0, e1) and same_bits(c0, c1) and same_bits(a0, a1), 'two identical calls differ'
    assert same_bits(e0, e2) and same_bits(c0, c2) and same_bits(a0, a2), '_stats + _apply is not _update'
    lab, _ = masked_labels(ind[0], length)
    xf = np.where((lab >= 0)[:, None], x[0].reshape(-1, d).numpy(), np.float32(0))
    sums, counts = restated_stats(xf, lab, K)
    assert same_bits(stats[:K * d].view(K, d), bits(sums)) and same_bits(stats[K * d:K * d + K], bits(counts))
    assert same_bits(stats[K * d + K:K * d + 2 * K], c0), 'the scratch of _apply holds the new cluster sizes'


# ---- 4. against the resident kernels where both take the shape ----------------------------------------------------------------------
def check_against_resident(dev, s):
    from msmctts_amd.hip import vq
    d, K, B, T, lengths = SHAPES[s]
    assert vq.ema_resident_takes(1, d, K) and vq.wide_takes(1, d, K)
    x, ind, length, embed, cs, ea = problem(s)
    got = {}
    for wide in (False, True):
        e, c, a = (t.clone().unsqueeze(0).to(dev) for t in (embed, cs, ea))
        vq.vq_ema_update(x[0].to(dev), ind[0].unsqueeze(-1).to(dev), length.to(dev), e, c, a, DECAY, EPS, wide=wide)
        got[wide] = (e[0].cpu(), c[0].cpu(), a[0].cpu())
        sync = vq.CodebookSync(embed.clone().unsqueeze(0).to(dev), cs.clone().unsqueeze(0).to(dev), ea.clone().unsqueeze(0).to(dev),
                               DECAY, EPS, wide=wide)
        sync.collect(x[0].to(dev), ind[0].unsqueeze(-1).to(dev), length.to(dev))
        got[wide] += (sync.stats.cpu(),)
    rc, e, c, a, _ = run_update(dev, x[0], ind[0], length, embed, cs, ea)
    assert rc == 0 and same_bits(got[True][0], e) and same_bits(got[True][1], c) and same_bits(got[True][2], a), 'the wrapper'
    assert same_bits(got[True][1], got[False][1]), 'cluster_size differs from msmc_vq_ema_update'
    st_w, st_r = got[True][3], got[False][3]
    assert st_w.numel() == st_r.numel() == K * (d + 2)
    assert same_bits(st_w[K * d:K * d + K], st_r[K * d:K * d + K]), 'counts differ from msmc_vq_ema_stats'
    lab, valid = masked_labels(ind[0], length)
    s64, a64, m = float64_stats(np.where(valid[:, None], x[0].reshape(-1, d).double().numpy(), 0.0), lab, K)
    assert np.array_equal(st_w[K * d:K * d + K].numpy(), m.astype(np.float32))
    within(st_w[:K * d].view(K, d), s64, (63 + np.ceil(m / RUN))[:, None] * U * a64, 'wide sums')
    within(st_r[:K * d].view(K, d), s64, m[:, None] * U * a64, 'resident sums')
    for wide in (False, True):
        ref, bound = float64_update(x[0], ind[0], length, embed, cs, ea, generic_sums=not wide)
        within(got[wide][0], ref[0], bound[0], 'wide=%s embed' % wide)
        within(got[wide][2], ref[2], bound[2], 'wide=%s embed_avg' % wide)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def workspace_formula(N, d, K):
    from msmctts_amd.hip import lib
    return (8 * N + 15) // 16 * 16 + int(lib.get().msmc_kmeans_stats_workspace(N, d, K)) + 4 * K * (d + 2)


def check_refusals(dev):
    from msmctts_amd.hip import lib, vq
    L = lib.get()
    gen = torch.Generator().manual_seed(6190)

    def unchanged(res, embed, cs, ea):
        return same_bits(res[1], embed) and same_bits(res[2], cs) and same_bits(res[3], ea)

    for d, K, B, T in ((24, 5, 2, 9), (8, 5, 2, 9), (2064, 5, 1, 3), (16, 0, 2, 9), (16, 5, 0, 9), (16, 5, 2, 0)):
        x, ind = torch.randn(max(B, 1), max(T, 1), d, generator=gen), torch.zeros(max(B, 1), max(T, 1), dtype=torch.int64)
        embed, cs, ea = torch.randn(d, max(K, 1), generator=gen), torch.ones(max(K, 1)), torch.randn(d, max(K, 1), generator=gen)
        length = torch.full((max(B, 1),), max(T, 1), dtype=torch.int64)
        for split in (False, True):
            res = run_update(dev, x, ind, length, embed, cs, ea, split=split, ws_bytes=1 << 40, sizes=(B, T, d, K))
            assert res[0] == E_SHAPE and unchanged(res, embed, cs, ea), (d, K, B, T, split, res[0])
            assert split is False or bool(torch.isnan(res[4]).all())
        assert int(L.msmc_vq_ema_wide_workspace(B * T, d, K)) == 0
        if B * T > 0:                                       # _apply takes no frame count: it refuses the width and K = 0
            stats = torch.zeros(max(K, 1) * (d + 2)).to(dev)
            e, c, a = guarded(embed).to(dev), guarded(cs).to(dev), guarded(ea).to(dev)
            rc = L.msmc_vq_ema_wide_apply(lib.ptr(stats), lib.ptr(e), lib.ptr(c), lib.ptr(a), d, K, DECAY, EPS, lib.stream(e))
            assert rc == E_SHAPE and same_bits(e.cpu(), guarded(embed)) and same_bits(c.cpu(), guarded(cs)) and same_bits(a.cpu(), guarded(ea))
    # N * d * 4 >= 2^32: sizes only, refused before anything is read or allocated
    x, ind, length = torch.randn(1, 9, 64, generator=gen), torch.zeros(1, 9, dtype=torch.int64), torch.tensor([9])
    embed, cs, ea = torch.randn(64, 5, generator=gen), torch.ones(5), torch.randn(64, 5, generator=gen)
    for split in (False, True):
        res = run_update(dev, x, ind, length, embed, cs, ea, split=split, ws_bytes=1 << 40, sizes=(1 << 12, 1 << 12, 64, 5))
        assert res[0] == E_SHAPE and unchanged(res, embed, cs, ea), res[0]
    assert int(L.msmc_vq_ema_wide_workspace(1 << 24, 64, 5)) == 0
    assert int(L.msmc_vq_ema_wide_workspace((1 << 24) - 1, 64, 5)) == workspace_formula((1 << 24) - 1, 64, 5)
    # a workspace one byte short
    s = 1
    d, K, B, T, lengths = SHAPES[s]
    x, ind, length, embed, cs, ea = problem(s)
    need = int(L.msmc_vq_ema_wide_workspace(B * T, d, K))
    res = run_update(dev, x[0], ind[0], length, embed, cs, ea, ws_bytes=need - 1)
    assert res[0] == E_WORKSPACE and unchanged(res, embed, cs, ea), res[0]
    res = run_update(dev, x[0], ind[0], length, embed, cs, ea, split=True, ws_bytes=need - 4 * K * (d + 2) - 1)
    assert res[0] == E_WORKSPACE and unchanged(res, embed, cs, ea) and bool(torch.isnan(res[4]).all()), res[0]
    res = run_update(dev, x[0], ind[0], length, embed, cs, ea, split=True, ws_bytes=need - 4 * K * (d + 2))
    assert res[0] == 0, '_stats needs the labels and the statistics workspace only'
    # the documented size, at every shape of the cases and at the sizes of the issue
    for d, K, N in [(sh[0], sh[1], sh[2] * sh[3]) for sh in SHAPES] + [(768, 500, 6400), (1024, 1000, 51200), (1024, 2000, 51200)]:
        assert int(L.msmc_vq_ema_wide_workspace(N, d, K)) == workspace_formula(N, d, K), (d, K, N)
    # the wrapper: more than one head, and a width the wide kernels refuse
    e2 = torch.zeros(2, 16, 5).to(dev)
    with _raises(RuntimeError, 'msmc_vq_ema_wide_update takes one head'):
        vq.vq_ema_update(torch.zeros(1, 3, 32).to(dev), torch.zeros(1, 3, 2, dtype=torch.int64).to(dev), torch.tensor([3]).to(dev),
                         e2, torch.zeros(2, 5).to(dev), e2.clone(), DECAY, EPS, wide=True)
    e1 = torch.zeros(1, 24, 5).to(dev)
    with _raises(RuntimeError, 'msmc_vq_ema_wide_update failed with code -2'):
        vq.vq_ema_update(torch.zeros(1, 3, 24).to(dev), torch.zeros(1, 3, 1, dtype=torch.int64).to(dev), torch.tensor([3]).to(dev),
                         e1, torch.ones(1, 5).to(dev), e1.clone(), DECAY, EPS, wide=True)


# ---- 7. - 9. the module ----------------------------------------------------------------------------------------------------------------
def module_case(dim, K, seed):
    gen = torch.Generator().manual_seed(seed)
    B, T = 3, 21
    x = torch.randn(B, T, dim, generator=gen)
    length = torch.tensor([T, 0, 8])
    return x, length


def make_quantize(dev, dim, K, seed, flag):
    from msmctts_amd.networks.vqgantts.modules import Quantize
    torch.manual_seed(seed)
    q = Quantize(dim, K)
    q.cluster_size.copy_(torch.rand(K, generator=torch.Generator().manual_seed(seed + 1)) * 3.0 + 0.5)
    if flag is not None:
        q.ema_wide = flag
    return q.to(dev)


def state(q):
    return tuple(getattr(q, k).detach().cpu().clone() for k in ('embed', 'cluster_size', 'embed_avg'))


def check_module(dev, dim, K):
    from msmctts_amd.networks.vqgantts.modules import Quantize
    assert Quantize.ema_wide is False
    x, length = module_case(dim, K, 6200 + K)
    q = make_quantize(dev, dim, K, 6300 + K, True).train()
    before = state(q)
    quant, diff, ind = q(x.to(dev), length.to(dev), update=True)
    assert tuple(quant.shape) == tuple(x.shape) and tuple(ind.shape) == tuple(x.shape[:2])
    after = state(q)
    idx = ind.cpu()
    ref, bound = float64_update(x, idx, length, *before, decay=q.decay, eps=q.eps)
    for got, r, b, name in zip(after, ref, bound, ('embed', 'cluster_size', 'embed_avg')):
        within(got, r, b, 'Quantize(%d, %d) %s' % (dim, K, name))
    want = restated_update(x, idx, length, *(t.numpy() for t in before), decay=q.decay, eps=q.eps)
    assert all(same_bits(g, bits(w)) for g, w in zip(after, want)), 'the module is not the restated update of its own indices'
    assert not same_bits(after[0], before[0])
    # eval(), and update=False in training, leave the buffers alone
    q.eval()
    q(x.to(dev), length.to(dev), update=True)
    assert all(same_bits(a, b) for a, b in zip(state(q), after))
    q.train()
    q(x.to(dev), length.to(dev), update=False)
    assert all(same_bits(a, b) for a, b in zip(state(q), after))


def check_flag_is_opt_in(dev):
    """without the flag the call raises what tests/_kmeanscases.py check_routing pins; with it a width the resident kernels take
    keeps their bits"""
    x, length = module_case(1024, 100, 6400)
    q = make_quantize(dev, 1024, 100, 6401, None).train()
    with _raises(RuntimeError, 'msmc_vq_ema_update failed with code -2'):
        q(x.to(dev), length.to(dev), update=True)
    x, length = module_case(256, 64, 6402)
    out = []
    for flag in (None, True):
        q = make_quantize(dev, 256, 64, 6403, flag).train()
        q(x.to(dev), length.to(dev), update=True)
        out.append(state(q))
    assert all(same_bits(a, b) for a, b in zip(*out)), 'the flag changed the bits of a width msmc_vq_ema_update takes'


def check_sync_path(dev, dim, K):
    """sync_stats: statistics at the forward, the update at ``flush_codebook_sync(local=True)`` -- the fused path's bits"""
    from msmctts_amd.hip import vq
    x, length = module_case(dim, K, 6500 + K)
    out = []
    for sync in (False, True):
        q = make_quantize(dev, dim, K, 6501 + K, True).train()
        q.sync_stats = sync
        before = state(q)
        del vq.PENDING[:]
        q(x.to(dev), length.to(dev), update=True)
        if sync:
            assert all(same_bits(a, b) for a, b in zip(state(q), before)) and len(vq.PENDING) == 1 and vq.PENDING[0].wide
            vq.flush_codebook_sync(local=True)
            assert not vq.PENDING
        out.append(state(q))
        assert not same_bits(out[-1][0], before[0])
    assert all(same_bits(a, b) for a, b in zip(*out))


# ---- 10. the trainer's keyword ---------------------------------------------------------------------------------------------------------
def check_trainer_keyword():
    from _parity import build_small
    from msmctts_amd.networks.vqgantts.modules import Quantize
    from msmctts_amd.trainers import build_trainer
    for flag in (None, True):
        cfg, task = build_small('cpu')
        if flag:
            cfg.trainer.wide_codebook_update = True
        tr = build_trainer(cfg, task, num_gpus=0, rank=0)
        qs = [m for m in task.modules() if isinstance(m, Quantize)]
        assert qs and tr.wide_codebook_update is bool(flag)
        assert all(m.ema_wide is bool(flag) for m in qs)


# ---- 11. feature presence ---------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    for name in ('msmc_vq_ema_wide_workspace', 'msmc_vq_ema_wide_stats', 'msmc_vq_ema_wide_apply', 'msmc_vq_ema_wide_update'):
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
