"""Shared cases of the unit-input path: runs back to frame labels (csrc/units.hip, msmc_units_total / msmc_units_expand), the decoder
input from labels and its gradient (csrc/unit_embed.hip, msmc_units_embed_fwd / _bwd), their host side (msmctts_amd/hip/units.py
``expand_units`` / ``unit_embed``), ``KMeansVQGANEmb.forward_units`` / ``synthesis_units`` / ``unit_table``, the unit batch of
``EmbVQGANTrainer`` and tools/synthesize_units.py.  tests/test_unit_embed_emu.py runs the small cases on the kernel interpreter,
tests/test_gpu_unit_embed.py all of them on the GPU.

References.
* Expand: ``restated_expand`` (``np.repeat`` on the valid runs); exact.  Round trip through ``collapse_units``.
* Embed forward: ``table[ind] + glob`` in numpy fp32 on the valid rows, zeros elsewhere; BIT FOR BIT (one IEEE add per element).
* Embed backward: ``restated_stats`` of tests/_kmeansfitcases.py -- the documented run order of msmc_kmeans_stats -- on the masked
  labels and on the utterance numbers; BIT FOR BIT.
* Model: the float64 restatement ``centers W^T + b`` (+ the global embedding) for the decoder input of both paths, and the frame
  path (``forward`` on the centroid rows of the labels) for outputs and gradients, at the project's fp32 bar of 1e-3 relative to
  the tensor's maximum (tests/_embcases.py ``FP32_BAR``).
"""
import ctypes
import functools
import importlib.util
import os
import wave

import numpy as np
import torch

from _embcases import FP32_BAR, _raises
from _kmeansfitcases import restated_stats

E_SHAPE, E_WORKSPACE = -2, -3
POISON = -99


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- (a) expand ---------------------------------------------------------------------------------------------------------------------------
EXPAND_R = (1, 255, 256, 257, 600)


def restated_expand(units, dur, ulen, T):
    B, R = units.shape
    ind, length = np.full((B, T), -1, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = min(max(int(ulen[b]), 0), R)
        row = np.repeat(units[b, :n], np.maximum(dur[b, :n], 0).astype(np.int64))[:T]
        ind[b, :len(row)] = row
        length[b] = len(row)
    return ind, length


@functools.lru_cache(maxsize=None)
def expand_problem(R):
    """-> (units [B, R], dur [B, R], ulen [B]): random short runs; zero durations at the start, in the middle and on the chunk
    boundary; a negative duration; a run longer than 256 frames; ulen = 0, ulen > R and a ragged ulen; behind ulen the slots hold
    other units with positive durations (read by mistake, they add frames)"""
    rng = np.random.default_rng(6100 + R)
    rows = []
    for kind in range(7):
        units = rng.integers(0, 50, R).astype(np.int64)
        dur = rng.integers(1, 4, R).astype(np.int32)
        ulen = R
        if kind == 1:
            dur[0] = 0
            dur[R // 2] = 0
            for r in (254, 255, 256, 257):
                if r < R:
                    dur[r] = 0
        elif kind == 2:
            dur[R // 3] = -5
            dur[R - 1] = -1
        elif kind == 3:
            dur[R // 2] = 700                   # one run longer than a chunk of frames
        elif kind == 4:
            ulen = 0
        elif kind == 5:
            ulen = R + 9
        elif kind == 6:
            ulen = max(R - 2, 0)
        rows.append((units, dur, ulen))
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int64))


def check_expand(dev, R):
    from msmctts_amd.hip import lib, units as hipunits
    units, dur, ulen = expand_problem(R)
    B = units.shape[0]
    totals = np.array([np.maximum(dur[b, :min(max(int(ulen[b]), 0), R)], 0).astype(np.int64).sum() for b in range(B)])
    ud, dd, ld = (torch.from_numpy(a).to(dev) for a in (units, dur, ulen))
    total = torch.full((B,), POISON, dtype=torch.int64).to(dev)
    assert lib.get().msmc_units_total(lib.ptr(dd), lib.ptr(ld), lib.ptr(total), B, R, lib.stream(ud)) == 0
    assert np.array_equal(total.cpu().numpy(), totals), (total.tolist(), totals.tolist())
    big = int(totals.max())
    # T below, equal to and above the totals; T = 1; a run longer than T (kind 3 at every T below 700)
    for T in sorted({1, max(big // 2, 1), int(np.median(totals)) or 1, big, big + 300}):
        wi, wl = restated_expand(units, dur, ulen, T)
        ind = torch.full((B, T), POISON, dtype=torch.int64).to(dev)
        length = torch.full((B,), POISON, dtype=torch.int64).to(dev)
        rc = lib.get().msmc_units_expand(lib.ptr(ud), lib.ptr(dd), lib.ptr(ld), lib.ptr(ind), lib.ptr(length), B, R, T, lib.stream(ud))
        assert rc == 0
        assert np.array_equal(length.cpu().numpy(), wl), (R, T, length.tolist(), wl.tolist())
        got = ind.cpu().numpy()
        assert np.array_equal(got, wi), (R, T, np.argwhere(got != wi)[:4].tolist())
        gi, gl = hipunits.expand_units(ud, dd, ld, T=T)
        assert gi.dtype == torch.int64 and gl.dtype == torch.int64
        assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gl.cpu().numpy(), wl)
    assert np.array_equal(ud.cpu().numpy(), units) and np.array_equal(dd.cpu().numpy(), dur), 'an input was written'
    gi, gl = hipunits.expand_units(ud, dd, ld)                 # T = None: the longest utterance
    wi, wl = restated_expand(units, dur, ulen, max(big, 1))
    assert tuple(gi.shape) == (B, max(big, 1)) and np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gl.cpu().numpy(), wl)


def check_expand_round_trip(dev):
    """random labels with repeats and ragged lengths: ``expand_units(*collapse_units(ind, length))`` is the prefix again"""
    from msmctts_amd.hip import units as hipunits
    B, T = 6, 700
    rng = np.random.default_rng(6110)
    ind = np.repeat(rng.integers(0, 30, (B, T)), rng.integers(1, 6, T), axis=1)[:, :T].astype(np.int64)
    length = np.array([T, 0, 1, 257, 613, T + 4], dtype=np.int64)
    indd, lend = torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
    units, dur, ulen = hipunits.collapse_units(indd, lend)
    assert int(ulen.max()) < T
    gi, gl = hipunits.expand_units(units, dur, ulen, T=T)
    valid = np.arange(T)[None, :] < np.clip(length, 0, T)[:, None]
    assert np.array_equal(gl.cpu().numpy(), np.clip(length, 0, T))
    assert np.array_equal(gi.cpu().numpy(), np.where(valid, ind, -1))
    gi, gl = hipunits.expand_units(units, dur, ulen)
    assert tuple(gi.shape) == (B, T) and np.array_equal(gi.cpu().numpy(), np.where(valid, ind, -1))
    # nothing to expand at all: one frame of -1
    gi, gl = hipunits.expand_units(units[1:2], dur[1:2], ulen[1:2])
    assert tuple(gi.shape) == (1, 1) and gi.tolist() == [[-1]] and gl.tolist() == [0]


def check_expand_refusals(dev):
    from msmctts_amd.hip import lib, units as hipunits
    g = torch.full((4,), POISON, dtype=torch.int64).to(dev)
    g32 = torch.full((4,), POISON, dtype=torch.int32).to(dev)
    for B, R, T in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -1)):
        rc = lib.get().msmc_units_expand(lib.ptr(g), lib.ptr(g32), lib.ptr(g), lib.ptr(g), lib.ptr(g), B, R, T, lib.stream(g))
        assert rc == E_SHAPE, (B, R, T, rc)
    for B, R in ((0, 4), (1, 0), (-2, 4)):
        assert lib.get().msmc_units_total(lib.ptr(g32), lib.ptr(g), lib.ptr(g), B, R, lib.stream(g)) == E_SHAPE
    assert bool((g.cpu() == POISON).all()) and bool((g32.cpu() == POISON).all())
    with _raises(RuntimeError, 'msmc_units_expand failed with code -2'):
        hipunits.expand_units(g.view(1, 4), g32.view(1, 4), g[:1], T=0)


# ---- (b) embed forward ----------------------------------------------------------------------------------------------------------------
# B, T, C, K: every C, K, T and B of the edges; 2048-piece blocks that end inside a row (C = 64: 16 pieces per row, T = 257) and
# several blocks (3 * 257 * 64 / 2048 = 24)
FWD_SHAPES = ((1, 1, 8, 1), (3, 63, 64, 100), (3, 257, 256, 2000), (1, 63, 2048, 100), (3, 257, 8, 1), (1, 257, 64, 2000),
              (3, 1, 2048, 1), (3, 63, 256, 100))
FWD_IDS = ['B%d T%d C%d K%d' % s for s in FWD_SHAPES]


@functools.lru_cache(maxsize=None)
def embed_problem(B, T, C, K, seed=6200):
    """-> ind [B, T], length [B], table [K + 1, C] (row K is NaN: only an invalid label reaches it), glob [B, C].  Labels -1 and
    K inside the valid prefixes; lengths T, 0 and T + 3 where B allows; behind ``length`` the labels are valid ones (read by
    mistake they make a row)"""
    rng = np.random.default_rng(seed + 7 * B + 11 * T + 13 * C + K)
    ind = rng.integers(0, K, (B, T)).astype(np.int64)
    ind[rng.random((B, T)) < 0.1] = -1
    ind[rng.random((B, T)) < 0.1] = K
    length = np.array([T + 3, 0, max(T - 2, 1)][:B] if B > 1 else [T], dtype=np.int64)
    if B == 1 and T > 1:
        length[0] = T - 1
    table = rng.standard_normal((K + 1, C)).astype(np.float32)
    table[K] = np.nan
    glob = rng.standard_normal((B, C)).astype(np.float32)
    return ind, length, table, glob


def valid_rows(ind, length, K):
    B, T = ind.shape
    return (np.arange(T)[None, :] < length[:, None]) & (ind >= 0) & (ind < K)


def restated_embed(ind, length, table, glob, K):
    ok = valid_rows(ind, length, K)
    rows = table[np.where(ok, ind, 0)]
    if glob is not None:
        rows = rows + glob[:, None, :]
    return np.where(ok[:, :, None], rows, np.float32(0)).astype(np.float32)


def _at(dev, values, offset, fill=None):
    """a device copy of ``values`` (or, with ``fill``, a buffer of that shape filled with it) that starts ``offset`` floats into
    its allocation: 16-byte aligned for offset % 4 == 0"""
    buf = torch.zeros(values.size + 8).to(dev)
    view = buf[offset:offset + values.size].view(values.shape)
    if fill is None:
        view.copy_(torch.from_numpy(values))
    else:
        view.fill_(fill)
    return view


def embed_fwd(dev, ind, length, table, glob, K, offset=0, glob_offset=0, out_offset=0):
    """msmc_units_embed_fwd directly on a poisoned output -> (rc, out); ``*offset``: the table / glob / out start that many floats
    into their buffers"""
    from msmctts_amd.hip import lib
    B, T = ind.shape
    C = table.shape[1]
    td = _at(dev, table, offset)
    indd, lend = torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
    gd = None if glob is None else _at(dev, glob, glob_offset)
    out = _at(dev, np.empty((B, T, C), dtype=np.float32), out_offset, fill=float(POISON))
    rc = lib.get().msmc_units_embed_fwd(lib.ptr(indd), lib.ptr(lend), lib.ptr(td), lib.ptr(gd), lib.ptr(out), B, T, C, K, lib.stream(out))
    return rc, out.cpu().numpy()


def check_embed_forward(dev, s):
    B, T, C, K = FWD_SHAPES[s]
    ind, length, table, glob = embed_problem(B, T, C, K)
    ok = valid_rows(ind, length, K)
    if B * T > 20:
        assert (ind[np.arange(T)[None, :] < length[:, None]] == K).any() and (ind[np.arange(T)[None, :] < length[:, None]] == -1).any()
    for g in (glob, None):
        rc, out = embed_fwd(dev, ind, length, table, g, K)
        assert rc == 0
        assert np.isfinite(out).all(), 'the NaN row behind the table was read'
        assert not (out[~ok] != 0).any(), 'an invalid row is not zero'
        assert same_bits(out, restated_embed(ind, length, table, g, K)), (FWD_SHAPES[s], g is None)


def check_embed_forward_strided_grid(dev, B, T, C, K):
    """more 2048-piece blocks than the launcher's grid (8 per CU): workgroups stride over the blocks"""
    from msmctts_amd.hip import lib
    cus = 256 if lib.backend() != 'emu' else int(os.environ.get('MSMC_EMU_CUS', 3))
    assert (B * T * C // 4 + 2047) // 2048 > 8 * cus, 'the case does not reach the grid cap'
    ind, length, table, glob = embed_problem(B, T, C, K)
    rc, out = embed_fwd(dev, ind, length, table, glob, K)
    assert rc == 0 and same_bits(out, restated_embed(ind, length, table, glob, K))


def check_embed_forward_refusals(dev):
    from msmctts_amd.hip import units as hipunits
    for B, T, C, K in ((1, 4, 4, 3), (1, 4, 12, 3), (1, 4, 2056, 3), (1, 4, 0, 3), (1, 4, 8, 0), (0, 4, 8, 3), (1, 0, 8, 3)):
        ind, length = np.zeros((max(B, 1), max(T, 1)), dtype=np.int64), np.ones(max(B, 1), dtype=np.int64)
        table = np.ones((max(K, 1), max(C, 4)), dtype=np.float32)
        from msmctts_amd.hip import lib
        out = torch.full((max(B, 1), max(T, 1), max(C, 4)), float(POISON)).to(dev)
        td, indd, lend = torch.from_numpy(table).to(dev), torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
        rc = lib.get().msmc_units_embed_fwd(lib.ptr(indd), lib.ptr(lend), lib.ptr(td), None, lib.ptr(out), B, T, C, K, lib.stream(out))
        assert rc == E_SHAPE and bool((out.cpu() == POISON).all()), (B, T, C, K, rc)
    ind, length, table, glob = embed_problem(3, 63, 64, 100)
    for off in (dict(offset=1), dict(glob_offset=1), dict(out_offset=1), dict(offset=2, out_offset=2)):
        rc, out = embed_fwd(dev, ind, length, table, glob, 100, **off)         # four / eight bytes off a 16-byte boundary
        assert rc == E_SHAPE and (out == POISON).all(), off
    rc, out = embed_fwd(dev, ind, length, table, glob, 100, offset=4, glob_offset=4, out_offset=4)   # 16 bytes in: taken
    assert rc == 0 and same_bits(out, restated_embed(ind, length, table, glob, 100))
    with _raises(RuntimeError, 'msmc_units_embed_fwd failed with code -2'):
        hipunits.unit_embed(torch.zeros(1, 4, dtype=torch.int64).to(dev), torch.ones(1, dtype=torch.int64).to(dev),
                            torch.ones(3, 12).to(dev))


# ---- (c) embed backward ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backward_problem():
    """B = 6, T = 300, C = 16, K = 12: labels 1 .. 5 own 0, 1, 64, 65 and 200 valid rows, the rest is spread over 6 .. 11; the
    utterances have exactly 0, 1, 64, 65, 257 and 260 valid frames -- the invalid labels (-1 and K, 20 of each) all sit inside the
    prefix of the last utterance, so they disturb no other count.  Behind ``length`` the labels are valid ones"""
    B, T, C, K = 6, 300, 16, 12
    rng = np.random.default_rng(6300)
    length = np.array([0, 1, 64, 65, 257, T + 2], dtype=np.int64)
    ind = rng.integers(6, K, (B, T)).astype(np.int64)
    prefix = np.argwhere(np.arange(T)[None, :] < length[:, None])
    last = prefix[prefix[:, 0] == B - 1]
    pick = rng.permutation(len(last))
    for k, n, at in ((-1, 20, 0), (K, 20, 20)):
        for b, t in last[pick[at:at + n]]:
            ind[b, t] = k
    free = np.array([bt for bt in prefix if 0 <= ind[bt[0], bt[1]] < K])
    pick = rng.permutation(len(free))
    at = 0
    for k, n in ((2, 1), (3, 64), (4, 65), (5, 200)):
        for b, t in free[pick[at:at + n]]:
            ind[b, t] = k
        at += n
    ind[~(np.arange(T)[None, :] < length[:, None])] = 5
    gout = rng.standard_normal((B, T, C)).astype(np.float32)
    ok = valid_rows(ind, length, K)
    assert [int((ok & (ind == k)).sum()) for k in (1, 2, 3, 4, 5)] == [0, 1, 64, 65, 200]
    assert ok.sum(1).tolist() == [0, 1, 64, 65, 257, 260]
    return ind, length, gout


def restated_backward(ind, length, gout, K):
    B, T, C = gout.shape
    ok = valid_rows(ind, length, K).reshape(-1)
    lab = np.where(ok, ind.reshape(-1), -1)
    ulab = np.where(ok, np.repeat(np.arange(B), T), -1)
    return restated_stats(gout.reshape(B * T, C), lab, K)[0], restated_stats(gout.reshape(B * T, C), ulab, B)[0]


def embed_bwd(dev, ind, length, gout, K, with_glob=True, ws_bytes=None, g_offset=0, gtable_offset=0, gglob_offset=0, ws_offset=0):
    """msmc_units_embed_bwd directly on poisoned outputs -> (rc, gtable, gglob); ``*_offset``: that buffer starts so many floats
    into its allocation"""
    from msmctts_amd.hip import lib
    B, T, C = gout.shape
    gd = _at(dev, gout, g_offset)
    indd, lend = torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
    gtable = _at(dev, np.empty((K, C), dtype=np.float32), gtable_offset, fill=float(POISON))
    gglob = _at(dev, np.empty((B, C), dtype=np.float32), gglob_offset, fill=float(POISON))
    need = int(lib.get().msmc_units_embed_workspace(B * T, C, K))
    ws = torch.empty(max(need // 4, 4) + 8).to(dev)[ws_offset:]
    rc = lib.get().msmc_units_embed_bwd(lib.ptr(gd), lib.ptr(indd), lib.ptr(lend), lib.ptr(gtable), lib.ptr(gglob) if with_glob else None,
                                        lib.ptr(ws), need if ws_bytes is None else ws_bytes, B, T, C, K, lib.stream(gd))
    return rc, gtable.cpu().numpy(), gglob.cpu().numpy()


def check_embed_backward(dev):
    ind, length, gout = backward_problem()
    K = 12
    want_t, want_g = restated_backward(ind, length, gout, K)
    rc, gt, gg = embed_bwd(dev, ind, length, gout, K)
    assert rc == 0
    assert same_bits(gt, want_t), np.argwhere(gt != want_t)[:4].tolist()
    assert same_bits(gg, want_g), np.argwhere(gg != want_g)[:4].tolist()
    assert not gt[1].any() and not gt[0].any() and not gg[0].any(), 'a label or an utterance without rows is not +0'
    rc, gt2, gg2 = embed_bwd(dev, ind, length, gout, K)                        # the same inputs: the same bits
    assert rc == 0 and same_bits(gt2, gt) and same_bits(gg2, gg)
    rc, gt3, gg3 = embed_bwd(dev, ind, length, gout, K, with_glob=False)
    assert rc == 0 and same_bits(gt3, gt) and (gg3 == POISON).all()
    # invalid rows contribute nothing: NaN in their gradient changes no bit
    poisoned = gout.copy()
    poisoned[~valid_rows(ind, length, K)] = np.nan
    rc, gt4, gg4 = embed_bwd(dev, ind, length, poisoned, K)
    assert rc == 0 and same_bits(gt4, gt) and same_bits(gg4, gg)


def check_embed_backward_wide(dev):
    """C = 2048 (two channel blocks of the statistics kernel), K = 2000 > N"""
    B, T, C, K = 2, 70, 2048, 2000
    ind, length, _, _ = embed_problem(B, T, C, K)
    gout = np.random.default_rng(6310).standard_normal((B, T, C)).astype(np.float32)
    want_t, want_g = restated_backward(ind, length, gout, K)
    rc, gt, gg = embed_bwd(dev, ind, length, gout, K)
    assert rc == 0 and same_bits(gt, want_t) and same_bits(gg, want_g)


def check_embed_backward_refusals(dev):
    from msmctts_amd.hip import lib
    ind, length, gout = backward_problem()
    K = 12
    B, T, C = gout.shape
    need = int(lib.get().msmc_units_embed_workspace(B * T, C, K))
    assert need > 0 and need % 16 == 0
    from msmctts_amd.hip.lib import get
    own = 2 * ((8 * B * T + 15) // 16 * 16) + 16 * ((4 * max(K, B) + 15) // 16) + max(
        int(get().msmc_kmeans_stats_workspace(B * T, C, K)), int(get().msmc_kmeans_stats_workspace(B * T, C, B)))
    assert own <= need
    rc, gt, gg = embed_bwd(dev, ind, length, gout, K, ws_bytes=own - 1)
    assert rc == E_WORKSPACE and (gt == POISON).all() and (gg == POISON).all()
    rc, gt, gg = embed_bwd(dev, ind, length, gout, K, ws_bytes=own)
    assert rc == 0 and same_bits(gt, restated_backward(ind, length, gout, K)[0])
    for off in ('g_offset', 'gtable_offset', 'gglob_offset', 'ws_offset'):          # each four bytes off a 16-byte boundary
        rc, gt, gg = embed_bwd(dev, ind, length, gout, K, **{off: 1})
        assert rc == E_SHAPE and (gt == POISON).all() and (gg == POISON).all(), off
    rc, gt, gg = embed_bwd(dev, ind, length, gout, K, g_offset=4, gtable_offset=4, gglob_offset=4, ws_offset=4)   # 16 bytes in
    assert rc == 0 and same_bits(gt, restated_backward(ind, length, gout, K)[0])
    for C2, K2 in ((4, 12), (12, 12), (2056, 12), (16, 0)):
        assert int(lib.get().msmc_units_embed_workspace(B * T, C2, K2)) == 0
        g2 = np.zeros((B, T, max(C2, 4)), dtype=np.float32)
        from msmctts_amd.hip import lib as L
        gd, indd, lend = torch.from_numpy(g2).to(dev), torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev)
        gtable = torch.full((max(K2, 1), max(C2, 4)), float(POISON)).to(dev)
        ws = torch.empty(1024).to(dev)
        rc = L.get().msmc_units_embed_bwd(L.ptr(gd), L.ptr(indd), L.ptr(lend), L.ptr(gtable), None, L.ptr(ws), 4096, B, T, C2, K2, L.stream(gd))
        assert rc == E_SHAPE and bool((gtable.cpu() == POISON).all()), (C2, K2, rc)
    # N C 4 >= 2^32 is refused before anything is read
    assert int(lib.get().msmc_units_embed_workspace(1 << 20, 2048, 12)) == 0
    g = torch.zeros(64).to(dev)
    gi = torch.zeros(8, dtype=torch.int64).to(dev)
    rc = lib.get().msmc_units_embed_bwd(lib.ptr(g), lib.ptr(gi), lib.ptr(gi), lib.ptr(g), None, lib.ptr(g), 256, 1 << 10, 1 << 10, 2048, 12,
                                        lib.stream(g))
    assert rc == E_SHAPE and not bool(g.cpu().any())


def check_autograd(dev):
    """``torch.autograd.grad`` of a random projection of ``unit_embed`` is what the kernels give; ind and length get none"""
    from msmctts_amd.hip import units as hipunits
    ind, length, gout = backward_problem()
    K = 12
    B, T, C = gout.shape
    rng = np.random.default_rng(6320)
    table = torch.from_numpy(rng.standard_normal((K, C)).astype(np.float32)).to(dev).requires_grad_(True)
    glob = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).to(dev).requires_grad_(True)
    indd, lend, w = torch.from_numpy(ind).to(dev), torch.from_numpy(length).to(dev), torch.from_numpy(gout).to(dev)
    out = hipunits.unit_embed(indd, lend, table, glob)
    assert same_bits(out.detach().cpu().numpy(), restated_embed(ind, length, table.detach().cpu().numpy(), glob.detach().cpu().numpy(), K))
    gt, gg = torch.autograd.grad((out * w).sum(), (table, glob))
    want_t, want_g = restated_backward(ind, length, gout, K)
    assert same_bits(gt.cpu().numpy(), want_t) and same_bits(gg.cpu().numpy(), want_g)
    out = hipunits.unit_embed(indd, lend, table)                             # without glob
    gt2, = torch.autograd.grad((out * w).sum(), (table,))
    assert same_bits(gt2.cpu().numpy(), want_t)
    # through the table's GEMM to a linear layer, against the stock gather
    lin = torch.nn.Linear(8, C).to(dev)
    centers = torch.from_numpy(rng.standard_normal((K, 8)).astype(np.float32)).to(dev)
    ok = torch.from_numpy(valid_rows(ind, length, K)).to(dev)
    out = hipunits.unit_embed(indd, lend, lin(centers))
    g1 = torch.autograd.grad((out * w).sum(), (lin.weight, lin.bias))
    ref = torch.where(ok[:, :, None], lin(centers)[torch.where(ok, indd, 0)], torch.zeros((), device=dev))
    g2 = torch.autograd.grad((ref * w).sum(), (lin.weight, lin.bias))
    for a, b in zip(g1, g2):
        assert float((a - b).abs().max()) <= FP32_BAR * float(b.abs().max())


# ---- (d) model ------------------------------------------------------------------------------------------------------------------------
D, K_MODEL, N_MODEL, MEL = 32, 20, 64, 24          # (n_model_size and mel_dim: those of the small_ecapa_emb fixture)
VOCODER = dict(upsample_rates=[5, 4, 2], upsample_kernel_sizes=[11, 8, 4], upsample_initial_channel=32, resblock_kernel_sizes=[3, 7],
               resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]])


def model_config(path, global_encoder, decoder_config=None):
    fft = dict(max_seq_len=64, n_layers=2, n_head=2, d_k=8, d_v=8, d_inner=64, fft_conv1d_kernel=3, fft_conv1d_padding=1,
               dropout=0.0, attn_dropout=0.0, fused_layernorm=False)
    cfg = dict(_name='KMeansVQGANEmb', emb_dim=D, n_model_size=N_MODEL, quantizer_path=path, frame_decoder_config=fft, pred_mel=True,
               mel_dim=MEL, decoder_config=dict(VOCODER if decoder_config is None else decoder_config))
    if global_encoder:
        cfg['global_encoder_config'] = {'_name': 'ECAPA_TDNN'}
    return cfg


def centers_file(tmpdir):
    path = os.path.join(str(tmpdir), 'units.npy')
    centers = np.random.default_rng(6400).standard_normal((K_MODEL, D)).astype(np.float32)
    np.save(path, centers)
    return path, centers


def build_model(dev, tmpdir, global_encoder, seed=41):
    from msmctts_amd.networks import find_modules
    path, centers = centers_file(tmpdir)
    torch.manual_seed(seed)
    (_, m), = find_modules({'autoencoder': model_config(path, global_encoder)})
    return m.to(dev), centers


def rel_close(a, b, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err, top = float((a - b).abs().max()), float(b.abs().max())
    print('%s: max err %.3e, max %.3e' % (what, err, top))
    assert a.shape == b.shape and err <= FP32_BAR * top, '%s: max err %.3e against %.3e (bar %.0e relative)' % (what, err, top, FP32_BAR)


def check_model(dev, tmpdir, global_encoder):
    m, centers = build_model(dev, tmpdir, global_encoder)
    m.eval()
    B, T = 3, 24
    gen = torch.Generator().manual_seed(42)
    ind = torch.randint(0, K_MODEL, (B, T), generator=gen)
    mel = torch.randn(B, T, MEL, generator=gen).to(dev)
    emb = torch.from_numpy(centers)[ind].to(dev)
    ind = ind.to(dev)
    assert tuple(m.unit_table().shape) == (K_MODEL, N_MODEL) and m.unit_table().requires_grad
    table64 = torch.from_numpy(centers).double() @ m.in_linear.weight.detach().double().cpu().t() + m.in_linear.bias.detach().double().cpu()
    for lengths in ((24, 17, 5), (T, T, T)):
        length = torch.tensor(lengths, dtype=torch.int64).to(dev)
        valid = (torch.arange(T)[None, :] < length.cpu()[:, None])
        with torch.no_grad():
            of, ou = m(emb, length, mel=mel), m.forward_units(ind, length, mel=mel)
            assert set(of) == set(ou) == {'encoder_indices', 'mel_outputs', 'decoder_outputs'}
            assert isinstance(ou['encoder_indices'], tuple) and len(ou['encoder_indices']) == 1
            assert torch.equal(of['encoder_indices'][0], ou['encoder_indices'][0]) and torch.equal(ou['encoder_indices'][0], ind)
            # the decoder input of both paths against float64
            glob = m.global_encoder(mel) if global_encoder else None
            want = table64[ind.cpu()] + (glob.double().cpu().unsqueeze(1) if global_encoder else 0.0)
            frames = m.in_linear(emb) + (glob.unsqueeze(1) if global_encoder else 0.0)
            units = m._embed_units(ind, length, mel)
            rel_close(frames[valid], want[valid], 'decoder input, frame path')
            rel_close(units[valid], want[valid], 'decoder input, unit path')
            assert not bool(units[~valid].any()), 'padded rows of the unit path are zeros'
            for b in range(B):
                n = lengths[b]
                rel_close(ou['mel_outputs'][b, :n], of['mel_outputs'][b, :n], 'mel_outputs, valid rows of utterance %d' % b)
            if min(lengths) == T:
                rel_close(ou['decoder_outputs'], of['decoder_outputs'], 'decoder_outputs')
                rel_close(ou['mel_outputs'], of['mel_outputs'], 'mel_outputs')
            o = m.forward_units(ind, length, mel=mel, window=None)
            assert set(o) == {'encoder_indices', 'mel_outputs'}
            win = [(0, 2, 6), (2, 0, 4)]
            a, b_ = m(emb, length, mel=mel, window=win), m.forward_units(ind, length, mel=mel, window=win)
            assert a['decoder_outputs'].shape == b_['decoder_outputs'].shape
    # gradients from a scalar loss, all lengths T; training mode (no dropout in this configuration): the vocoder in evaluation
    # mode runs on folded weights that carry no gradient
    m.train()
    length = torch.full((B,), T, dtype=torch.int64).to(dev)
    w1 = torch.randn(of['decoder_outputs'].shape, generator=gen).to(dev)
    w2 = torch.randn(of['mel_outputs'].shape, generator=gen).to(dev)
    voc = dict(m.decoder.named_parameters())['conv_pre.weight_v']
    params = (m.in_linear.weight, m.in_linear.bias, voc)

    def grads(o):
        # (.backward and .grad: the vocoder's kernels hand their weight gradients to .grad themselves)
        m.zero_grad(set_to_none=True)
        ((o['decoder_outputs'] * w1).sum() + (o['mel_outputs'] * w2).sum()).backward()
        return [p.grad.detach().clone() for p in params]
    gf, gu = grads(m(emb, length, mel=mel)), grads(m.forward_units(ind, length, mel=mel))
    for name, a, b_ in zip(('in_linear.weight', 'in_linear.bias', 'a vocoder weight'), gu, gf):
        assert float(b_.abs().max()) > 0
        rel_close(a, b_, 'gradient of ' + name)


def check_synthesis_units(dev, tmpdir, global_encoder=True):
    """runs against the labels they expand to: bit for bit; eval returns the waveform, training mode the dictionary"""
    from msmctts_amd.hip import units as hipunits
    m, _ = build_model(dev, tmpdir, global_encoder)
    m.eval()
    B, T = 3, 24
    gen = torch.Generator().manual_seed(43)
    ind = torch.repeat_interleave(torch.randint(0, K_MODEL, (B, T), generator=gen), 3, dim=1)[:, :T].contiguous().to(dev)
    length = torch.tensor([24, 17, 5], dtype=torch.int64).to(dev)
    ref = torch.randn(B, 30, MEL, generator=gen).to(dev) if global_encoder else None
    units, dur, ulen = hipunits.collapse_units(ind, length)
    with torch.no_grad():
        a = m.synthesis_units(ind, length, ref=ref)
        b = m.synthesis_units(units, ref=ref, dur=dur, ulen=ulen)
        assert a.dim() == 3 and a.shape[0] == B and a.shape[1] == T * 40 and torch.equal(a, b)
        full = m.synthesis_units(ind[:1], ref=None if ref is None else ref[:1])            # length None: every frame
        assert torch.equal(full, m.synthesis_units(ind[:1], torch.tensor([T]).to(dev), ref=None if ref is None else ref[:1]))
        m.train()
        out = m.synthesis_units(ind, length, ref=ref)
        assert set(out) == {'decoder_outputs', 'mel_outputs'}


# ---- (e) trainer, dataset, synthetic batch -----------------------------------------------------------------------------------------------
def check_trainer_phase(dev, tmpdir, phase):
    import _embcases as E
    from msmctts_amd import synthetic
    from msmctts_amd.tasks import build_task
    from msmctts_amd.utils.config import Config
    path, centers = centers_file(tmpdir)
    base = E.config(False)
    ae = model_config(path, True, decoder_config=dict(base.task.autoencoder.decoder_config))
    cfg = Config({'id': 'small_units', 'task': {'_name': 'NASynTTSEmb', 'autoencoder': ae, 'discriminator': base.task.discriminator},
                  'trainer': dict(E.TRAINER), 'optimizer': {'_default': dict(E.OPT)},
                  'dataset': dict(samplerate=24000, feature=['units', 'mel', 'wav'], frameshift=[E.HOP, E.HOP, 1])})
    torch.manual_seed(51)
    task = build_task(cfg, mode='train').to(dev).train()
    tr = E._trainer(cfg, task, seed=300 + phase)
    iteration = E.PHASE_ITERATION[phase]
    assert tr._phase(iteration) == phase
    batch = synthetic.make_unit_batch(batch_size=3, frames=24, n_units=K_MODEL, mel_dim=MEL, hop=E.HOP, seed=52, device=dev)
    assert set(batch) == {'units', 'units_length', 'mel', 'wav', 'wav_length', 'units_length_host'}
    before = {k: v.detach().clone() for k, v in task.state_dict().items()}
    task.zero_grad()
    log = tr.train_step(batch, iteration)
    expect = {'frame_loss'} | ({'stft_loss'} if phase > 0 else set())
    expect |= {'d_loss_real', 'd_loss_fake', 'd_loss', 'fm_loss', 'adv_loss', 'g_loss'} if phase == 2 else set()
    assert set(log['loss']) == expect, sorted(log['loss'])                  # the keys of the frame path (tests/_kmeanscases.py)
    for k, v in log['loss'].items():
        assert np.isfinite(float(v)), (k, float(v))
    after = task.state_dict()
    moved = {k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k])}
    assert 'autoencoder.in_linear.weight' in moved, sorted(moved)[:8]
    k = 'autoencoder.quantizer.quantizer.0.embed'
    assert torch.equal(after[k].cpu(), torch.from_numpy(centers).t())


def check_trainer_needs_forward_units(dev):
    import _embcases as E
    from msmctts_amd import synthetic
    cfg, task = E.build(dev, False)
    tr = E._trainer(cfg, task, seed=7)
    batch = synthetic.make_unit_batch(batch_size=3, frames=24, n_units=16, mel_dim=E.MEL_DIM, hop=E.HOP, seed=53, device=dev)
    with _raises(TypeError, 'MSMCVQGANEmb'):
        tr.train_step(batch, E.PHASE_ITERATION[0])


def check_unit_batch_and_collation():
    """CPU, no kernels: ``make_unit_batch`` and ``EmbDataset.collate_fn`` on items without ``emb``"""
    from msmctts_amd import synthetic
    from msmctts_amd.datasets.emb_dataset import EmbDataset
    b = synthetic.make_unit_batch(batch_size=4, frames=20, n_units=7, mel_dim=8, hop=5, seed=3)
    e = synthetic.make_emb_batch(batch_size=4, frames=20, emb_dim=6, mel_dim=8, hop=5, seed=3)
    assert b['units'].dtype == torch.int64 and tuple(b['units'].shape) == (4, 20) and b['units_length'].dtype == torch.int64
    assert torch.equal(b['units_length'], e['emb_length']) and b['units_length_host'] == b['units_length'].tolist()
    assert int(b['units_length'].max()) == 20 and b['units_length'].tolist() == sorted(b['units_length'].tolist(), reverse=True)
    valid = torch.arange(20)[None, :] < b['units_length'][:, None]
    assert bool((b['units'][~valid] == -1).all()) and int(b['units'][valid].min()) >= 0 and int(b['units'][valid].max()) < 7
    assert bool((b['mel'][~valid] == -4).all()) and torch.equal(b['wav_length'], b['units_length'] * 5)
    assert tuple(b['mel'].shape) == (4, 20, 8) and tuple(b['wav'].shape) == (4, 100, 1)
    ds = EmbDataset.__new__(EmbDataset)
    ds.padding_value, ds.frameshift = {'units': -1, 'mel': -4, 'wav': 0}, {'units': 4, 'mel': 4, 'wav': 1}
    rng = np.random.default_rng(1)
    items = [{'units': rng.integers(0, 9, n).astype(np.int64), 'mel': rng.standard_normal((n, 8)).astype(np.float32),
              'wav': rng.standard_normal((4 * n, 1)).astype(np.float32)} for n in (3, 7, 5)]
    out = ds.collate_fn(items)
    assert set(out) == {'units', 'units_length', 'mel', 'mel_length', 'wav', 'wav_length'}
    assert out['units_length'].tolist() == [7, 5, 3] == out['mel_length'].tolist() and out['units'].dtype == torch.int64
    for row, src in enumerate((1, 2, 0)):
        n = len(items[src]['units'])
        assert torch.equal(out['units'][row, :n], torch.from_numpy(items[src]['units'])) and bool((out['units'][row, n:] == -1).all())
        assert torch.equal(out['mel'][row, :n], torch.from_numpy(items[src]['mel'])) and bool((out['mel'][row, n:] == -4).all())
    # the device loader hands the unit lengths along on the host, as it does for ``emb_length``
    from msmctts_amd.datasets import DeviceLoader
    up = next(iter(DeviceLoader([out], 'cpu')))
    assert up['units_length_host'] == [7, 5, 3] and 'emb_length_host' not in up and torch.equal(up['units'], out['units'])


# ---- (f) tool -------------------------------------------------------------------------------------------------------------------------
def check_tool(dev, tmpdir):
    """tools/synthesize_units.py (in process) on files in the format of tools/extract_units.py: the ``indices/`` form and the
    ``units/`` + ``durations/`` form write the same waveform bit for bit, with --jobs 3 (one launch) and --jobs 1"""
    from msmctts_amd.tasks import build_task
    from msmctts_amd.utils.config import Config
    import _embcases as E
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('synthesize_units_tool', os.path.join(root, 'tools', 'synthesize_units.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tmp = str(tmpdir)
    path, _ = centers_file(tmpdir)
    base = E.config(False)
    cfg = Config({'id': 'small_units', 'task': {'_name': 'NASynTTSEmb', 'autoencoder': model_config(path, True),
                                                'discriminator': base.task.discriminator},
                  'trainer': dict(E.TRAINER), 'optimizer': {'_default': dict(E.OPT)},
                  'dataset': dict(samplerate=16000, feature=['units', 'mel', 'wav'], frameshift=[40, 40, 1])})
    torch.manual_seed(61)
    task = build_task(cfg, mode='train').to(dev)
    rng = np.random.default_rng(6500)
    for kind in ('indices', 'units', 'durations', 'mel'):
        os.makedirs(os.path.join(tmp, kind))
    labels = {'a': np.repeat(rng.integers(0, K_MODEL, 9), rng.integers(1, 4, 9)).astype(np.int64),
              'b': np.array([4], dtype=np.int64), 'c': np.repeat(rng.integers(0, K_MODEL, 5), 3).astype(np.int64)}
    with open(os.path.join(tmp, 'ids.list'), 'w') as f:
        for name, row in labels.items():
            starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
            np.save(os.path.join(tmp, 'indices', name + '.npy'), row)
            np.save(os.path.join(tmp, 'units', name + '.npy'), row[starts])
            np.save(os.path.join(tmp, 'durations', name + '.npy'), np.diff(np.r_[starts, len(row)]).astype(np.int32))
            np.save(os.path.join(tmp, 'mel', name + '.npy'), rng.standard_normal((12, MEL)).astype(np.float32))
            f.write('%s spk0\n' % name)
    common = ['--ref', os.path.join(tmp, 'mel', '{0}.npy'), '--device', dev]
    waves = {}
    for form, jobs in (('indices', 3), ('runs', 3), ('indices', 1), ('runs', 1)):
        out = os.path.join(tmp, 'wav_%s_%d' % (form, jobs))
        pattern = [os.path.join(tmp, 'indices', '{0}.npy')] if form == 'indices' else [
            os.path.join(tmp, 'units', '{0}.npy'), '--durations', os.path.join(tmp, 'durations', '{0}.npy')]
        tool.main([os.path.join(tmp, 'ids.list')] + pattern + ['-o', out, '--jobs', str(jobs)] + common, task=task)
        assert sorted(os.listdir(out)) == ['a.wav', 'b.wav', 'c.wav']
        for name, row in labels.items():
            with wave.open(os.path.join(out, name + '.wav'), 'rb') as w:
                assert w.getframerate() == 16000 and w.getnframes() == 40 * len(row), (name, w.getnframes())
                waves[form, jobs, name] = w.readframes(w.getnframes())
    for name in labels:
        for jobs in (3, 1):                     # (across --jobs the padded width differs: not compared)
            assert waves['indices', jobs, name] == waves['runs', jobs, name], (name, jobs)
            assert any(waves['indices', jobs, name])


# ---- (g) feature presence ---------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'msmc_hip.h')) as f:
        header = f.read()
    for name in ('msmc_units_total', 'msmc_units_expand', 'msmc_units_embed_fwd', 'msmc_units_embed_workspace', 'msmc_units_embed_bwd'):
        assert name + '(' in header, name
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansVQGANEmb, expand_units, unit_embed  # noqa: F401
    from msmctts_amd.synthetic import make_unit_batch  # noqa: F401
    assert all(callable(getattr(KMeansVQGANEmb, name)) for name in ('unit_table', 'forward_units', 'synthesis_units'))
    assert os.path.isfile(os.path.join(root, 'tools', 'synthesize_units.py'))
