"""Shared cases of the kernels of csrc/wnorm.hip through the C entries -- weight-norm prepare (msmc_wn_prepare_multi, _multi_tiled,
_multi_tiles), weight-norm backward (msmc_wn_backward_multi_rows, _acc, _multi), column sums (msmc_colsum_ws, msmc_colsum), the
reflect-padding fold (msmc_reflect_fold, msmc_reflect_fold_multi / _res / _tap) and the leaky-ReLU backward (msmc_lrelu_bwd,
msmc_lrelu_bwd_multi) -- and of one pass through the host layer (hip/conv.py, hip/convnet.py): tests/test_wnorm_emu.py runs them on
the kernel interpreter, tests/test_gpu_wnorm.py on the GPU.

Reference of every comparison: stock torch operators on the CPU in float64 (norm, *, /, sum, F.pad(mode='reflect'), where) from the
same fp32 / bf16 input bits, and their float64 autograd gradients.  No reference restates a kernel's lane or index arithmetic; the
positions of a weight image are those of the ABI, dst[t * s[0] + a * s[1] + b * s[2]].  Every output is pre-filled with NaN and none
may remain in the part the entry owns; GUARD NaN elements behind every output, and every gap of a padded layout or between privatised
copies, must keep their bits (the weight images of one prepare call lie in one buffer with 2^18 NaN elements behind the last, so
that a stray store is found by a comparison and not by the operating system); every case runs twice and the two results agree bit for bit (but for the atomic msmc_colsum).

Bars (u = 2^-24; h(r) = half a bf16 ulp of the float64 reference r, added wherever the output is bf16; ONE = 1 + 2^-20):
  prepare, backward   the project's yardstick rule (tests/_normcases.py), per quantity (w in each layout, inv_norm; gv, gg, gb), in the
                  max norm and in the L2 norm: the error against float64 is at most RATIO = 4 x the error of the same chain written
                  with elementary fp32 torch operators on the CPU (v * v, sum, sqrt, /, *; the copies folded in order, (dw * v).sum,
                  dot * inv, g * inv, k1 * (dw - v * k2)).  The backward is fed inv_norm = fp32(1 / ||v||_float64); the chain uses
                  the same fp32 value, so its u is in the bar.
  ... or a floor  where torch's chain is exact (its error is 0) the rule is no bar; such a comparison, and the ones listed by name
                  in FLOOR_HELD, pass only if EVERY element lies inside the rounding-count floor.  A sum of a row of n parameters
                  passes through at most c = ceil(n / NT) + 3 additions in a work-item (NT = 256 work-items, 128 in the short-row
                  backward; + 3: the four-element vector steps), 6 butterfly steps and 3 LDS additions: D(n) = c + 9.
                      ss       relative D u (every term is positive)
                      inv_norm sqrtf, the quotient: (D / 2 + 2) u / ||v||
                      w        g * inv_norm (or g / norm), v * scale: (D / 2 + 4) u |w|
                  Backward, with S = the in-order fold of the R copies, e_S = (R - 1) u sum_r |dw_r|, inv within u of 1 / ||v||:
                      dot      E_d = D u sum |S v| + sum e_S |v|
                      gg       E_d inv + 2 u |dot inv|
                      k2       E_k = E_d inv^2 + 4 u |k2|           (two inv, two products)
                      gv       k1 (e_S + |v| E_k + u |v k2| + u (|S| + |v k2|)) + 3 u k1 (|S| + |v k2|)
                               -- S - v k2 cancels, hence the absolute terms in sum |dw v| and ||v|| instead of |gv|
                      gb       (R + 1) u (sum_r |db_r| + |pre|)         (R - 1 additions of the fold, one under accumulate)
                  and one more u (|pre| + |result|) where accumulate adds gv / gg to a pre-set gradient.  All times ONE.
  plain items     bit equality: w == v (rounded once to bf16), gv == the in-order fp32 fold of the copies (pre + fold under
                  accumulate); inv_norm / gg keep the bits they had.
  consumed dw/db  +0 bit for bit in every copy; every other element of those buffers keeps its bits.
  column sums     (rows - 1) u sum_rows |g| per column, times ONE: any order of rows - 1 fp32 additions of inputs that are exact in
                  fp32.  Under accumulate the entry makes one addition more, out = pre + sum, and pre is one addend more: the same
                  bar over rows + 1 addends and rows additions, rows u (sum_rows |g| + |pre|) ONE.  That is what the pre-set addend
                  costs and nothing else: without accumulate the bar stays (rows - 1) u sum_rows |g| ONE.  msmc_colsum_ws
                  is bit-reproducible; the atomic msmc_colsum is held to the same bar without the run-twice equality.  A view that
                  starts one element into its buffer leaves the vector branch: the same bar, and bit equality with the aligned
                  call at rows = 1 (no addition at all).
  reflect fold    up to nine addends, one product, one more addition: (8 + 2) u (sum |addends| + |res|) + h(ref).
  leaky ReLU      bit equality with where(y > 0, g, g * slope) computed in fp32 and rounded once to the storage type.
  host route      conv.colsum / conv.reflect_fold / the groups: the bars above.  The weight-normalised layer through ConvBank:
                  dW is the bank's own weight gradient, a sum of K = B * L products per element in fp32: e_S = (K + 2) u sum |x| |gy|
                  (a product within 2 u, K - 1 additions, one more into the accumulator); the backward floor above with that e_S,
                  R = 1, and one more u for inv_norm (the kernel's own, within (D / 2 + 2) u of 1 / ||v||: k1, k2, gg get
                  (D / 2 + 2) u |.| per factor inv on top).  Bias gradient: K u sum |gy|.

Which case reaches which path / instantiation (P n = item n of PREP_ITEMS, S n / G n = item n of BW_SMALL / BW_LARGE):
  wn_prepare_kernel       every P through msmc_wn_prepare_multi (both layouts; padded strides: gaps keep NaN) and _multi_tiled
                          (layout 1, skip2); vector sum of squares P2, P7, P8, P9 (n % 4 == 0, P9: 1040 > 1024 elements, a second
                          vector step), scalar P0, P1, P3, P4, P6; plain P5, P10
  wn_transpose_kernel     every P with dst2 through _multi_tiled; P6 (no dst2) owns no tile-block
  wn_norm_kernel          _multi_tiles: the weight-normalised P (row_item / norm_rows; 1-row items P3, P4, P5 next to each other)
  wn_layout_kernel        tile rule T = 1: P0, P3 (128 columns: Bc = 129 ends one column into the second tile); T = 2: P1 (64: Bc = 65);
                          T <= 4: P4 (3), P6, P9 (4), P10 (3); T > 4: P2 (5, Bc = 36 past 32), P5 (7), P7 (11), P8 (16: 65 664 bytes
                          of LDS, msmc_allow_lds); rows past a tile P0 (65), P1 (100), P2 (33), P10 (68)
    layout 2 stores       A % 4 == 0 four-row vectors: P1, P6 (no dst2: skipped), P7, P10; A % 4 != 0 elements: P0, P2, P3, P4, P5,
                          P8, P9.  The (b, t) carry after t += rs: P10 (T = 3, step 16), P7 (T = 11, step 32), P2 (T = 5, step 8)
    layout 1 stores       Bc % 4 == 0 four-column vectors: P2, P5, P7, P9, P10; elements: P0, P1, P3, P4, P6, P8
    tile_item             given, and NULL (wn_find_tile)
  wn_backward_kernel      128 work-items, buffer 4032: BW_SMALL at max_row = 4000; 256 work-items, buffer 6144: BW_SMALL at max_row = 0
                          (through _acc and _multi too), BW_LARGE at max_row = 7175
    staged, R = 1         S0 (n = 15 < NT, 3 steps), S1 (Bc = 129 > 128, 8 steps; n = 516 > 4 NT), S5, S6 (n = 4000); G2 (Bc = 300 >
                          256, 6 steps), G6
    staged, R in 2 .. 8   S2 (R = 2, n = 511 < 4 NT), S3 (R = 8, plain); G3 (R = 2, n = 1020 < 4 NT), G4 (R = 8, n = 1028 > 4 NT)
    staged, R > 8         S4 (R = 9), G5 (R = 9, plain)
    unstaged (n > 6144)   G0 (R = 1), G1 (R = 3), G7 (R = 2, plain)
    bias                  db == NULL S3, G1, G6; nbias == A S0, S4, S6, G0, G4, G5; nbias == 2 A S1, S5, G2; nbias < A S2, G3
    accumulate            0 and 1 on every table
  colsum_part_kernel      vector branch: fp32 C = 4, 8, 64, 256, 1024, bf16 C = 8, 64, 256, 1024, 2048; whole-column branch: C = 3, 24,
                          80, 257, 513 and every vector C on a view one element into its buffer; C-divides-256 branch: fp32 C = 1, 2,
                          bf16 C = 1, 2, 4.  rows = 1, 127, 128, 129, 257 at C <= 257; C = 513: 1, 129; C >= 1024: 1, 33 (to stay
                          below 100 000 elements).  rows = 32 897 > 256 * 128: the block cap binds and all 256 blocks own rows;
                          rows = 32 769 = colsum_fewer(): the smallest row count for which fewer blocks own rows (255) than are
                          launched (256), found from the launcher's arithmetic -- below the cap every block owns rows.  Both at
                          C = 4 fp32 (vector), C = 3 bf16 (whole-column) and C = 2 fp32 (C-divides-256).
  colsum_final_kernel     slices > 1 (C < 256) and 1; more than one workgroup (C = 257, 513, 1024, 2048)
  colsum_kernel (atomic)  whole-column C = 3, 257; C-divides-256 C = 4, 64
  reflect_fold_multi_kernel  <float, 4>: C = 4, 8, 12, 32; <float, 2>: C = 2, 6, the group (8, 12, 6), a member two elements into
                          its buffer; <float, 1>: C = 1, the group (8, 4, 1), a member one element in; <bf16, 8>: C = 8, 32;
                          <bf16, 4>: C = 4, 12; <bf16, 2>: C = 2, 6, (8, 12, 6), two elements in; <bf16, 1>: C = 1, (8, 4, 1), one in.
                          (Seven instantiations exist: the launcher's <float, 2> branch appears twice in the source.)
                          Past the grid cap: C = 1 with more than 16 * CUs * 256 items.
  reflect_fold_kernel     the first member of every group, bit-equal to a one-member group; past 4096 * 256 elements
  lrelu_bwd_multi_kernel  <T, VEC>: n = 4 (fp32), 8, 5000 (fp32 and bf16), the groups whose members are all whole vectors;
                          <T, 1>: n = 1, 3, 7, 1023, 1025, a group with one member of n % VEC != 0, views at element offset 1
  lrelu_bwd_kernel        every n
each in fp32 and in bf16.  Every comparison is appended to MEASURED and printed; the figures are recorded in
profiles/wnorm_direct.md.
"""
import ctypes
import math
import os

import torch
import torch.nn.functional as F_

from _spectralcases import _nan, same_bits, twice
from _normcases import U, E_SHAPE, E_WORKSPACE, GUARD, DTYPES, half_ulp, Out, at, L, gen_for
import _normcases

ONE = 1.0 + 2.0 ** -20
MEASURED = []          # (what, case, figure, how it was held)
# comparisons that may miss 4 x and be held by the rounding-count floor (profiles/wnorm_direct.md says why); any other comparison may
# use the floor only where the yardstick is no bar at all (torch's chain is exact: its error is 0)
FLOOR_HELD = set()
BOOK = (MEASURED, FLOOR_HELD, 'wnorm')
SLOPE = 0.1


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def held(what, case, got, ref, bound):
    """tests/_normcases.py held, recorded in this module's MEASURED"""
    _normcases.held(what, case, got, ref, bound, book=BOOK)


def yard(what, case, got, t32, ref, floor, half=None):
    """tests/_normcases.py yard (the yardstick rule, RATIO = 4), with this module's MEASURED and FLOOR_HELD"""
    _normcases.yard(what, case, got, t32, ref, floor, half, book=BOOK)


def dev_table(items, dev):
    return torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)


def kept(buf, idx, what):
    """every element of the NaN-filled ``buf`` (on the CPU) outside ``idx`` still has its bits"""
    rest = torch.ones(buf.numel(), dtype=torch.bool)
    rest[idx.reshape(-1)] = False
    assert same_bits(buf[rest], _nan((int(rest.sum()),), 'cpu', buf.dtype)), '%s: an element outside the image was written' % what


def all_nan(t):
    return same_bits(t, _nan(t.shape, 'cpu', t.dtype))


def seed_of(key):
    return sum(ord(c) * (i + 1) for i, c in enumerate(str(key)))


def d_sum(n, nt=256):
    return (n + nt - 1) // nt + 3 + 9


# ---- 1: weight-norm prepare ----------------------------------------------------------------------------------------------------------
# (A, Bc, T, weight-normalised, dst2)
PREP_ITEMS = ((65, 129, 1, True, True), (100, 65, 2, True, True), (33, 36, 5, True, True), (1, 1, 1, True, True),
              (1, 2, 3, True, True), (1, 4, 7, False, True), (4, 2, 4, True, False), (8, 40, 11, True, True),
              (3, 3, 16, True, True), (2, 260, 4, True, True), (68, 8, 3, False, True))
PREP_ENTRIES = ('multi', 'multi padded', 'tiled', 'tiles', 'tiles searched')


def prep_strides(A, Bc, T, padded):
    if padded:
        return (A * (2 * Bc + 3) + 5, 2 * Bc + 3, 2), (Bc * (3 * A + 1) + 2, 3, 3 * A + 1)
    return (A * Bc, Bc, 1), (A * Bc, 1, A)


def image_index(A, Bc, T, s):
    """position of w[a][b][t] in a weight image: t * s[0] + a * s[1] + b * s[2] (include/msmc_hip.h)"""
    a, b, t = torch.meshgrid(torch.arange(A), torch.arange(Bc), torch.arange(T), indexing='ij')
    return t * s[0] + a * s[1] + b * s[2]


def prep_inputs(specs):
    vs, gs = [], []
    for i, (A, Bc, T, _, _) in enumerate(specs):
        gen = gen_for(4000, i, A, Bc, T)
        vs.append(torch.randn(A, Bc, T, generator=gen))
        gs.append(torch.rand(A, generator=gen) + 0.5)
    return vs, gs


def tile_blocks(entry, A, Bc, T, two):
    if entry == 'tiled':
        return ((A + 63) // 64) * ((Bc + 15) // 16) if two else 0
    return int(L().get().msmc_wn_tile_blocks(A, Bc, T)) if entry.startswith('tiles') else 0


def prep_call(entry, items, n, blk, tblk, max_taps, dev, like):
    """-> return code of the entry over a host item table"""
    from msmctts_amd.hip import convnet
    lib = L()
    table = dev_table(items, dev)
    st = lib.stream(like)
    if entry.startswith('multi'):
        return lib.get().msmc_wn_prepare_multi(lib.ptr(table), n, blk, st)
    if entry == 'tiled':
        return lib.get().msmc_wn_prepare_multi_tiled(lib.ptr(table), n, blk, tblk, st)
    flat, o_norm, n_norm, o_tile = convnet._wn_maps(items, torch.device(dev))
    base = flat.data_ptr()
    return lib.get().msmc_wn_prepare_multi_tiles(lib.ptr(table), n, blk, tblk, max_taps, ctypes.c_void_p(base),
                                                 ctypes.c_void_p(base + 4 * o_norm), n_norm,
                                                 ctypes.c_void_p(base + 4 * o_tile) if entry == 'tiles' else None, st)


PREP_SLACK = 1 << 18


def prep_table(dev, specs, vd, gd, which, entry):
    """-> host item table over fresh NaN-filled images, [(w1, w2 | None, inv_norm)], rows, tile-blocks, slack.  The images (each
    with its GUARD, starting at a multiple of eight elements) lie one behind the other in ONE buffer with PREP_SLACK NaN elements
    behind the last: a store that strays past its own image (a walk of (b, t) that runs on) lands in another image, a guard or
    the slack, where the comparisons find it, not in unmapped memory"""
    lib = L()
    code, dtype, _ = DTYPES[which]
    padded = entry.endswith('padded')
    items = (lib.WnItem * len(specs))()
    spans = []
    for A, Bc, T, _, two in specs:
        s1, s2 = prep_strides(A, Bc, T, padded)
        spans.append((int(image_index(A, Bc, T, s1).max()) + 1 + GUARD, int(image_index(A, Bc, T, s2).max()) + 1 + GUARD if two else 0))
    pad8 = lambda n: (n + 7) // 8 * 8
    total = sum(pad8(a) + pad8(b) for a, b in spans)
    arena = _nan((total + PREP_SLACK,), dev, dtype)
    bufs, blk, tblk, o = [], 0, 0, 0
    for it, (A, Bc, T, normed, two), v, g, (n1, n2) in zip(items, specs, vd, gd, spans):
        s1, s2 = prep_strides(A, Bc, T, padded)
        w1 = arena[o:o + n1]
        w2 = arena[o + pad8(n1):o + pad8(n1) + n2] if two else None
        o += pad8(n1) + pad8(n2)
        inv = _nan((A + GUARD,), dev)
        it.v, it.g = v.data_ptr(), (g.data_ptr() if normed else None)
        it.dst1, it.dst2, it.inv_norm = w1.data_ptr(), (w2.data_ptr() if two else None), inv.data_ptr()
        it.A, it.Bc, it.T, it.dtype, it.block0, it.tblock0 = A, Bc, T, code, blk, tblk
        for k in range(3):
            it.s1[k], it.s2[k] = s1[k], s2[k]
        blk += A
        tblk += tile_blocks(entry, A, Bc, T, two)
        bufs.append((w1, w2, inv))
    return items, bufs, blk, tblk, arena[total:]


def check_prepare(dev, which, entry, specs=PREP_ITEMS):
    code, dtype, name = DTYPES[which]
    vs, gs = prep_inputs(specs)
    vd, gd = [v.to(dev) for v in vs], [g.to(dev) for g in gs]

    def run():
        items, bufs, blk, tblk, slack = prep_table(dev, specs, vd, gd, which, entry)
        assert prep_call(entry, items, len(specs), blk, tblk, max(s[2] for s in specs), dev, vd[0]) == 0
        return tuple(t.cpu() if t is not None else torch.zeros(0) for b in bufs for t in b) + (slack.cpu(),)

    got = twice(run)
    assert all_nan(got[-1]), 'an element behind the last image was written'
    for i, ((A, Bc, T, normed, two), v, g) in enumerate(zip(specs, vs, gs)):
        w1, w2, inv = got[3 * i:3 * i + 3]
        tag = 'P%d %dx%dx%d %s %s' % (i, A, Bc, T, name, entry)
        v64, n = v.double(), Bc * T
        norm = v64.reshape(A, -1).norm(dim=1)
        w64 = v64 * (g.double() / norm)[:, None, None] if normed else v64
        nrm32 = (v * v).reshape(A, -1).sum(1).sqrt()
        w32 = v * (g / nrm32)[:, None, None]
        f_w = (d_sum(n) / 2.0 + 4) * U * w64.abs() * ONE
        assert same_bits(inv[A:], _nan((GUARD,), 'cpu')), tag + ': a guard of inv_norm was overwritten'
        if normed:
            yard('prepare inv_norm', tag, inv[:A], 1.0 / nrm32, 1.0 / norm, (d_sum(n) / 2.0 + 2) * U / norm * ONE)
        else:
            assert all_nan(inv), tag + ': inv_norm of a plain item was written'
        for k, (buf, s) in enumerate(zip((w1, w2), prep_strides(A, Bc, T, entry.endswith('padded')))):
            if k == 1 and not two:
                continue
            idx = image_index(A, Bc, T, s)
            kept(buf, idx, '%s layout %d' % (tag, k + 1))
            w = buf[idx.reshape(-1)].view(A, Bc, T)
            if normed:
                yard('prepare w layout %d' % (k + 1), tag, w, w32, w64, f_w, half_ulp(w64, dtype))
            else:
                assert same_bits(w, v.to(dtype)), '%s layout %d: a plain weight is not v' % (tag, k + 1)


def check_prepare_refusals(dev):
    """every condition of the three entries that returns MSMC_E_SHAPE; nothing is written"""
    from msmctts_amd.hip import convnet
    lib = L()
    specs = ((5, 8, 3, True, True), (3, 4, 1, False, True))
    vs, gs = prep_inputs(specs)
    vd, gd = [v.to(dev) for v in vs], [g.to(dev) for g in gs]
    seen = []
    for entry in ('multi', 'tiled', 'tiles'):
        items, bufs, blk, tblk, slack = prep_table(dev, specs, vd, gd, 0, entry)
        table = dev_table(items, dev)
        tp, st, n = lib.ptr(table), lib.stream(vd[0]), len(specs)
        G = lib.get()
        if entry == 'multi':
            rcs = [G.msmc_wn_prepare_multi(None, n, blk, st), G.msmc_wn_prepare_multi(tp, 0, blk, st),
                   G.msmc_wn_prepare_multi(tp, -1, blk, st), G.msmc_wn_prepare_multi(tp, n, 0, st)]
        elif entry == 'tiled':
            rcs = [G.msmc_wn_prepare_multi_tiled(None, n, blk, tblk, st), G.msmc_wn_prepare_multi_tiled(tp, 0, blk, tblk, st),
                   G.msmc_wn_prepare_multi_tiled(tp, n, 0, tblk, st), G.msmc_wn_prepare_multi_tiled(tp, n, blk, -1, st)]
        else:
            flat, o_norm, n_norm, o_tile = convnet._wn_maps(items, torch.device(dev))
            base = flat.data_ptr()
            ri, nr, ti = ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * o_norm), ctypes.c_void_p(base + 4 * o_tile)
            f = G.msmc_wn_prepare_multi_tiles
            rcs = [f(None, n, blk, tblk, 3, ri, nr, n_norm, ti, st), f(tp, 0, blk, tblk, 3, ri, nr, n_norm, ti, st),
                   f(tp, n, 0, tblk, 3, ri, nr, n_norm, ti, st), f(tp, n, blk, 0, 3, ri, nr, n_norm, ti, st),
                   f(tp, n, blk, tblk, 0, ri, nr, n_norm, ti, st), f(tp, n, blk, tblk, 17, ri, nr, n_norm, ti, st),
                   f(tp, n, blk, tblk, 3, ri, nr, -1, ti, st), f(tp, n, blk, tblk, 3, None, nr, n_norm, ti, st),
                   f(tp, n, blk, tblk, 3, ri, None, n_norm, ti, st)]
        assert rcs == [E_SHAPE] * len(rcs), (entry, rcs)
        seen.append(len(rcs))
        for b in bufs:
            for t in b:
                assert all_nan(t.cpu()), entry + ': a refused call wrote something'
        assert all_nan(slack.cpu()), entry + ': a refused call wrote something'
    assert seen == [4, 4, 9]


# ---- 2: weight-norm backward -----------------------------------------------------------------------------------------------------------
# (A, Bc, T, weight-normalised, copies, nbias | None)
BW_SMALL = ((3, 5, 3, True, 0, 3), (2, 129, 4, True, 1, 4), (5, 73, 7, True, 2, 3), (1, 40, 3, False, 8, None), (1, 33, 5, True, 9, 1),
            (4, 16, 16, False, 1, 8), (2, 1000, 4, True, 1, 2))
BW_LARGE = ((2, 1025, 7, True, 1, 2), (2, 1025, 7, True, 3, None), (2, 300, 3, True, 0, 4), (3, 255, 4, True, 2, 2),
            (2, 257, 4, True, 8, 2), (1, 7, 2, False, 9, 1), (1, 100, 1, True, 1, None), (1, 1025, 7, False, 2, 1))
BW_TABLES = {'small': (BW_SMALL, 4000), 'large': (BW_LARGE, 7175)}


def bw_inputs(specs, key):
    data = []
    for i, (A, Bc, T, normed, copies, nbias) in enumerate(specs):
        gen = gen_for(5000, key, i, A, Bc, T)
        R = max(copies, 1)
        d = dict(v=torch.randn(A, Bc, T, generator=gen), g=torch.rand(A, generator=gen) + 0.5,
                 dw=torch.randn(R, T, A, Bc, generator=gen),                               # layout 1: [T][A][Bc]
                 db=torch.randn(R, nbias, generator=gen) if nbias else None,
                 pre_gv=torch.randn(A, Bc, T, generator=gen), pre_gg=torch.randn(A, generator=gen),
                 pre_gb=torch.randn(nbias, generator=gen) if nbias else None)
        d['inv'] = (1.0 / d['v'].double().reshape(A, -1).norm(dim=1)).float()
        data.append(d)
    return data


def copies_buffer(x, stride, dev):
    """the R copies x[r] (flattened) at ``stride`` elements from each other in a NaN-filled buffer -> the buffer, consumed positions"""
    R, n = x.shape[0], x[0].numel()
    buf = _nan(((R - 1) * stride + n + GUARD,), 'cpu')
    idx = (torch.arange(R)[:, None] * stride + torch.arange(n)[None, :]).reshape(-1)
    buf[idx] = x.reshape(-1)
    return buf, idx


def bw_run(dev, specs, data, accumulate, entry, max_row=0):
    """one launch over the table -> per item gv, gg, gb, dw buffer, db buffer after the call (CPU), run twice"""
    lib = L()
    fixed = [(d['v'].to(dev), d['g'].to(dev), d['inv'].to(dev)) for d in data]

    def run():
        items = (lib.WnItem * len(specs))()
        outs, blk = [], 0
        for it, (A, Bc, T, normed, copies, nbias), d, (v, g, inv) in zip(items, specs, data, fixed):
            n_tot = A * Bc * T
            dw0, _ = copies_buffer(d['dw'], n_tot + 5, dev)
            dw = dw0.to(dev)
            gv, gg = Out((A, Bc, T), dev), Out((A,), dev)
            db = gb = None
            if nbias:
                db = copies_buffer(d['db'], nbias + 3, dev)[0].to(dev)
                gb = Out((nbias,), dev)
            if accumulate:
                gv.t.copy_(d['pre_gv'].reshape(-1).to(dev))
                gg.t.copy_(d['pre_gg'].to(dev))
                if nbias:
                    gb.t.copy_(d['pre_gb'].to(dev))
            it.v, it.g, it.inv_norm = v.data_ptr(), (g.data_ptr() if normed else None), inv.data_ptr()
            it.dw, it.gv, it.gg = dw.data_ptr(), gv.t.data_ptr(), gg.t.data_ptr()
            it.db, it.gb = (db.data_ptr() if nbias else None), (gb.t.data_ptr() if nbias else None)
            it.A, it.Bc, it.T, it.dtype, it.block0, it.nbias = A, Bc, T, 0, blk, (nbias or 0)
            it.s1[0], it.s1[1], it.s1[2] = A * Bc, Bc, 1
            it.copies, it.dw_copy_stride, it.db_copy_stride = copies, n_tot + 5, (nbias or 0) + 3
            blk += A
            outs.append((gv, gg, gb, dw, db))
        table = dev_table(items, dev)
        tp, st, n = lib.ptr(table), lib.stream(fixed[0][0]), len(specs)
        if entry == 'rows':
            lib.call('msmc_wn_backward_multi_rows', tp, n, blk, accumulate, max_row, st)
        elif entry == 'acc':
            lib.call('msmc_wn_backward_multi_acc', tp, n, blk, accumulate, st)
        else:
            lib.call('msmc_wn_backward_multi', tp, n, blk, st)
        res = []
        for gv, gg, gb, dw, db in outs:
            res += [gv.get(written=False), gg.get(written=False), gb.get(written=False) if gb else torch.zeros(0), dw.cpu(),
                    db.cpu() if db is not None else torch.zeros(0)]
        return tuple(res)

    return twice(run)


def bw_floor(S, v, g, inv, e_S, nt, extra_inv=0.0):
    """the rounding-count bounds of gv, gg (module docstring); S, v [A][Bc][T] float64, e_S the bound on S itself, ``extra_inv`` the
    relative error of inv beyond its own rounding"""
    A = v.shape[0]
    n = v[0].numel()
    D = d_sum(n, nt)
    row = lambda t: t.reshape(A, -1).sum(1)
    dot = row(S * v)
    e_d = D * U * row((S * v).abs()) + row(e_S * v.abs())
    ei = U + extra_inv
    f_gg = e_d * inv + (2 * U + ei) * (dot * inv).abs()
    k1, k2 = (g * inv).abs(), (dot * inv * inv).abs()
    e_k = e_d * inv * inv + (2 * U + 2 * ei) * k2
    k1_, k2_, ek_ = k1[:, None, None], k2[:, None, None], e_k[:, None, None]
    mag = S.abs() + v.abs() * k2_
    f_gv = k1_ * (e_S + v.abs() * ek_ + U * v.abs() * k2_ + U * mag) + (2 * U + ei) * k1_ * mag
    return f_gv * ONE, f_gg * ONE


def bw_reference(d, spec, accumulate):
    """float64 autograd of sum(dW * g v / ||v||) and the fp32 chain -> dict of (ref, t32) per quantity, the fold S and its bound"""
    A, Bc, T, normed, copies, nbias = spec
    R = max(copies, 1)
    S64 = d['dw'].double().sum(0).permute(1, 2, 0).contiguous()                       # [A][Bc][T]
    fold = d['dw'][0]
    for r in range(1, R):
        fold = fold + d['dw'][r]
    fold = fold.permute(1, 2, 0).contiguous()
    e_S = (R - 1) * U * d['dw'].double().abs().sum(0).permute(1, 2, 0)
    out = dict(S64=S64, fold=fold, e_S=e_S)
    if normed:
        v_ = d['v'].double().requires_grad_(True)
        g_ = d['g'].double().requires_grad_(True)
        W = g_[:, None, None] * v_ / v_.reshape(A, -1).norm(dim=1)[:, None, None]
        (S64 * W).sum().backward()
        inv, v, g = d['inv'], d['v'], d['g']
        dot = (fold * v).reshape(A, -1).sum(1)
        k1, k2 = g * inv, dot * inv * inv
        out['gv'] = (v_.grad, k1[:, None, None] * (fold - v * k2[:, None, None]))
        out['gg'] = (g_.grad, dot * inv)
    if nbias:
        f = d['db'][0]
        for r in range(1, R):
            f = f + d['db'][r]
        out['gb'] = (d['db'].double().sum(0), f)
    if accumulate:
        for nm in ('gv', 'gg', 'gb'):
            if nm in out:
                pre = d['pre_' + nm]
                out[nm] = (out[nm][0] + pre.double(), pre + out[nm][1])
    return out


def bw_compare(tag, spec, d, got, accumulate, nt):
    A, Bc, T, normed, copies, nbias = spec
    R = max(copies, 1)
    gv, gg, gb, dw, db = got
    ref = bw_reference(d, spec, accumulate)
    n_tot = A * Bc * T
    if normed:
        f_gv, f_gg = bw_floor(ref['S64'], d['v'].double(), d['g'].double(), d['inv'].double(), ref['e_S'], nt)
        if accumulate:
            f_gv = f_gv + U * (d['pre_gv'].double().abs() + ref['gv'][0].abs()) * ONE
            f_gg = f_gg + U * (d['pre_gg'].double().abs() + ref['gg'][0].abs()) * ONE
        yard('backward gv', tag, gv, ref['gv'][1], ref['gv'][0], f_gv)
        yard('backward gg', tag, gg, ref['gg'][1], ref['gg'][0], f_gg)
    else:
        assert same_bits(gv, d['pre_gv'] + ref['fold'] if accumulate else ref['fold']), tag + ': gv of a plain item is not the fold'
        assert same_bits(gg, d['pre_gg']) if accumulate else all_nan(gg), tag + ': gg of a plain item was written'
    if nbias:
        pre = d['pre_gb'].double().abs() if accumulate else 0.0
        yard('backward gb', tag, gb, ref['gb'][1], ref['gb'][0], (R + 1) * U * (d['db'].double().abs().sum(0) + pre) * ONE)
    # every consumed accumulator element is +0, nothing else moved
    want, idx = copies_buffer(d['dw'], n_tot + 5, 'cpu')
    want[idx] = 0.0
    assert same_bits(dw, want), tag + ': dw is not +0 where consumed and untouched elsewhere'
    if nbias:
        want, idx = copies_buffer(d['db'], nbias + 3, 'cpu')
        want[idx] = 0.0
        assert same_bits(db, want), tag + ': db is not +0 where consumed and untouched elsewhere'


def check_backward(dev, table, accumulate, max_row):
    """msmc_wn_backward_multi_rows over one mixed table; at max_row = 0 also _acc (and _multi without accumulate), bit-equal"""
    specs, longest = BW_TABLES[table]
    assert longest == max(s[1] * s[2] for s in specs) and max_row in (0, longest)
    nt = 128 if 0 < max_row <= 4096 else 256
    data = bw_inputs(specs, 0 if table == 'small' else 1)
    got = bw_run(dev, specs, data, accumulate, 'rows', max_row)
    for i, (spec, d) in enumerate(zip(specs, data)):
        tag = '%s%d %dx%dx%d R%d nb%s acc%d mr%d' % (table[0].upper() if table == 'small' else 'G', i, spec[0], spec[1], spec[2], spec[4],
                                                      spec[5], accumulate, max_row)
        bw_compare(tag, spec, d, got[5 * i:5 * i + 5], accumulate, nt)
    if max_row == 0:
        for entry in ('acc',) + (() if accumulate else ('multi',)):
            other = bw_run(dev, specs, data, accumulate, entry)
            assert len(other) == len(got)
            for a, b in zip(got, other):
                assert same_bits(a, b), 'msmc_wn_backward_multi%s differs from _rows with the arguments it forwards' % (
                    '_acc' if entry == 'acc' else '')


def check_backward_refusals(dev):
    lib = L()
    z = torch.zeros(64, dtype=torch.uint8).to(dev)
    G, st = lib.get(), lib.stream(z)
    assert G.msmc_wn_backward_multi_rows(None, 1, 1, 0, 0, st) == E_SHAPE
    assert G.msmc_wn_backward_multi_rows(lib.ptr(z), 0, 1, 0, 0, st) == E_SHAPE
    assert G.msmc_wn_backward_multi_rows(lib.ptr(z), 1, 0, 0, 0, st) == E_SHAPE
    assert G.msmc_wn_backward_multi_acc(None, 1, 1, 0, st) == E_SHAPE
    assert G.msmc_wn_backward_multi(None, 1, 1, st) == E_SHAPE


# ---- 3: column sums ------------------------------------------------------------------------------------------------------------------
COLSUM_C = (1, 2, 3, 4, 8, 24, 64, 80, 256, 257, 513, 1024, 2048)
COLSUM_CAP_ROWS = 256 * 128 + 129
COLSUM_BIG = ((4, 0), (3, 1), (2, 0))        # (C, dtype) of the two row counts past the block cap


def colsum_rows(C):
    return (1, 127, 128, 129, 257) if C <= 257 else (1, 129) if C <= 513 else (1, 33)


def colsum_vector(C, which):
    """whether an aligned [rows][C] input takes the 16-byte branch: whole vectors per row, whole rows per 256 vectors"""
    ve = 4 if which == 0 else 8
    return C % ve == 0 and (256 * ve) % C == 0


def colsum_fewer():
    """the smallest row count for which fewer blocks own rows than are launched (the launcher's arithmetic: at most 256 blocks of
    at least 128 rows, the rows spread evenly over them), or None below 40 000"""
    for rows in range(1, 40000):
        nb = min(256, (rows + 127) // 128)
        rpb = (rows + nb - 1) // nb
        if (rows + rpb - 1) // rpb < nb:
            return rows
    return None


def colsum_call(dev, g, C, which, accumulate, pre, off=0, ws_short=0, atomic=False):
    """-> out (CPU) of msmc_colsum_ws (or the atomic msmc_colsum) over g [rows][C]; the workspace is NaN-filled with guards"""
    lib = L()
    code, dtype, _ = DTYPES[which]
    rows = g.shape[0]
    gd = at(g, dev, off)
    need = int(lib.get().msmc_colsum_workspace(rows, C))

    def run():
        out, ws = Out((C,), dev), Out((need // 4,), dev)
        if accumulate:
            out.t.copy_(pre.to(dev))
        if atomic:
            lib.call('msmc_colsum', lib.ptr(gd), lib.ptr(out.t), rows, C, code, lib.stream(gd))
        else:
            lib.call('msmc_colsum_ws', lib.ptr(gd), lib.ptr(out.t), rows, C, code, accumulate, lib.ptr(ws.t), need, lib.stream(gd))
        ws.get(written=False)
        return (out.get(),)

    return run()[0] if atomic else twice(run)[0]


def colsum_compare(what, tag, out, g, accumulate, pre):
    rows = g.shape[0]
    g64 = g.double()
    if accumulate:
        held(what, tag, out, g64.sum(0) + pre.double(), rows * U * (g64.abs().sum(0) + pre.double().abs()) * ONE)
    else:
        held(what, tag, out, g64.sum(0), (rows - 1) * U * g64.abs().sum(0) * ONE)


def check_colsum(dev, C, which, rows_list=None):
    code, dtype, name = DTYPES[which]
    for rows in rows_list or colsum_rows(C):
        gen = gen_for(6000, C, rows, which)
        g = torch.randn(rows, C, generator=gen).to(dtype)
        pre = torch.randn(C, generator=gen)
        for accumulate in (0, 1):
            tag = '%dx%d %s acc%d' % (rows, C, name, accumulate)
            out = colsum_call(dev, g, C, which, accumulate, pre)
            colsum_compare('colsum_ws', tag, out, g, accumulate, pre)
            if colsum_vector(C, which):
                off = colsum_call(dev, g, C, which, accumulate, pre, off=1)
                colsum_compare('colsum_ws view + 1', tag, off, g, accumulate, pre)
                if rows == 1:
                    assert same_bits(off, out), tag + ': one row, and the view differs from the aligned call'


def check_colsum_atomic(dev, C, which):
    code, dtype, name = DTYPES[which]
    for rows in (1, 257, 600):
        gen = gen_for(6100, C, rows, which)
        g = torch.randn(rows, C, generator=gen).to(dtype)
        out = colsum_call(dev, g, C, which, 0, None, atomic=True)
        colsum_compare('colsum atomic', '%dx%d %s' % (rows, C, name), out, g, 0, None)


def check_colsum_refusals(dev):
    lib = L()
    G = lib.get()
    rows, C = 300, 8
    g = torch.randn(rows, C, generator=gen_for(6200)).to(dev)
    need = int(G.msmc_colsum_workspace(rows, C))
    assert need == 3 * C * 4 and G.msmc_colsum_workspace(0, C) == 0 and G.msmc_colsum_workspace(rows, 0) == 0
    out, ws = Out((C,), dev), Out((need // 4,), dev)
    st = lib.stream(g)
    f = G.msmc_colsum_ws
    assert f(lib.ptr(g), lib.ptr(out.t), rows, C, 0, 0, lib.ptr(ws.t), need - 1, st) == E_WORKSPACE
    assert f(lib.ptr(g), lib.ptr(out.t), rows, C, 0, 0, None, need, st) == E_WORKSPACE
    for r_, c_ in ((0, C), (-1, C), (rows, 0), (rows, -1)):
        assert f(lib.ptr(g), lib.ptr(out.t), r_, c_, 0, 0, lib.ptr(ws.t), need, st) == E_SHAPE, (r_, c_)
        assert G.msmc_colsum(lib.ptr(g), lib.ptr(out.t), r_, c_, 0, st) == E_SHAPE, (r_, c_)
    assert f(None, lib.ptr(out.t), rows, C, 0, 0, lib.ptr(ws.t), need, st) == E_SHAPE
    assert f(lib.ptr(g), None, rows, C, 0, 0, lib.ptr(ws.t), need, st) == E_SHAPE
    assert all_nan(out.get(written=False)) and all_nan(ws.get(written=False)), 'a refused call wrote something'


# ---- 4: reflect fold --------------------------------------------------------------------------------------------------------------------
# the padding each channel count of the per-C groups runs with: every p in 0 .. 3
FOLD_P = {1: 0, 2: 1, 4: 2, 6: 3, 8: 1, 12: 2, 32: 3}
# multi form: more than 16 * CUs * 256 items of one channel (MI355X: 256 CUs); single form: more than 4096 * 256 elements
FOLD_CAP_GPU = ((2, 725, 725, 1), (2, 130, 127, 32))


def fold_cap_emu():
    """the same past the interpreter's own 16 * MSMC_NUM_CU workgroups (3 compute units unless MSMC_EMU_CUS says otherwise); the
    single form's 4096 workgroups do not depend on the machine"""
    cap = 16 * int(os.environ.get('MSMC_EMU_CUS', '3')) * 256
    side = int(math.isqrt(cap // 2)) + 2
    return (2, side, side, 1), FOLD_CAP_GPU[1]


def fold_members(C, p):
    """(B, H, W, C, mask, res, offset): the smallest legal extent on either axis, H != W, B > 1; members without a mask or a third
    input next to members that have them"""
    return ((2, p + 1, p + 3, C, True, True, 0), (1, p + 2, p + 1, C, True, False, 0), (3, 5, 4, C, False, False, 0))


def fold_inputs(members, p, which, key):
    code, dtype, _ = DTYPES[which]
    data = []
    for i, (B, H, W, C, has_mask, has_res, off) in enumerate(members):
        gen = gen_for(7000, seed_of(key), i, B, H, W, C, p)
        gp = torch.randn(B, H + 2 * p, W + 2 * p, C, generator=gen).to(dtype)
        mask = torch.randn(B, H, W, C, generator=gen)
        flat = mask.view(-1)
        flat[0::5] = 0.0                                                  # +0 and -0: both take the slope
        flat[3::5] = -0.0
        res = torch.randn(B, H, W, C, generator=gen).to(dtype)
        data.append((gp, mask.to(dtype) if has_mask else None, res if has_res else None))
    return data


def fold_reference(gp, mask, res, H, W, p, mode):
    """float64 autograd of F.pad(mode='reflect') on the NCHW permutation -> reference, sum |addends| + |res|"""
    B, C = gp.shape[0], gp.shape[3]

    def adjoint(t):
        if p == 0:
            return t.clone()
        x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        F_.pad(x, (p, p, p, p), mode='reflect').backward(t.permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous()

    s, mag = adjoint(gp.double()), adjoint(gp.double().abs())
    m = torch.where(mask.double() > 0, 1.0, SLOPE_F64) if mask is not None else torch.ones_like(s)
    r = res.double() if (res is not None and mode != 'multi') else torch.zeros_like(s)
    ref = (s + r) * m if mode == 'tap' else s * m + r
    return ref, mag + r.abs()


SLOPE_F32 = torch.tensor(SLOPE, dtype=torch.float32)
SLOPE_F64 = float(SLOPE_F32.double())


def fold_group_call(dev, members, data, p, which, mode, expect=0, n=None):
    """one launch of msmc_reflect_fold_multi (mode 'multi'), _res or _tap -> the folded gradients on the CPU (run twice)"""
    lib = L()
    code, dtype, _ = DTYPES[which]
    n = len(members) if n is None else n
    gpd = [at(gp, dev, m[6]) for (gp, _, _), m in zip(data, members)]
    md = [at(mk, dev, m[6]) for (_, mk, _), m in zip(data, members)]
    rd = [at(rs, dev, m[6]) for (_, _, rs), m in zip(data, members)]
    vp, ip = ctypes.c_void_p * len(members), ctypes.c_int * len(members)
    pt = lambda ts: vp(*[t.data_ptr() if t is not None else None for t in ts])

    def run():
        outs = [Out((B, H, W, C), dev, dtype, off) for B, H, W, C, _, _, off in members]
        dims = [ip(*[m[k] for m in members]) for k in range(4)]
        gx = vp(*[o.t.data_ptr() for o in outs])
        st = lib.stream(gpd[0])
        if mode == 'multi':
            rc = lib.get().msmc_reflect_fold_multi(pt(gpd), pt(md), gx, dims[0], dims[1], dims[2], dims[3], n, p, SLOPE, code, st)
        else:
            f = lib.get().msmc_reflect_fold_multi_tap if mode == 'tap' else lib.get().msmc_reflect_fold_multi_res
            rc = f(pt(gpd), pt(md), pt(rd), gx, dims[0], dims[1], dims[2], dims[3], n, p, SLOPE, code, st)
        assert rc == expect, (rc, expect)
        got = tuple(o.get(written=(expect == 0)) for o in outs)
        if expect != 0:
            assert all(all_nan(g) for g in got), 'a refused call wrote something'
        return got

    return twice(run)


def fold_single_call(dev, member, d, p, which, with_mask=True):
    lib = L()
    code, dtype, _ = DTYPES[which]
    B, H, W, C = member[:4]
    gpd, md = d[0].to(dev), (d[1].to(dev) if (d[1] is not None and with_mask) else None)

    def run():
        o = Out((B, H, W, C), dev, dtype)
        lib.call('msmc_reflect_fold', lib.ptr(gpd), lib.ptr(md), lib.ptr(o.t), B, H, W, C, p, SLOPE, code, lib.stream(gpd))
        return (o.get(),)

    return twice(run)[0]


def fold_compare(what, tag, got, d, member, p, mode, which):
    B, H, W, C = member[:4]
    ref, mag = fold_reference(d[0], d[1], d[2], H, W, p, mode)
    held(what, tag, got, ref, 10 * U * mag + half_ulp(ref, DTYPES[which][1]))


def check_fold_group(dev, members, p, which, key, modes=('multi', 'res', 'tap'), single=True):
    """the group in every mode against float64; the single entry on the first member, bit-equal to a one-member group"""
    name = DTYPES[which][2]
    data = fold_inputs(members, p, which, key)
    for mode in modes:
        got = fold_group_call(dev, members, data, p, which, mode)
        for i, (m, d, g) in enumerate(zip(members, data, got)):
            tag = '%s m%d %dx%dx%dx%d p%d %s%s' % (key, i, m[0], m[1], m[2], m[3], p, name, ' +%d' % m[6] if m[6] else '')
            fold_compare('fold %s' % mode, tag, g, d, m, p, mode, which)
    if single:
        m, d = members[0], data[0]
        one = fold_single_call(dev, m, d, p, which)
        fold_compare('fold single', '%s %dx%dx%dx%d p%d %s' % (key, m[0], m[1], m[2], m[3], p, name), one, d, m, p, 'multi', which)
        grp = fold_group_call(dev, members[:1], data[:1], p, which, 'multi')[0]
        assert same_bits(one, grp), 'the single entry and a one-member group differ'


def check_fold_channels(dev, C, which):
    check_fold_group(dev, fold_members(C, FOLD_P[C]), FOLD_P[C], which, 'C%d' % C)


FOLD_SPECIAL = {
    'V forced to 2': ((1, 3, 4, 8, True, True, 0), (2, 2, 3, 12, True, False, 0), (1, 4, 2, 6, False, True, 0)),
    'V forced to 1': ((1, 3, 4, 8, True, True, 0), (2, 2, 3, 4, True, False, 0), (1, 4, 2, 1, False, True, 0)),
    'one member + 1': ((1, 3, 4, 8, True, True, 0), (2, 2, 3, 8, True, True, 1), (1, 4, 2, 16, False, False, 0)),
    'one member + 2': ((1, 3, 4, 8, True, True, 0), (2, 2, 3, 8, True, True, 2), (1, 4, 2, 16, False, False, 0)),
    'six members': tuple((1 + i % 2, 2 + i, 3 + (i * 2) % 3, 8, i % 2 == 0, i % 3 != 0, 0) for i in range(6)),
}


def check_fold_special(dev, key, which):
    check_fold_group(dev, FOLD_SPECIAL[key], 1, which, key, single=False)


def check_fold_refusals(dev):
    """seven members, H <= p, W <= p and NULL operands -> MSMC_E_SHAPE in every entry, nothing written (fold_group_call itself
    holds every output of a refused group call to its NaN bits)"""
    lib = L()
    seven = tuple((1, 2, 3, 4, True, True, 0) for _ in range(7))
    for mode in ('multi', 'res', 'tap'):
        fold_group_call(dev, seven, fold_inputs(seven, 1, 0, 'seven'), 1, 0, mode, expect=E_SHAPE)
        fold_group_call(dev, seven[:2], fold_inputs(seven[:2], 1, 0, 'zero'), 1, 0, mode, expect=E_SHAPE, n=0)
        for bad in ((1, 2, 3, 4, True, True, 0), (1, 3, 2, 4, True, True, 0)):                # H <= p, W <= p at p = 2
            ms = (seven[0], bad)
            data = [(torch.zeros(m[0], m[1] + 4, m[2] + 4, 4), torch.ones(m[:4]), torch.ones(m[:4])) for m in ms]
            fold_group_call(dev, ms, data, 2, 0, mode, expect=E_SHAPE)
    G = lib.get()
    B, H, W, C, p = 1, 3, 3, 4, 1
    gp = torch.zeros(B, H + 2, W + 2, C).to(dev)
    o = Out((B, H, W, C), dev)
    st = lib.stream(gp)
    vp, ip = ctypes.c_void_p * 1, ctypes.c_int * 1
    gpa, gxa, one = vp(gp.data_ptr()), vp(o.t.data_ptr()), ip(1)
    hs, ws, cs = ip(H), ip(W), ip(C)
    f = G.msmc_reflect_fold_multi_res
    assert f(gpa, None, None, gxa, one, hs, ws, cs, 1, p, SLOPE, 0, st) == 0
    o.get()
    o = Out((B, H, W, C), dev)
    gxa = vp(o.t.data_ptr())
    assert f(None, None, None, gxa, one, hs, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, None, one, hs, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(vp(None), None, None, gxa, one, hs, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, vp(None), one, hs, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, None, hs, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, one, None, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, one, hs, None, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, one, hs, ws, None, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, one, hs, ws, cs, 1, -1, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, one, hs, ws, cs, 1, p, SLOPE, 2, st) == E_SHAPE
    assert f(gpa, None, None, gxa, ip(0), hs, ws, cs, 1, p, SLOPE, 0, st) == E_SHAPE
    assert f(gpa, None, None, gxa, one, hs, ws, ip(0), 1, p, SLOPE, 0, st) == E_SHAPE
    s = G.msmc_reflect_fold
    assert s(None, None, lib.ptr(o.t), B, H, W, C, p, SLOPE, 0, st) == E_SHAPE
    assert s(lib.ptr(gp), None, None, B, H, W, C, p, SLOPE, 0, st) == E_SHAPE
    for b_, h_, w_, c_, p_ in ((0, H, W, C, p), (B, 1, W, C, 1), (B, H, 1, C, 1), (B, H, W, 0, p), (B, H, W, C, -1)):
        assert s(lib.ptr(gp), None, lib.ptr(o.t), b_, h_, w_, c_, p_, SLOPE, 0, st) == E_SHAPE, (b_, h_, w_, c_, p_)
    assert all_nan(o.get(written=False)), 'a refused call wrote something'


def check_fold_past_cap(dev, sizes):
    """one case per entry whose item count exceeds the grid cap, so that work-items take their stride a second time (bf16)"""
    multi, single = sizes
    m = multi + (True, True, 0)
    check_fold_group(dev, (m,), 1, 1, 'cap', modes=('tap',), single=False)
    m = single + (True, False, 0)
    assert m[0] * m[1] * m[2] * m[3] > 4096 * 256
    d = fold_inputs((m,), 1, 1, 'cap1')[0]
    one = fold_single_call(dev, m, d, 1, 1)
    fold_compare('fold single', 'cap %dx%dx%dx%d p1 bf16' % m[:4], one, d, m, 1, 'multi', 1)


# ---- 5: leaky-ReLU backward ---------------------------------------------------------------------------------------------------------------
LRELU_SIZES = (1, 3, 4, 7, 8, 1023, 1025, 5000)


def lrelu_inputs(n, which, key):
    dtype = DTYPES[which][1]
    gen = gen_for(8000, key, n, which)
    g = torch.randn(n, generator=gen).to(dtype)
    y = torch.randn(n, generator=gen)
    y[0::5] = 0.0
    y[3::5] = -0.0
    return g, y.to(dtype)


def lrelu_want(g, y):
    return torch.where(y.float() > 0, g.float(), g.float() * SLOPE_F32).to(g.dtype)


def lrelu_group_call(dev, pairs, which, offs=None, expect=0):
    lib = L()
    code, dtype, _ = DTYPES[which]
    n = len(pairs)
    offs = offs or [(0, 0, 0)] * n
    gd = [at(g, dev, o[0]) for (g, _), o in zip(pairs, offs)]
    yd = [at(y, dev, o[1]) for (_, y), o in zip(pairs, offs)]
    vp = ctypes.c_void_p * n

    def run():
        outs = [Out((g.numel(),), dev, dtype, o[2]) for (g, _), o in zip(pairs, offs)]
        rc = lib.get().msmc_lrelu_bwd_multi(vp(*[t.data_ptr() for t in gd]), vp(*[t.data_ptr() for t in yd]),
                                            vp(*[o.t.data_ptr() for o in outs]), (ctypes.c_long * n)(*[g.numel() for g, _ in pairs]), n,
                                            SLOPE, code, lib.stream(gd[0]))
        assert rc == expect, (rc, expect)
        got = tuple(o.get(written=(expect == 0)) for o in outs)
        if expect != 0:
            assert all(all_nan(g) for g in got), 'a refused call wrote something'
        return got

    return twice(run)


def check_lrelu(dev, n, which):
    """msmc_lrelu_bwd and a one-member msmc_lrelu_bwd_multi: bit-equal to where(y > 0, g, g * slope) rounded once"""
    lib = L()
    code, dtype, name = DTYPES[which]
    g, y = lrelu_inputs(n, which, 0)
    want = lrelu_want(g, y)
    gd, yd = g.to(dev), y.to(dev)

    def run():
        o = Out((n,), dev, dtype)
        lib.call('msmc_lrelu_bwd', lib.ptr(gd), lib.ptr(yd), lib.ptr(o.t), n, SLOPE, code, lib.stream(gd))
        return (o.get(),)

    assert same_bits(twice(run)[0], want), 'msmc_lrelu_bwd n %d %s' % (n, name)
    assert same_bits(lrelu_group_call(dev, [(g, y)], which)[0], want), 'msmc_lrelu_bwd_multi n %d %s' % (n, name)
    MEASURED.append(('lrelu', 'n %d %s' % (n, name), 0.0, 'bit-equal'))


def check_lrelu_groups(dev, which):
    """whole-vector members (the 16-byte kernel); one member with n % VEC != 0 (the element kernel for all); six members; seven refused"""
    vec = 4 if which == 0 else 8
    for sizes in ((vec, 128 * vec, 2 * vec), (vec, 128 * vec - 1, 2 * vec), (vec, 3 * vec, 5, 1, 40 * vec, 7 * vec)):
        pairs = [lrelu_inputs(n, which, 1 + i) for i, n in enumerate(sizes)]
        for got, (g, y) in zip(lrelu_group_call(dev, pairs, which), pairs):
            assert same_bits(got, lrelu_want(g, y)), sizes
    pairs = [lrelu_inputs(vec, which, 20 + i) for i in range(7)]
    for got in lrelu_group_call(dev, pairs, which, expect=E_SHAPE):
        assert all_nan(got), 'a refused call wrote something'
    MEASURED.append(('lrelu groups', DTYPES[which][2], 0.0, 'bit-equal'))


def check_lrelu_misaligned(dev, which):
    """g, y, gx in turn (and all three) one element into their buffers with n % VEC == 0: the launcher must leave the 16-byte
    kernel; bit-equal to the aligned result"""
    vec = 4 if which == 0 else 8
    pairs = [lrelu_inputs(n, which, 30 + i) for i, n in enumerate((4 * vec, 64 * vec))]
    base = lrelu_group_call(dev, pairs, which)
    for (g, y), b in zip(pairs, base):
        assert same_bits(b, lrelu_want(g, y))
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        for member in (0, 1):
            offs = [off if k == member else (0, 0, 0) for k in range(2)]
            for got, b in zip(lrelu_group_call(dev, pairs, which, offs=offs), base):
                assert same_bits(got, b), (off, member)
    MEASURED.append(('lrelu misaligned', DTYPES[which][2], 0.0, 'bit-equal'))


def check_lrelu_refusals(dev):
    lib = L()
    G = lib.get()
    g = torch.ones(8).to(dev)
    o = Out((8,), dev)
    st = lib.stream(g)
    s = G.msmc_lrelu_bwd
    assert s(None, lib.ptr(g), lib.ptr(o.t), 8, SLOPE, 0, st) == E_SHAPE and s(lib.ptr(g), None, lib.ptr(o.t), 8, SLOPE, 0, st) == E_SHAPE
    assert s(lib.ptr(g), lib.ptr(g), None, 8, SLOPE, 0, st) == E_SHAPE and s(lib.ptr(g), lib.ptr(g), lib.ptr(o.t), 0, SLOPE, 0, st) == E_SHAPE
    vp, lp = ctypes.c_void_p * 1, ctypes.c_long * 1
    ga, oa, na = vp(g.data_ptr()), vp(o.t.data_ptr()), lp(8)
    f = G.msmc_lrelu_bwd_multi
    for args in ((None, ga, oa, na, 1, 0), (ga, None, oa, na, 1, 0), (ga, ga, None, na, 1, 0), (ga, ga, oa, None, 1, 0), (ga, ga, oa, na, 0, 0),
                 (ga, ga, oa, na, 1, 2), (vp(None), ga, oa, na, 1, 0), (ga, vp(None), oa, na, 1, 0), (ga, ga, vp(None), na, 1, 0),
                 (ga, ga, oa, lp(0), 1, 0)):
        assert f(args[0], args[1], args[2], args[3], args[4], SLOPE, args[5], st) == E_SHAPE, args[4:]
    assert all_nan(o.get(written=False)), 'a refused call wrote something'


# ---- 6: the host layer, once ---------------------------------------------------------------------------------------------------------------
def check_host_colsum_and_folds(dev):
    """conv.colsum with and without ``out``, conv.reflect_fold, reflect_fold_group (res and tap_first) and lrelu_bwd_group with seven
    items each (two launches)"""
    from msmctts_amd.hip import conv
    gen = gen_for(9000)
    for which, (_, dtype, name) in enumerate(DTYPES):
        g = torch.randn(300, 24, generator=gen).to(dtype)
        pre = torch.randn(24, generator=gen)
        out = conv.colsum(g.to(dev))
        assert out.dtype == torch.float32
        colsum_compare('host colsum', '300x24 %s' % name, out.cpu(), g, 0, None)
        acc = pre.clone().to(dev)
        assert conv.colsum(g.to(dev), out=acc) is acc
        colsum_compare('host colsum out', '300x24 %s' % name, acc.cpu(), g, 1, pre)
        members = tuple((1 + i % 2, 2 + i % 3, 4 - i % 2, 4 if i < 6 else 6, i % 2 == 0, i % 3 != 1, 0) for i in range(7))
        data = fold_inputs(members, 1, which, 'host')
        m, d = members[0], data[0]
        one = conv.reflect_fold(d[0].to(dev), m[1], m[2], 1, d[1].to(dev), SLOPE)
        fold_compare('host fold', '%dx%dx%dx%d %s' % (m[:4] + (name,)), one.cpu(), d, m, 1, 'multi', which)
        for tap_first in (False, True):
            items = [(gp.to(dev), mm[1], mm[2], mk.to(dev) if mk is not None else None, rs.to(dev) if rs is not None else None)
                     for mm, (gp, mk, rs) in zip(members, data)]
            outs = conv.reflect_fold_group(items, p=1, slope=SLOPE, tap_first=tap_first)
            assert len(outs) == 7
            for i, (mm, dd, o) in enumerate(zip(members, data, outs)):
                fold_compare('host fold group', 'm%d %s tap_first %d' % (i, name, tap_first), o.cpu(), dd, mm, 1,
                             'tap' if tap_first else 'res', which)
        pairs = [lrelu_inputs(n, which, 40 + i) for i, n in enumerate((8, 16, 5, 64, 1, 24, 1000))]
        outs = conv.lrelu_bwd_group([(a.to(dev), b.to(dev)) for a, b in pairs], SLOPE)
        assert len(outs) == 7
        for (a, b), o in zip(pairs, outs):
            assert same_bits(o.cpu(), lrelu_want(a, b))
        # a contiguous view one element into a buffer: the host layer refuses it (the C entry itself takes it on the element
        # kernel: check_lrelu_misaligned)
        vec = 4 if which == 0 else 8
        a, b = lrelu_inputs(16 * vec + 1, which, 50)
        ad, bd = a.to(dev)[1:], b.to(dev)[1:]
        assert ad.is_contiguous() and ad.data_ptr() % 16 != 0
        try:
            conv.lrelu_bwd_group([(ad, bd)], SLOPE)
        except ValueError:
            pass
        else:
            raise AssertionError('lrelu_bwd_group took an offset view')


def check_host_weight_norm_layer(dev):
    """one weight-normalised Conv1d through ConvBank.prepare, hip_conv and the bank's backward against float64 autograd of
    torch.nn.utils.weight_norm; a second pass accumulates into the live gradients"""
    import torch.nn as nn
    from msmctts_amd.hip import convnet
    from msmctts_amd.networks.layers import WNConv1d
    Cin, Cout, k, B, Ln = 12, 20, 3, 2, 37
    gen = gen_for(9100)
    conv = WNConv1d(Cin, Cout, k, padding=1)
    with torch.no_grad():
        conv.weight_v.copy_(torch.randn(Cout, Cin, k, generator=gen))
        conv.weight_g.copy_((torch.rand(Cout, generator=gen) + 0.5).view_as(conv.weight_g))
        conv.bias.copy_(torch.randn(Cout, generator=gen))
    x = torch.randn(B, Ln, Cin, generator=gen)
    go = torch.randn(B, Ln, Cout, generator=gen)
    ref = torch.nn.utils.weight_norm(nn.Conv1d(Cin, Cout, k, padding=1)).double()
    with torch.no_grad():
        ref.weight_v.copy_(conv.weight_v.double())
        ref.weight_g.copy_(conv.weight_g.double().view_as(ref.weight_g))
        ref.bias.copy_(conv.bias.double())
    x64 = x.double().transpose(1, 2).contiguous()
    y64 = ref(x64)
    y64.backward(go.double().transpose(1, 2))
    # bounds: e_S of the bank's own dW (module docstring) from the same convolution on absolute values
    wabs = torch.ones(Cout, Cin, k, dtype=torch.float64, requires_grad=True)
    F_.conv1d(x64.abs(), wabs, None, 1, 1).backward(go.double().abs().transpose(1, 2))
    K = B * Ln
    e_S = (K + 2) * U * wabs.grad
    v64, g64 = conv.weight_v.detach().double(), conv.weight_g.detach().double().reshape(-1)
    inv = 1.0 / v64.reshape(Cout, -1).norm(dim=1)
    w_ = ((g64 * inv)[:, None, None] * v64).requires_grad_(True)
    F_.conv1d(x64, w_, None, 1, 1).backward(go.double().transpose(1, 2))
    S = w_.grad                                                                       # dW in the parameter's order [Cout][Cin][k]
    f_gv, f_gg = bw_floor(S, v64, g64, inv, e_S, 128, extra_inv=(d_sum(Cin * k) / 2.0 + 2) * U)
    f_gb = K * U * go.double().abs().sum((0, 1)) * ONE
    conv = conv.to(dev)
    layer = conv.hip_layer()
    bank = convnet.ConvBank([layer])
    xd = x.view(B, 1, Ln, Cin).to(dev)
    for rnd in (1, 2):
        bank.prepare(torch.float32)
        y = convnet.hip_conv(bank, layer, xd)
        y.backward(go.view(B, 1, Ln, Cout).to(dev))
        tag = '%dx%dx%d pass %d' % (Cout, Cin, k, rnd)
        pre = (rnd - 1)
        acc = lambda f, r: rnd * f + pre * U * 2 * r.abs() * ONE                      # (the second pass adds to the live gradient)
        held('host wn gv', tag, conv.weight_v.grad.cpu(), rnd * ref.weight_v.grad, acc(f_gv, ref.weight_v.grad))
        held('host wn gg', tag, conv.weight_g.grad.cpu().reshape(-1), rnd * ref.weight_g.grad.reshape(-1),
             acc(f_gg, ref.weight_g.grad.reshape(-1)))
        held('host wn gb', tag, conv.bias.grad.cpu(), rnd * ref.bias.grad, acc(f_gb, ref.bias.grad))
    # the weight image the bank prepared: both layouts against g v / ||v||
    w64 = (g64 * inv)[:, None, None] * v64
    f_w = (d_sum(Cin * k) / 2.0 + 4) * U * w64.abs() * ONE
    held('host wn w layout 1', tag, layer.wf.cpu().permute(1, 2, 0), w64, f_w)
    held('host wn w layout 2', tag, layer.wb.cpu().permute(2, 1, 0), w64, f_w)
