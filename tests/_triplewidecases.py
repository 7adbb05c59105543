"""Shared cases of the wide triple loss (csrc/triple_wide.inc, msmc_triple_loss_wide, and hip/losses.py triple_loss / Quantize
.compute_triple_loss at the widths no other kernel takes): tests/test_triple_wide_emu.py runs them on the kernel interpreter,
tests/test_gpu_triple_wide.py on the GPU.  ``reference64``, ``clustered_problem`` and ``near_problem`` come from
tests/_triplestreamcases.py.

1. Integer lattice (codebook and predictions in {-1, 0, 1}, margin 0): every product and every partial sum is an integer below
   2^24 (a distance <= 4 d, the loss sum <= 4 d K <= 2^24 for all shapes here), so every fp32 sum equals the float64 one in any
   order.  The kernel multiplies the loss sum by ONE factor, 1 / d or 1 / (d K) rounded once by the host, and the gradient sum
   by 2 / d or 2 / (d K): exact, hence bit-equal to float64, for 'sum' where d is a power of two and for 'mean' where K is one
   too; two roundings (factor, product), relative 2^-23 < 2^-22, elsewhere.

2. Real values against the same expressions in float64.  u = 2^-24.  One fp32 distance (|p|^2 - 2 p.e) + |e|^2 is within
   b = 4 d u (|p| + max|e|)^2 of the exact one in any order of its d products (the bound of _triplestreamcases.reference64; it
   holds for the MFMA blocking and for the direct difference pos); a term v_k = t_k + margin with |v_k| <= b on the float64 side
   is undecided and may be counted on either side.  A = the active or undecided codewords of a frame, n_A their number.
   loss:  a counted term is off by the two distance errors and the roundings of the subtraction and of the margin, 2 b +
     2 u |v| <= 3 b; an undecided one counted on one side only by |v| + 2 b <= 3 b.  The terms add up in chains of at most
     K / 4 + 2 additions and the sum is scaled with two roundings: at most (K + 4) u times the sum of the magnitudes.
       loss_b = scale / d  (3 b n_A + (K + 4) u (sum_active |v_k| + 3 b n_A))
   gradient, per channel c: the kernel forms scale (2 / d) (S - n e_trg) with S = sum_{k in mask} e_k, NOT sum (e_k - e_trg): the
     roundings scale with |e_k|, not with |e_k - e_trg|.
     - decisions: an undecided codeword on the other side moves the result by |e_k - e_trg| (the target's own row: 0; its bit
       is never set);
     - S: the second GEMM adds the rows of one 64-codeword tile in a chain on the matrix cores, order (m, r, g) -> codeword
       16 m + 4 g + r (inactive rows add an exact 0): at most 63 u sum_tile |e_k| (first order); the tile sums enter a
       compensated sum: 2 u |S| + O(u^2), at most 3 u sum |e_k|;
     - fma(-n, e_trg, S) and the subtraction of the compensation: 2 u (sum |e_k| + n |e_trg|); the factor 2 / (d K) and its
       product: 2 u of the same.
     Together under 70 u sum_A |e_k| + 4 u n_A |e_trg|; the budget takes 80 and 8:
       grad_b = scale (2 / d) (sum_{k undecided} |e_k - e_trg| + u (80 sum_{k in A} |e_k| + 8 n_A |e_trg|))
   Everything comes from the float64 side; no frame is excluded.  Largest share of a budget used: profiles/triple_wide.md.
"""
import ctypes
import functools

import torch

from _triplestreamcases import (RESIDENT, STREAMED, clustered_problem, last_kernel, near_problem, reference64, same_bits)
import _triplestreamcases as stream_cases

E_SHAPE = -2
WIDE = 'triple_loss_wide_kernel'
U = 2.0 ** -24

SHAPES = ((16, 7), (48, 100), (768, 333), (1024, 100), (2048, 72), (64, 1))              # d, K
NS = (1, 37, 300)                                                                         # a partial tile and several tiles
PARAMS = [(s, n) for s in range(len(SHAPES)) for n in NS]
IDS = ['d%d K%d N%d' % (SHAPES[s] + (n,)) for s, n in PARAMS]
INVARIANT_SHAPES = (0, 1, 5, 2, 3)
INVARIANT_IDS = ['d%d K%d' % SHAPES[s] for s in INVARIANT_SHAPES]
SHARED_SHAPES = ((64, 64), (256, 160), (512, 96))                                         # the other kernels take these too
SHARED_PARAMS = [(0, 37), (0, 300), (1, 37), (2, 37)]
SHARED_IDS = ['d%d K%d N%d' % (SHARED_SHAPES[s] + (n,)) for s, n in SHARED_PARAMS]
MODULES = ((1024, 100), (768, 333))
MODULE_IDS = ['Quantize(%d, %d)' % m for m in MODULES]


def run_wide(dev, p, trg, embed, margin, mean, frames=0):
    """msmc_triple_loss_wide directly -> (rc, lossh [N, 1], gp [N, d]) on the host; the outputs start as NaN"""
    from msmctts_amd.hip import lib, vq
    H, d, K = embed.shape
    N = p.shape[0]
    assert H == 1
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    pd, td = p.clone().to(dev), trg.clone().to(dev)
    lossh = torch.full((N, 1), float('nan')).to(dev)
    gp = torch.full((N, d), float('nan')).to(dev)
    L = lib.get()
    ws = lib.workspace(int(L.msmc_triple_loss_wide_workspace(N, d, K)), pd.device)
    L.msmc_triple_wide_set_frames(int(frames))
    try:
        rc = L.msmc_triple_loss_wide(lib.ptr(pd), lib.ptr(td), lib.ptr(et), lib.ptr(en), lib.ptr(lossh), lib.ptr(gp), N, d, K,
                                     float(margin), int(mean), lib.ptr(ws), ws.numel() * 4, lib.stream(pd))
    finally:
        L.msmc_triple_wide_set_frames(0)
    return rc, lossh.cpu(), gp.cpu()


# ---- 1. exact on an integer lattice -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_problem(d, K, N, seed):
    """codebook and predictions in {-1, 0, 1}; targets 0 and K - 1 planted; where K >= 8 codeword 5 is duplicated at K - 2 (an
    exact tie with the target for targets 5 and K - 2: t_k == 0 at k != trg); every third frame is far from its target, frames
    3 .. 5 are exactly a non-target codeword, frames 6 .. 8 exactly the target"""
    gen = torch.Generator().manual_seed(seed)
    embed = torch.randint(-1, 2, (1, d, K), generator=gen).float()
    if K >= 8:
        embed[:, :, K - 2] = embed[:, :, 5]
    trg = torch.randint(0, K, (N, 1), generator=gen)
    for i, k in enumerate((0, K - 1, 5 % K)[:N]):
        trg[i] = k
    rows = embed[0].t()[trg[:, 0]]
    noise = torch.randint(-1, 2, (N, d), generator=gen).float() * (torch.rand(N, d, generator=gen) < 0.1)
    p = (rows + noise).clamp(-1, 1)
    far = torch.arange(N) % 3 == 2
    p[far] = torch.randint(-1, 2, (int(far.sum()), d), generator=gen).float()
    for n in range(3, min(N, 6)):
        p[n] = embed[0][:, int(trg[n, 0] + 3) % K]
    for n in range(6, min(N, 9)):
        p[n] = rows[n]
    return p.contiguous(), trg, embed


def check_lattice(dev, s, N):
    d, K = SHAPES[s]
    assert 4 * d * K <= 2 ** 24
    p, trg, embed = lattice_problem(d, K, N, 6100 + s)
    assert float(p.abs().max()) <= 1 and float(embed.abs().max()) <= 1
    if N > 1:
        assert int(trg[0]) == 0 and int(trg[1]) == K - 1
    for mean in (0, 1):
        ref = reference64(p, trg, embed, 0.0, mean)
        if N >= 37 and K >= 8:
            assert float(ref['active'].double().sum(-1).mean()) > 1, 'the lattice case has no hinge terms'
            assert bool((ref['t'][2, :, K - 2] == 0).all()), 'the duplicate of the target is not an exact tie'
        want_l, want_g = ref['loss'].float(), ref['gp'].float()
        exact = (d & (d - 1)) == 0 and ((not mean) or (K & (K - 1)) == 0)
        rc, l1, g1 = run_wide(dev, p, trg, embed, 0.0, mean)
        assert rc == 0 and last_kernel() == WIDE, (rc, last_kernel())
        if exact:
            assert same_bits(l1, want_l), ('lossh', mean, (l1 - want_l).abs().max().item())
            assert same_bits(g1, want_g), ('gp', mean, (g1 - want_g).abs().max().item())
        else:
            rel = 2.0 ** -22
            assert bool(((l1.double() - ref['loss']).abs() <= rel * ref['loss'].abs()).all()), ('lossh', mean)
            assert bool(((g1.double() - ref['gp']).abs() <= rel * ref['gp'].abs()).all()), ('gp', mean)


# ---- 2. real values against float64 with the derived budget -----------------------------------------------------------------------
def budgets(ref, margin):
    """(loss budget [N, 1], gradient budget [N, d], undecided [N, 1, K]) of the module docstring, from the float64 side alone"""
    H, K, d = ref['rows'].shape
    N = ref['t'].shape[0]
    b = ref['b']                                                                        # [N, 1]
    v = ref['t'] + margin
    und = v.abs() <= b.unsqueeze(-1)                                                    # [N, 1, K]
    in_a = ref['active'] | und
    n_a = in_a.double().sum(-1)                                                         # [N, 1]
    sum_v = (ref['active'] * v.abs()).sum(-1)
    loss_b = ref['scale'] / d * (3 * b * n_a + (K + 4) * U * (sum_v + 3 * b * n_a))
    # sum_{k undecided} |e_k - e_trg| (the target's own row: 0), 32 frames at a time: [32, 1, K, d] in float64
    flips = torch.cat([torch.einsum('nhk,nhkd->nhd', und[i:i + 32].double(),
                                    (ref['rows'].unsqueeze(0) - ref['et'][i:i + 32].unsqueeze(2)).abs()) for i in range(0, N, 32)])
    s_abs = torch.einsum('nhk,hkd->nhd', in_a.double(), ref['rows'].abs())              # (the target, where in A, counted too)
    grad_b = ref['scale'] * (2.0 / d) * (flips + U * (80 * s_abs + 8 * n_a.unsqueeze(-1) * ref['et'].abs()))
    return loss_b, grad_b.reshape(N, H * d), und


def check_real_values(dev, s, N, report=None):
    d, K = SHAPES[s]
    p, trg, embed = clustered_problem(1, d, K, N, 6200 + s)
    for mean in (0, 1):
        ref = reference64(p, trg, embed, 1e-6, mean)
        loss_b, grad_b, und = budgets(ref, 1e-6)
        rc, l1, g1 = run_wide(dev, p, trg, embed, 1e-6, mean)
        assert rc == 0 and last_kernel() == WIDE, (rc, last_kernel())
        assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(g1).all())
        le = (l1.double() - ref['loss']).abs()
        ge = (g1.double() - ref['gp']).abs()
        share = lambda e, bud: float(torch.where(bud > 0, e / bud, (e > 0).double() * float('inf')).max())
        figures = dict(shape=(d, K, N), mean=mean, loss_err_over_budget=share(le, loss_b), grad_err_over_budget=share(ge, grad_b),
                       mean_active=float(ref['active'].double().sum(-1).mean()),
                       frames_with_undecided=float((und & (ref['t'] != 0)).any(-1).any(-1).double().mean()))
        print(figures)
        if report is not None:
            report.append(figures)
        assert bool((le <= loss_b).all()), figures
        assert bool((ge <= grad_b).all()), figures


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------------
def check_invariance(dev, s):
    d, K = SHAPES[s]
    p, trg, embed = clustered_problem(1, d, K, 300, 6300 + s)
    rc, l0, g0 = run_wide(dev, p, trg, embed, 1e-6, 1)
    assert rc == 0 and last_kernel() == WIDE
    rc, l1, g1 = run_wide(dev, p, trg, embed, 1e-6, 1)
    assert rc == 0 and same_bits(l1, l0) and same_bits(g1, g0), 'two identical calls differ'
    rc, l2, g2 = run_wide(dev, p[:37].contiguous(), trg[:37].contiguous(), embed, 1e-6, 1)
    assert rc == 0
    assert same_bits(l2, l0[:37]) and same_bits(g2, g0[:37]), 'rows 0 .. 36 depend on the other frames of the call'
    for frames in (16, 32, 64):                                    # ... nor on the frames per workgroup
        rc, l3, g3 = run_wide(dev, p, trg, embed, 1e-6, 1, frames)
        assert rc == 0 and same_bits(l3, l0) and same_bits(g3, g0), frames


# ---- 4. agreement with the resident / streamed kernels ------------------------------------------------------------------------------
def check_agrees_with_the_other_kernels(dev, s, N):
    """both kernels are within their own float64 budgets, so they differ by at most the sum of the two"""
    d, K = SHARED_SHAPES[s]
    p, trg, embed = clustered_problem(1, d, K, N, 6400 + s)
    for mean in (0, 1):
        ref = reference64(p, trg, embed, 1e-6, mean)
        loss_b, grad_b, _ = budgets(ref, 1e-6)
        loss_o, grad_o, _ = stream_cases.budgets(ref, 1e-6)
        from msmctts_amd.hip import losses
        rc, l0, g0 = stream_cases.run(dev, p, trg, embed, 1e-6, mean, None if losses.triple_resident(d, K) else 0)
        assert rc == 0 and last_kernel() == (RESIDENT if losses.triple_resident(d, K) else STREAMED), (rc, last_kernel())
        rc, l1, g1 = run_wide(dev, p, trg, embed, 1e-6, mean)
        assert rc == 0 and last_kernel() == WIDE, (rc, last_kernel())
        assert bool(((l1.double() - ref['loss']).abs() <= loss_b).all()) and bool(((g1.double() - ref['gp']).abs() <= grad_b).all())
        assert bool(((l1 - l0).double().abs() <= loss_b + loss_o).all()), ('lossh', mean)
        assert bool(((g1 - g0).double().abs() <= grad_b + grad_o).all()), ('gp', mean)


# ---- 5. module and routing ------------------------------------------------------------------------------------------------------------
def check_module(dev, m):
    from msmctts_amd.networks.vqgantts.modules import Quantize
    from oracle import predictor as op
    D, K = MODULES[m]
    B, T = 3, 13
    p, trg, embed = clustered_problem(1, D, K, B * T, 6500 + m)
    q = Quantize(D, K)
    q.embed.copy_(embed[0])
    q = q.to(dev)
    gen = torch.Generator().manual_seed(6600 + m)
    wts = torch.rand(B, T, generator=gen)
    trg_in = trg[:, 0].view(B, T).to(dev)
    for reduction in ('sum', 'mean'):
        ref = reference64(p, trg, embed, 1e-6, reduction == 'mean')
        loss_b, grad_b, _ = budgets(ref, 1e-6)
        # the oracle (reference expressions) evaluated in float64
        p64 = p.double().view(B, T, D).requires_grad_(True)
        want = op.triple_loss(p64, trg[:, 0].view(B, T), embed[0].double(), reduction)
        (want * wts.double()).sum().backward()
        p1 = p.view(B, T, D).clone().to(dev).requires_grad_(True)
        got = q.compute_triple_loss(p1, trg_in, reduction=reduction)
        assert last_kernel() == WIDE, last_kernel()
        assert got.shape == (B, T)
        (got * wts.to(dev)).sum().backward()
        le = (got.detach().cpu().double() - want.detach()).abs().view(B * T)
        assert bool((le <= loss_b[:, 0]).all()), (reduction, float((le / loss_b[:, 0]).max()))
        ge = (p1.grad.cpu().double() - p64.grad).abs().view(B * T, D)
        # (the product with the incoming gradient: one more rounding of the result)
        gb = grad_b * wts.double().view(B * T, 1) + U * p64.grad.abs().view(B * T, D)
        assert bool((ge <= gb).all()), (reduction, float((ge / gb).max()))
    # reduction='none' and adaptive_margin keep the stock chain: the [B, T, K] tensor, no launch of the kernel
    before = short_call(dev)
    none = q.compute_triple_loss(p.view(B, T, D).to(dev), trg_in, reduction='none')
    assert none.shape == (B, T, K) and last_kernel() == before
    want = op.triple_loss(p.view(B, T, D), trg[:, 0].view(B, T), embed[0], 'none')
    assert float((none.cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    q.compute_triple_loss(p.view(B, T, D).to(dev), trg_in, reduction='sum', adaptive_margin=True)
    assert last_kernel() == before


def short_call(dev):
    """a resident-kernel call, so that the observer names another kernel than the wide one -> that name"""
    from msmctts_amd.hip import losses, vq
    p, trg, embed = near_problem(4, 64, 256, 37, 3.0, 5101)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    losses.triple_loss(p.to(dev), trg.to(dev), et, en, 'sum')
    assert last_kernel() == RESIDENT, last_kernel()
    return RESIDENT


def check_wrapper_routes(dev):
    """hip/losses.py triple_loss: the shapes the other kernels take keep them; wide=True forces the wide entry; a width only
    the wide kernel takes reaches it unasked"""
    from msmctts_amd.hip import losses, vq
    short_call(dev)                                                                     # (4, 64, 256): resident
    p, trg, embed = near_problem(1, 256, 160, 37, 3.0, 5202)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    losses.triple_loss(p.to(dev), trg.to(dev), et, en, 'mean')
    assert last_kernel() == STREAMED, last_kernel()
    pa = p.clone().to(dev).requires_grad_(True)
    la = losses.triple_loss(pa, trg.to(dev), et, en, 'mean', wide=True)
    assert last_kernel() == WIDE, last_kernel()
    rc, l1, g1 = run_wide(dev, p, trg, embed, 1e-6, 1)
    assert rc == 0 and same_bits(la.detach().cpu(), l1)
    w = torch.arange(37).view(37, 1).float() / 100
    (la * w.to(dev)).sum().backward()
    assert same_bits(pa.grad.cpu(), g1 * w)
    assert losses.triple_wide_takes(1, 768, 333) and not losses.triple_kernel_takes(768, 333)
    assert not losses.triple_wide_takes(2, 768, 333) and not losses.triple_wide_takes(1, 40, 8)
    assert not losses.triple_wide_takes(1, 2064, 8) and not losses.triple_wide_takes(1, 64, 0)
    p, trg, embed = near_problem(1, 48, 100, 37, 3.0, 6700)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    lb = losses.triple_loss(p.to(dev), trg.to(dev), et, en, 'sum')
    assert last_kernel() == WIDE, last_kernel()
    rc, l1, _ = run_wide(dev, p, trg, embed, 1e-6, 0)
    assert rc == 0 and same_bits(lb.cpu(), l1)
    with_heads = near_problem(2, 48, 100, 5, 3.0, 6701)
    et, en = vq.vq_prepare(with_heads[2].to(dev), frames=0)
    try:
        losses.triple_loss(with_heads[0].to(dev), with_heads[1].to(dev), et, en, 'sum', wide=True)
    except RuntimeError:
        pass
    else:
        raise AssertionError('two heads went to the wide entry')


# ---- 6. refusals and the empty input ------------------------------------------------------------------------------------------------
def check_refusals(dev):
    from msmctts_amd.hip import lib, vq
    L = lib.get()
    N = 5
    p, trg, embed = near_problem(1, 64, 64, 37, 0.05, 5100)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    big = torch.zeros(37 * 2064 + 4).to(dev)                       # frames for every width tried below
    td = trg.to(dev)
    lossh = torch.full((37, 1), float('nan')).to(dev)
    gp = torch.full((37 * 2064,), float('nan')).to(dev)
    ws = torch.zeros(37 * 64).to(dev)

    def call(pp, n, d, K, ws_bytes=None):
        return L.msmc_triple_loss_wide(pp, lib.ptr(td), lib.ptr(et), lib.ptr(en), lib.ptr(lossh), lib.ptr(gp), n, d, K, 1e-6, 0,
                                       lib.ptr(ws), ws.numel() * 4 if ws_bytes is None else ws_bytes, lib.stream(td))

    def untouched():
        return bool(torch.isnan(lossh.cpu()).all()) and bool(torch.isnan(gp.cpu()).all())
    for d, K in ((40, 64), (2064, 1), (64, 0), (8, 64)):           # the codebook behind et has 64 x 64 floats: enough for each
        assert call(lib.ptr(big), N, d, K) == E_SHAPE, (d, K)
        assert int(L.msmc_triple_loss_wide_workspace(N, d, K)) == 0
        assert untouched(), 'a refused call launched'
    assert call(lib.ptr(big), -1, 64, 64) == E_SHAPE and untouched()
    off = big[1:1 + 37 * 64]
    assert off.data_ptr() % 16 == 4
    assert call(ctypes.c_void_p(off.data_ptr()), 37, 64, 64) == E_SHAPE and untouched()
    assert call(lib.ptr(big), 37, 64, 64, ws_bytes=37 * 8 - 1) == -3 and untouched()      # MSMC_E_WORKSPACE
    assert int(L.msmc_triple_loss_wide_workspace(37, 64, 65)) == 37 * 2 * 8
    # N = 0: 0 and nothing written
    assert call(lib.ptr(big), 0, 64, 64) == 0 and untouched()
    # the streamed entry keeps its refusal
    rc, l, g = stream_cases.run(dev, torch.zeros(N, 160), torch.zeros(N, 1, dtype=torch.int64), torch.ones(1, 160, 32), 1e-6, 0, 0)
    assert rc == E_SHAPE and bool(torch.isnan(l).all()) and bool(torch.isnan(g).all())


# ---- 7. the symbols -------------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    assert 'msmc_triple_loss_wide' in lib.exported_symbols()
    assert 'msmc_triple_loss_wide_workspace' in lib.exported_symbols()
    assert 'msmc_triple_wide_set_frames' in lib.debug_symbols()
    assert isinstance(lib.get().msmc_triple_loss_wide, ctypes._CFuncPtr)
    assert isinstance(lib.get().msmc_triple_loss_wide_workspace, ctypes._CFuncPtr)
