"""Shared cases of the unit predictor's loss and label decoding: csrc/unit_ce.hip (msmc_unit_ce_fwd / _bwd, msmc_unit_argmax),
their host side (msmctts_amd/hip/unit_ce.py ``masked_cross_entropy`` / ``unit_argmax``), the ``'softmax'`` method of
``MultiStageQuantizer.compute_embedding_loss``, ``KMeansVQGANEmb.compute_embedding_loss`` / ``decode_units`` and
``UnitPredictorTrainer``.  tests/test_unit_ce_emu.py runs the cases of at most a few hundred thousand elements on the kernel
interpreter, tests/test_gpu_unit_ce.py all of them on the GPU.

Reference: ``restated`` -- the definition in float64 numpy on the stored logits (bf16 logits upcast exactly).

EXACT: the arg-max (comparisons only; lowest index on ties), -1 on padded rows, ``correct``, the zero bits of the gradient on
padded rows, ignored rows and in the columns K .. ld - 1, K = 1 (loss 0, gradient 0), bits between two runs, and bits with NaN
in the padded logits.

BOUND (``row_bound`` / ``loss_bound`` / ``grad_bound``): expf and logf differ between the GPU, the interpreter and numpy, so lse,
loss and gradient are compared within a bound derived from the ORDER documented in csrc/unit_ce.hip.  u = 2^-24 (fp32 unit
roundoff); expf and logf are stated at 1 ulp = 2u relative (HIP math API; glibc likewise).
* A lane's chain has at most c = ceil(K / 64) + 8 additions (its share of the row, the tail element) and the butterfly adds 6:
  positive terms, so the sum s carries at most (c + 6) u relative from the additions.
* Every term expf(x - m) carries 2u from expf and |x - m| u from the rounded difference; terms with |x - m| > 104 are exactly 0
  in fp32, so at most (2 + 104) u, and one more u where the term is scaled.  A rescale s <- s expf(m - m') costs the same
  (2 + 104 + 1) u; a lane rescales at most once per vector and the butterfly once per step: R = c + 6 rescales at most.
  rel(s) <= u (c + 6 + 107 (R + 1)).
* lse = m + logf(s): |d lse| <= rel(s) + 2u |log s| + u |lse|, and the row loss lse - x_t adds u |loss|.  With A = max |x| over
  the row: |log s| <= log K, |lse| <= A + log K, |loss| <= 2 A + log K.  lse_bound = rel(s) + u (3 log K + A),
  row_bound = lse_bound + u (log K + 2 A).
* The loss adds N_rows non-negative row losses in fp32 chains of at most N_rows additions (rows of a wave, four waves, the
  partials of a lane, six butterfly steps) and divides twice-rounded: (N_rows + 12) u relative on the sum.
* The gradient (expf(x - lse) - [k = t]) scale: p = expf(x - lse) <= 1 carries 2u p + u |x - lse| p (<= u / e ... <= u) +
  lse_bound p; the subtraction, gout out[1] and the product one u each, out[1] = 1 / (float)tot two: |dg| <= scale (lse_bound + 8u).
  bf16 gradients add the output rounding, 2^-8 |g| per element (8 significant bits, round to nearest even).
Each bound is asserted to stay inside the project's bar of 1e-3 relative to the tensor's maximum (tests/_embcases.py FP32_BAR;
for bf16 gradients the part before the output rounding -- the rounding itself is the format's, not the computation's).
"""
import ctypes
import functools
import math
import os

import numpy as np
import torch

from _embcases import FP32_BAR, _raises

E_SHAPE, E_WORKSPACE = -2, -3
POISON = -99
U = 2.0 ** -24


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ceil8(k):
    return (k + 7) // 8 * 8


# ---- (a) the kernels, directly ------------------------------------------------------------------------------------------------------------
# name: B, T, K, ld, bf16, int64 lengths, offset (elements the logits start into their 16-byte aligned allocation), lengths
def _case(B, T, K, ld=None, bf16=False, len64=True, offset=0, lengths=None):
    return dict(B=B, T=T, K=K, ld=K if ld is None else ld, bf16=bf16, len64=len64, offset=offset, lengths=lengths)


CASES = {
    # K: idle lanes, one element per lane, a tail, unit sizes that are no multiple of 8, more than UC_UNROLL vectors per lane
    'K1': _case(3, 5, 1), 'K8': _case(3, 5, 8), 'K63': _case(3, 5, 63), 'K64': _case(3, 5, 64), 'K65': _case(3, 5, 65),
    'K100': _case(3, 5, 100), 'K500': _case(3, 5, 500, len64=False), 'K2000': _case(3, 5, 2000), 'K4100': _case(3, 5, 4100),
    'K8 bf16': _case(3, 5, 8, bf16=True), 'K65 bf16': _case(3, 5, 65, bf16=True), 'K2000 bf16': _case(3, 5, 2000, bf16=True, len64=False),
    'K4100 bf16': _case(3, 5, 4100, bf16=True),
    # ld = ceil8(K) > K: the vector path with a tail and zero columns
    'K100 ld104': _case(3, 5, 100, 104), 'K500 ld504': _case(3, 5, 500, 504), 'K100 ld104 bf16': _case(3, 5, 100, 104, bf16=True),
    'K500 ld504 bf16': _case(3, 5, 500, 504, bf16=True, len64=False),
    # a base that is not 16-byte aligned: the scalar path on a width the vector path would take
    'K100 ld104 off1': _case(3, 5, 100, 104, offset=1), 'K100 ld104 bf16 off1': _case(3, 5, 100, 104, bf16=True, offset=1),
    'B1': _case(1, 7, 65, lengths=(6,)),
    'no valid row': _case(2, 4, 8, lengths=(0, 0)),
    # 771 rows: no multiple of the 4 rows of a workgroup, 193 partials -- more than one pass of the second launch's 64 lanes
    'rows 3x257': _case(3, 257, 8, len64=False, lengths=(257, 1, 130)),
}
SMALL = [n for n, c in CASES.items() if c['B'] * c['T'] * c['ld'] <= 300000]


def _round_bf16(a):
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> logits [B, T, ld] fp32 (bf16 cases: already rounded), target [B, T], lengths [B].  Every other valid row has its target's
    logit raised, the rest have it lowered (so that ``correct`` is neither 0 nor all), a tie between the two largest entries sits in one valid row, targets
    -1 and K sit on valid rows; behind ``lengths`` the rows hold finite logits and valid targets (read by mistake they count);
    the columns K .. ld - 1 hold large values (read as classes they win the arg-max)."""
    c = CASES[name]
    B, T, K, ld = c['B'], c['T'], c['K'], c['ld']
    rng = np.random.default_rng(7000 + 13 * B + 17 * T + 19 * K + ld + 5 * c['offset'] + c['bf16'])
    x = rng.standard_normal((B, T, ld)).astype(np.float32) * 2
    target = rng.integers(0, K, (B, T)).astype(np.int64)
    lengths = np.array(c['lengths'] if c['lengths'] is not None else ([T, 0, 1][:B]), dtype=np.int64)
    valid = np.argwhere(np.arange(T)[None, :] < lengths[:, None])
    raise_ = rng.random((B, T)) < 0.5
    for i, (b, t) in enumerate(valid):                # (valid rows: alternately)
        raise_[b, t] = i % 2 == 0
    bb, tt = np.nonzero(np.ones((B, T), dtype=bool))
    x[bb, tt, target[bb, tt]] += np.where(raise_, 8, -8)[bb, tt].astype(np.float32)
    x[:, :, K:] = 50
    if len(valid) >= 4:
        target[tuple(valid[1])] = -1
        target[tuple(valid[2])] = K
        if K >= 3:
            b, t = valid[3]
            x[b, t, K - 1] = x[b, t, 1] = x[b, t, :K].max() + 1           # a tie: index 1 wins
    if c['bf16']:
        x = _round_bf16(x)
    return x, target, lengths


def restated(x, target, lengths, K, gout=1.0):
    """float64: lse [B, T], pred [B, T], loss, correct, glogits [B, T, ld], row losses, valid, live"""
    B, T, ld = x.shape
    z = x[:, :, :K].astype(np.float64)
    valid = np.arange(T)[None, :] < lengths[:, None]
    live = valid & (target >= 0) & (target < K)
    m = z.max(-1)
    lse = m + np.log(np.exp(z - m[..., None]).sum(-1))
    pred = np.where(valid, z.argmax(-1), -1).astype(np.int64)
    tsafe = np.where(live, target, 0)
    rows = np.where(live, lse - np.take_along_axis(z, tsafe[..., None], -1)[..., 0], 0.0)
    tot = float(lengths.sum())
    loss = rows.sum() / tot if tot > 0 else 0.0
    correct = int((live & (pred == target)).sum())
    g = np.zeros((B, T, ld))
    p = np.exp(z - lse[..., None])
    np.put_along_axis(p, tsafe[..., None], np.take_along_axis(p, tsafe[..., None], -1) - 1.0, -1)
    g[:, :, :K] = np.where(live[..., None], p, 0.0) * (gout / tot if tot > 0 else 0.0)
    return dict(lse=np.where(valid, lse, 0.0), pred=pred, loss=loss, correct=correct, g=g, rows=rows, valid=valid, live=live)


def lse_bound(K, A):
    c = -(-K // 64) + 8
    R = c + 6
    return U * (c + 6 + 107 * (R + 1)) + U * (3 * math.log(K) + A)


def row_bound(K, A):
    return lse_bound(K, A) + U * (math.log(K) + 2 * A)


def loss_bound(K, x, ref, lengths):
    A = np.abs(x[:, :, :K]).max(-1)
    tot = max(float(lengths.sum()), 1.0)
    n = int(ref['live'].sum())
    return float((row_bound(K, A) * ref['live']).sum() / tot + U * (n + 12) * np.abs(ref['rows']).sum() / tot)


def grad_bound(K, x, lengths, gout):
    A = np.abs(x[:, :, :K]).max(-1)
    return abs(gout) / max(float(lengths.sum()), 1.0) * (lse_bound(K, A) + 8 * U)            # [B, T]


def _at(dev, values, offset, dtype):
    """a device copy of ``values`` that starts ``offset`` elements into a 16-byte aligned allocation"""
    buf = torch.zeros(values.size + 16, dtype=dtype).to(dev)
    view = buf[offset:offset + values.size].view(values.shape)
    view.copy_(torch.from_numpy(values).to(dtype))
    assert view.data_ptr() % 16 == (offset * view.element_size()) % 16
    return view


def run_kernels(dev, x, target, lengths, K, bf16=False, len64=True, offset=0, gout=0.75, ws_bytes=None, want_pred=True):
    """the three entry points on poisoned outputs -> dict(rc_fwd, rc_bwd, rc_arg, lse, pred, out, correct, g, arg)"""
    from msmctts_amd.hip import lib
    L = lib.get()
    B, T, ld = x.shape
    dt = torch.bfloat16 if bf16 else torch.float32
    xd = _at(dev, x, offset, dt)
    td = torch.from_numpy(target).to(dev)
    ld_ = torch.from_numpy(lengths.astype(np.int64 if len64 else np.int32)).to(dev)
    lse = torch.full((B, T), float(POISON)).to(dev)
    pred = torch.full((B, T), POISON, dtype=torch.int64).to(dev)
    arg = torch.full((B, T), POISON, dtype=torch.int64).to(dev)
    out = torch.full((2,), float(POISON)).to(dev)
    correct = torch.full((1,), POISON, dtype=torch.int64).to(dev)
    gd = _at(dev, np.full(x.shape, float(POISON), dtype=np.float32), offset, dt)
    need = int(L.msmc_unit_ce_workspace(B, T))
    ws = torch.empty(max(need // 4, 4) + 4).to(dev)
    go = torch.tensor([gout]).to(dev)
    st = lib.stream(xd)
    r = {}
    r['rc_fwd'] = L.msmc_unit_ce_fwd(lib.ptr(xd), int(bf16), lib.ptr(td), lib.ptr(ld_), int(len64), lib.ptr(lse), lib.ptr(pred) if want_pred else None,
                                     lib.ptr(out), lib.ptr(correct), lib.ptr(ws), need if ws_bytes is None else ws_bytes, B, T, K, ld, st)
    if r['rc_fwd'] == 0:
        r['rc_bwd'] = L.msmc_unit_ce_bwd(lib.ptr(xd), int(bf16), lib.ptr(td), lib.ptr(ld_), int(len64), lib.ptr(lse), lib.ptr(out), lib.ptr(go),
                                         lib.ptr(gd), B, T, K, ld, st)
    r['rc_arg'] = L.msmc_unit_argmax(lib.ptr(xd), int(bf16), lib.ptr(ld_), int(len64), lib.ptr(arg), B, T, K, ld, st)
    r.update(lse=lse.cpu().numpy(), pred=pred.cpu().numpy(), arg=arg.cpu().numpy(), out=out.cpu().numpy(), correct=int(correct.cpu()[0]),
             g=gd.float().cpu().numpy(), g_bits=gd.cpu().view(torch.int16 if bf16 else torch.int32).numpy(), need=need)
    return r


def compare(name, x, target, lengths, K, r, bf16, gout=0.75):
    ref = restated(x, target, lengths, K, gout)
    valid, live = ref['valid'], ref['live']
    assert r['rc_fwd'] == 0 and r['rc_bwd'] == 0 and r['rc_arg'] == 0, (name, r['rc_fwd'], r.get('rc_bwd'), r['rc_arg'])
    # exact
    assert np.array_equal(r['pred'], ref['pred']), (name, np.argwhere(r['pred'] != ref['pred'])[:4].tolist())
    assert np.array_equal(r['arg'], ref['pred']), name
    assert r['correct'] == ref['correct'], (name, r['correct'], ref['correct'])
    dead = np.broadcast_to(~live[..., None], x.shape) | (np.arange(x.shape[2]) >= K)[None, None, :]
    assert not r['g_bits'][dead].any(), '%s: a padded / ignored row or a column behind K is not +0' % name
    assert not (r['lse'][~valid] != 0).any()
    assert np.isfinite(r['lse']).all() and np.isfinite(r['out']).all() and np.isfinite(r['g']).all(), name
    # within the bound
    tot = float(lengths.sum())
    A = np.abs(x[:, :, :K]).max(-1)
    rb = lse_bound(K, A)
    err = np.abs(r['lse'] - ref['lse'])
    print('%s: lse err %.3e (bound %.3e)' % (name, err[valid].max() if valid.any() else 0.0, rb[valid].max() if valid.any() else 0.0))
    assert (err <= rb)[valid].all(), (name, float(err[valid].max()))
    if valid.any():
        assert rb[valid].max() <= FP32_BAR * max(1.0, np.abs(ref['lse']).max()), name
    lb = loss_bound(K, x, ref, lengths)
    print('%s: loss %.7g, restated %.7g, bound %.3e' % (name, r['out'][0], ref['loss'], lb))
    assert abs(float(r['out'][0]) - ref['loss']) <= lb, name
    if K > 1:                                   # (K = 1: the loss is exactly 0, checked as such by the caller)
        assert lb <= FP32_BAR * abs(ref['loss']), name
    if tot > 0:
        assert abs(float(r['out'][1]) - 1.0 / tot) <= 2 * U / tot
    else:
        assert float(r['out'][0]) == 0.0 and float(r['out'][1]) == 0.0 and r['correct'] == 0, name
    gb = grad_bound(K, x, lengths, gout)[..., None]
    gmax = np.abs(ref['g']).max()
    gerr = np.abs(r['g'] - ref['g'])
    slack = gb + (2.0 ** -8 * np.abs(ref['g']) if bf16 else 0.0)
    print('%s: gradient err %.3e, max %.3e' % (name, gerr.max(), gmax))
    assert (gerr <= slack).all(), (name, float(gerr.max()))
    if gmax > 0:
        assert gb.max() <= FP32_BAR * gmax, name
    return ref


def check_case(dev, name):
    c = CASES[name]
    x, target, lengths = problem(name)
    K = c['K']
    kw = dict(bf16=c['bf16'], len64=c['len64'], offset=c['offset'])
    saved = os.environ.get('MSMC_EMU_CUS')
    os.environ['MSMC_EMU_CUS'] = '256'          # (interpreter: the chip's grid -- one workgroup per group of rows up to 2048)
    try:
        r = run_kernels(dev, x, target, lengths, K, **kw)
        ref = compare(name, x, target, lengths, K, r, c['bf16'])
        if name == 'rows 3x257':
            assert r['need'] >= 193 * 8, 'the case does not reach a second pass over the partials'
        if K == 1:
            assert float(r['out'][0]) == 0.0 and not r['g'].any(), 'K = 1: the loss is exactly 0 and so is the gradient'
        if ref['valid'].sum() >= 4:
            assert (~ref['live'] & ref['valid']).sum() == 2 and (K == 1 or 0 < ref['correct'] < ref['live'].sum())
        # the same inputs: the same bits; pred is optional
        r2 = run_kernels(dev, x, target, lengths, K, want_pred=False, **kw)
        assert all(same_bits(r[k], r2[k]) for k in ('lse', 'out', 'g_bits', 'arg')) and (r2['pred'] == POISON).all(), name
        # NaN in the padded logits: never read
        xp = x.copy()
        xp[~ref['valid']] = np.nan
        r3 = run_kernels(dev, xp, target, lengths, K, **kw)
        assert all(same_bits(r[k], r3[k]) for k in ('lse', 'out', 'g_bits', 'pred', 'arg')) and r3['correct'] == r['correct'], name
    finally:
        if saved is None:
            del os.environ['MSMC_EMU_CUS']
        else:
            os.environ['MSMC_EMU_CUS'] = saved


def check_strided_grid(dev):
    """the interpreter's own grid (8 workgroups per 'CU' of 3): workgroups stride over the groups of rows; the same labels and
    counts, loss and gradient within the bound"""
    name = 'rows 3x257'
    x, target, lengths = problem(name)
    c = CASES[name]
    r = run_kernels(dev, x, target, lengths, c['K'], len64=c['len64'])
    compare(name + ' (strided)', x, target, lengths, c['K'], r, False)


def check_extreme_rows(dev):
    """entries of +-1e4 and a constant row, fp32: nothing overflows, the constant row's loss is log K within the bound"""
    B, T, K = 1, 4, 500
    rng = np.random.default_rng(7100)
    x = rng.standard_normal((B, T, K)).astype(np.float32)
    x[0, 0] = np.where(rng.random(K) < 0.5, 1e4, -1e4).astype(np.float32)
    x[0, 1] = 3.25
    x[0, 2, 7] = 1e4
    x[0, 3, 9] = -1e4
    target = np.array([[int(np.argmax(x[0, 0])), 11, 7, 9]], dtype=np.int64)
    lengths = np.array([T], dtype=np.int64)
    r = run_kernels(dev, x, target, lengths, K)
    compare('extreme rows', x, target, lengths, K, r, False)
    only = np.array([[0, 11, 0, 0]], dtype=np.int64)
    one = run_kernels(dev, x[:, 1:2].copy(), only[:, 1:2].copy(), np.array([1], dtype=np.int64), K)
    assert abs(float(one['out'][0]) - math.log(K)) <= row_bound(K, 3.25) + 2 * U * math.log(K), float(one['out'][0])
    assert one['pred'][0, 0] == 0, 'a constant row: the lowest index'


def check_refusals(dev):
    from msmctts_amd.hip import lib
    L = lib.get()
    x, target, lengths = problem('K100 ld104')
    B, T, ld = x.shape

    def untouched(r):
        return ((r['lse'] == POISON).all() and (r['pred'] == POISON).all() and (r['out'] == POISON).all() and r['correct'] == POISON
                and (r['g'] == POISON).all() and (r['arg'] == POISON).all())
    for K in (0, -1, ld + 1):
        r = run_kernels(dev, x, target, lengths, K)
        assert r['rc_fwd'] == E_SHAPE and r['rc_arg'] == E_SHAPE and untouched(r), K
    need = int(L.msmc_unit_ce_workspace(B, T))
    assert need > 0 and need % 16 == 0
    r = run_kernels(dev, x, target, lengths, 100, ws_bytes=need - 1)
    assert r['rc_fwd'] == E_WORKSPACE and (r['lse'] == POISON).all() and (r['out'] == POISON).all() and r['correct'] == POISON
    for b, t in ((0, 5), (3, 0), (-1, 5), (3, -2), (1 << 16, 1 << 15)):
        assert int(L.msmc_unit_ce_workspace(b, t)) == 0, (b, t)
    xd, td, ld_ = torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(lengths).to(dev)
    o = torch.full((B, T, ld), float(POISON)).to(dev)
    oi = torch.full((B, T), POISON, dtype=torch.int64).to(dev)
    ws = torch.empty(1024).to(dev)
    st = lib.stream(xd)
    for b, t, dtype in ((0, T, 0), (B, 0, 0), (B, T, 2), (B, T, -1)):
        rc = L.msmc_unit_ce_fwd(lib.ptr(xd), dtype, lib.ptr(td), lib.ptr(ld_), 1, lib.ptr(o), lib.ptr(oi), lib.ptr(o), lib.ptr(oi), lib.ptr(ws), 4096,
                                b, t, 100, ld, st)
        assert rc == E_SHAPE, (b, t, dtype, rc)
        rc = L.msmc_unit_ce_bwd(lib.ptr(xd), dtype, lib.ptr(td), lib.ptr(ld_), 1, lib.ptr(ws), lib.ptr(ws), lib.ptr(ws), lib.ptr(o), b, t, 100, ld, st)
        assert rc == E_SHAPE, (b, t, dtype, rc)
        assert L.msmc_unit_argmax(lib.ptr(xd), dtype, lib.ptr(ld_), 1, lib.ptr(oi), b, t, 100, ld, st) == E_SHAPE
    assert bool((o.cpu() == POISON).all()) and bool((oi.cpu() == POISON).all())
    from msmctts_amd.hip import unit_ce
    with _raises(RuntimeError, 'msmc_unit_ce_fwd failed with code -2'):
        unit_ce.masked_cross_entropy(xd, td, ld_, classes=ld + 1)
    with _raises(RuntimeError, 'msmc_unit_argmax failed with code -2'):
        unit_ce.unit_argmax(xd, ld_, classes=0)
    with _raises(TypeError, 'lengths'):
        unit_ce.masked_cross_entropy(xd, td, [5, 0, 1])


# ---- (b) autograd -------------------------------------------------------------------------------------------------------------------------
def chain64(logits, target, lengths):
    """the parent's operator chain in float64: cross_entropy(reduction='none'), mask, sum, / sum of lengths"""
    import torch.nn.functional as F
    B, T, K = logits.shape
    loss = F.cross_entropy(logits.reshape(-1, K), target.reshape(-1), reduction='none').view(B, T)
    pad = torch.arange(T, device=logits.device)[None, :] >= lengths[:, None]
    return loss.masked_fill(pad, 0).sum() / lengths.sum()


def check_autograd(dev, bf16=False):
    from msmctts_amd.hip import unit_ce
    B, T, K = 3, 9, 100
    rng = np.random.default_rng(7200 + bf16)
    x = (rng.standard_normal((B, T, K)) * 2).astype(np.float32)
    if bf16:
        x = _round_bf16(x)
    target = rng.integers(0, K, (B, T)).astype(np.int64)
    lengths = np.array([9, 4, 1], dtype=np.int64)
    xd = torch.from_numpy(x).to(dev).to(torch.bfloat16 if bf16 else torch.float32).requires_grad_(True)
    td, ld_ = torch.from_numpy(target).to(dev), torch.from_numpy(lengths).to(dev)
    loss, correct = unit_ce.masked_cross_entropy(xd, td, ld_, return_correct=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and correct.dtype == torch.int64 and not correct.requires_grad
    g, = torch.autograd.grad(loss * 0.75, (xd,))
    assert g.dtype == xd.dtype and g.shape == xd.shape
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    want = chain64(x64, torch.from_numpy(target), torch.from_numpy(lengths))
    g64, = torch.autograd.grad(want * 0.75, (x64,))
    ref = restated(x, target, lengths, K, 0.75)
    assert abs(float(want.detach()) - ref['loss']) <= 1e-12 and float((g64 - torch.from_numpy(ref['g'])).abs().max()) <= 1e-12
    assert abs(float(loss.detach()) - float(want.detach())) <= loss_bound(K, x, ref, lengths)
    assert int(correct) == ref['correct']
    slack = grad_bound(K, x, lengths, 0.75)[..., None] + (2.0 ** -8 * np.abs(ref['g']) if bf16 else 0.0)
    assert (np.abs(g.float().cpu().numpy() - ref['g']) <= slack).all()
    assert torch.equal(unit_ce.unit_argmax(xd, ld_).cpu(), torch.from_numpy(ref['pred']))
    assert unit_ce.masked_cross_entropy(xd, td, ld_).dim() == 0


# ---- (c) the 'softmax' method of the multi-stage quantiser ---------------------------------------------------------------------------------
def check_softmax_method(dev):
    from msmctts_amd.networks.vqgantts.msmc_vqgan import MultiStageQuantizer
    from msmctts_amd.hip import lib
    torch.manual_seed(7300)
    q = MultiStageQuantizer(32, [1, 1], embedding_sizes=24, embedding_dims=32, n_heads=1,
                            prior_config=dict(kernel_size=5, dilation_rate=1, n_layers=1)).to(dev)
    B, T, K = 3, 9, 24
    gen = torch.Generator().manual_seed(7301)
    lengths = torch.tensor([9, 4, 1], dtype=torch.int64).to(dev)
    states = []
    for shape in ((B, T), (B, T, 1)):
        states.append({'predictor_outputs': (torch.randn(B, T, K, generator=gen) * 2).to(dev).requires_grad_(True),
                       'target_outputs': None, 'target_indices': torch.randint(0, K, shape, generator=gen).to(dev),
                       'target_lengths': lengths})
    ps = [s['predictor_outputs'] for s in states]
    calls = []
    real = lib.get().msmc_unit_ce_fwd
    try:
        setattr(lib.get(), 'msmc_unit_ce_fwd', lambda *a: calls.append(1) or real(*a))
        fused = q.compute_embedding_loss(states, methods=['softmax'], loss_weights=[0.5])
        gf = torch.autograd.grad(fused['total_loss'], ps)
        assert len(calls) == 2
        q.fused_softmax = False
        stock = q.compute_embedding_loss(states, methods=['softmax'], loss_weights=[0.5])
        gs = torch.autograd.grad(stock['total_loss'], ps)
        assert len(calls) == 2, 'the guard set aside: the stock chain'
    finally:
        setattr(lib.get(), 'msmc_unit_ce_fwd', real)
    assert set(fused) == set(stock) == {'embed_loss_softmax_0', 'embed_loss_softmax_1', 'total_loss'}
    for i, s in enumerate(states):
        x = s['predictor_outputs'].detach().cpu().numpy()
        t = s['target_indices'].reshape(B, T).cpu().numpy()
        ref = restated(x, t, lengths.cpu().numpy(), K, 0.5)
        lb = loss_bound(K, x, ref, lengths.cpu().numpy())
        k = 'embed_loss_softmax_%d' % i
        assert abs(float(fused[k]) - ref['loss']) <= lb and abs(float(fused[k]) - float(stock[k])) <= lb + 16 * U * ref['loss'], k
        slack = grad_bound(K, x, lengths.cpu().numpy(), 0.5)[..., None]
        assert (np.abs(gf[i].cpu().numpy() - ref['g']) <= slack).all()
        assert float((gf[i] - gs[i]).abs().max()) <= 2 * slack.max() + 16 * U * np.abs(ref['g']).max()
    assert abs(float(fused['total_loss']) - 0.5 * (float(fused['embed_loss_softmax_0']) + float(fused['embed_loss_softmax_1']))) <= 1e-6
    # a host lengths tensor keeps the stock chain (the guard), as for 'mse'
    q.fused_softmax = True
    if dev != 'cpu':
        states[0]['target_lengths'] = lengths.cpu()
        try:
            setattr(lib.get(), 'msmc_unit_ce_fwd', lambda *a: calls.append(1) or real(*a))
            q.compute_embedding_loss(states[:1], methods=['softmax'], loss_weights=[1.0])
        finally:
            setattr(lib.get(), 'msmc_unit_ce_fwd', real)
        assert len(calls) == 2


# ---- (d) KMeansVQGANEmb -------------------------------------------------------------------------------------------------------------------
def _rel(got, want, what):
    err = abs(float(got) - float(want))
    print('%s: %.7g against %.7g' % (what, float(got), float(want)))
    assert err <= FP32_BAR * abs(float(want)), (what, float(got), float(want))


def check_kmeans_losses(dev, tmpdir):
    """every method of ``KMeansVQGANEmb.compute_embedding_loss`` against its float64 restatement, on a unit batch (-1 padding)"""
    import _unitembedcases as UE
    m, centers = UE.build_model(dev, tmpdir, False)
    K, D = UE.K_MODEL, UE.D
    B, T = 3, 9
    gen = torch.Generator().manual_seed(7400)
    lengths = torch.tensor([9, 4, 1], dtype=torch.int64)
    valid = torch.arange(T)[None, :] < lengths[:, None]
    ind = torch.where(valid, torch.randint(0, K, (B, T), generator=gen), torch.full((B, T), -1))
    logits = (torch.randn(B, T, ceil8(K), generator=gen) * 2).to(dev).requires_grad_(True)
    frames = torch.randn(B, T, D, generator=gen).to(dev).requires_grad_(True)
    states = {'quantizer_indices': (ind.to(dev),), 'quantizer_lengths': [lengths.to(dev)]}
    tot = float(lengths.sum())
    # softmax over the K centroids of logits built ceil8(K) wide
    out = m.compute_embedding_loss([logits], [lengths.to(dev)], states, methods=['softmax'], loss_weights=[2.0])
    assert set(out) == {'embed_loss_softmax_0', 'total_loss'}
    ref = restated(logits.detach().cpu().numpy(), ind.numpy(), lengths.numpy(), K, 2.0)
    assert abs(float(out['embed_loss_softmax_0']) - ref['loss']) <= loss_bound(K, logits.detach().cpu().numpy(), ref, lengths.numpy())
    _rel(out['total_loss'], 2.0 * ref['loss'], 'softmax total')
    assert int(states['unit_correct']) == ref['correct']
    g, = torch.autograd.grad(out['total_loss'], (logits,))
    assert not bool(g[:, :, K:].any()) and not bool(g[~valid].any())
    assert (np.abs(g.cpu().numpy() - ref['g']) <= grad_bound(K, logits.detach().cpu().numpy(), lengths.numpy(), 2.0)[..., None] + 4 * U * np.abs(ref['g'])).all()
    # mse against the centroid rows of the labels, and against given target frames
    c64 = torch.from_numpy(centers).double()
    p64 = frames.detach().double().cpu()
    rows = ((p64 - c64[ind.clamp(min=0)]) ** 2).mean(-1)
    out = m.compute_embedding_loss([frames], [lengths.to(dev)], states, methods=['mse'], loss_weights=[1.0])
    _rel(out['embed_loss_mse_0'], (rows * valid).sum() / tot, 'mse, centroid rows')
    given = torch.randn(B, T, D, generator=gen)
    out = m.compute_embedding_loss([frames], [lengths.to(dev)], dict(states, quantizer_outputs=(given.to(dev),)), methods=['mse'])
    _rel(out['embed_loss_mse_0'], ((((p64 - given.double()) ** 2).mean(-1)) * valid).sum() / tot, 'mse, given frames')
    # the triple losses (reference modules.py:86-116) and the weighting of several methods
    dist = ((p64[:, :, None, :] - c64[None, None]) ** 2).sum(-1)                       # [B, T, K]
    pos = ((p64 - c64[ind.clamp(min=0)]) ** 2).sum(-1, keepdim=True)
    tri = pos - dist
    tri = (tri != 0) * (torch.clamp(tri + 1e-6, min=0) / D)
    out = m.compute_embedding_loss([frames], [lengths.to(dev)], states, methods=['triple_sum', 'triple', 'mse'], loss_weights=[0.5, 2.0, 1.0])
    assert set(out) == {'embed_loss_triple_sum_0', 'embed_loss_triple_0', 'embed_loss_mse_0', 'total_loss'}
    _rel(out['embed_loss_triple_sum_0'], (tri.sum(-1) * valid).sum() / tot, 'triple_sum')
    _rel(out['embed_loss_triple_0'], (tri.mean(-1) * valid).sum() / tot, 'triple')
    _rel(out['total_loss'], 0.5 * float(out['embed_loss_triple_sum_0']) + 2.0 * float(out['embed_loss_triple_0']) + float(out['embed_loss_mse_0']), 'total')
    g, = torch.autograd.grad(out['total_loss'], (frames,))
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    with _raises(NotImplementedError, 'embedding loss'):
        m.compute_embedding_loss([frames], [lengths.to(dev)], states, methods=['cosine'])


def check_decode_units(dev, tmpdir):
    """one-hot rows of known labels come back as those labels; through ``collapse`` to the waveform of the labels"""
    import _unitembedcases as UE
    from msmctts_amd.hip import units as hipunits
    m, _ = UE.build_model(dev, tmpdir, True)
    m.eval()
    K = UE.K_MODEL
    B, T = 3, 24
    gen = torch.Generator().manual_seed(7500)
    labels = torch.repeat_interleave(torch.randint(0, K, (B, T), generator=gen), 3, dim=1)[:, :T].contiguous()
    length = torch.tensor([24, 17, 5], dtype=torch.int64)
    logits = torch.randn(B, T, ceil8(K), generator=gen)
    logits[:, :, K:] = 100.0                                                      # (not classes)
    logits.scatter_(2, labels.unsqueeze(-1), 30.0)
    valid = torch.arange(T)[None, :] < length[:, None]
    want = torch.where(valid, labels, torch.full_like(labels, -1))
    for lg in (logits, logits.to(torch.bfloat16)):
        got = m.decode_units(lg.to(dev), length.to(dev))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert torch.equal(m.decode_units(logits.to(dev), length.tolist()).cpu(), want)
    runs = m.decode_units(logits.to(dev), length.to(dev), collapse=True)
    for a, b in zip(runs, hipunits.collapse_units(want.to(dev), length.to(dev))):
        assert torch.equal(a, b)
    ref = torch.randn(B, 30, UE.MEL, generator=gen).to(dev)
    with torch.no_grad():
        a = m.synthesis_units(*runs, ref=ref)
        b = m.synthesis_units(want.to(dev), length.to(dev), ref=ref)
        assert a.dim() == 3 and a.shape[1] == T * 40 and torch.equal(a, b)
        assert torch.equal(m.synthesis_units(want.to(dev), length.to(dev), ref), b)      # (a third positional argument is still ref)


# ---- (e) trainer --------------------------------------------------------------------------------------------------------------------------
def predictor_width(K):
    """the width the predictor's head is built with: see ``check_head_width``"""
    return ceil8(K)


def build_trainer(dev, tmpdir, autoencoder=None, methods=None):
    import _unitembedcases as UE
    from _util import small_predictor_cfg
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer as make
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    pc = small_predictor_cfg()
    pc.update(n_pred_size=predictor_width(UE.K_MODEL), n_pred_scale=[1])
    trainer = dict(_name='UnitPredictorTrainer', grad_clip_thresh=10.0)
    if methods is not None:
        trainer.update(training_methods=methods, loss_weights=[1.0] * len(methods))
    cfg = Config({'id': 'small_unit_predictor', 'task': {'_name': 'MSMCTTS', '_mode': 'train_predictor', 'predictor': pc},
                  'trainer': trainer,
                  'optimizer': {'_default': dict(_name='Adam', learning_rate=2e-4, betas=[0.9, 0.98], eps=1e-9, weight_decay=0)},
                  'dataset': dict(samplerate=16000, feature=['units'], frameshift=[40])})
    torch.manual_seed(7600)
    task = build_task(cfg, mode='train').to(dev).train()
    tr = make(cfg, task, num_gpus=0, rank=0)
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True) if dev != 'cpu' else build_optimizer(task, cfg.optimizer)
    centers = None
    if autoencoder is None:
        autoencoder, centers = UE.build_model(dev, tmpdir, False)
    tr.autoencoder = autoencoder
    return task, tr, centers


def _batch(dev, centers=None):
    import _unitembedcases as UE
    from msmctts_amd import synthetic
    return synthetic.make_text_unit_batch(batch_size=3, frames=24, n_units=UE.K_MODEL, n_symbols=(20, 5, 2), phonemes=(4, 8),
                                          centers=centers, seed=7601, device=dev)


def check_text_unit_batch():
    """CPU, no kernels"""
    b = _batch('cpu')
    assert set(b) == {'text', 'text_length', 'dur', 'units', 'units_length'}
    assert b['units'].dtype == torch.int64 and tuple(b['units'].shape) == (3, 24) and int(b['units_length'].max()) == 24
    valid = torch.arange(24)[None, :] < b['units_length'][:, None]
    assert bool((b['units'][~valid] == -1).all()) and int(b['units'][valid].min()) >= 0 and int(b['units'][valid].max()) < 20
    assert torch.equal(b['dur'].sum(-1), b['units_length']) and tuple(b['text'].shape[::2]) == (3, 3)
    centers = np.random.default_rng(1).standard_normal((20, 6)).astype(np.float32)
    e = _batch('cpu', centers)
    assert set(e) == {'text', 'text_length', 'dur', 'emb', 'emb_length'} and torch.equal(e['emb_length'], b['units_length'])
    assert torch.equal(e['text'], b['text']) and torch.equal(e['dur'], b['dur'])
    assert torch.equal(e['emb'][valid], torch.from_numpy(centers)[b['units'][valid]]) and not bool(e['emb'][~valid].any())


def check_trainer_step(dev, tmpdir):
    """one step on a unit batch: finite losses, the predictor moves; the emb batch of the same labels' centroid frames gives the
    same loss bits"""
    import _unitembedcases as UE
    task, tr, centers = build_trainer(dev, tmpdir)
    assert type(tr).__name__ == 'UnitPredictorTrainer' and tr.training_methods == ['softmax']
    before = {k: v.detach().clone() for k, v in task.state_dict().items()}
    frozen = {k: v.detach().clone() for k, v in tr.autoencoder.state_dict().items()}
    log = tr.train_step(_batch(dev), 0)['loss']
    assert {'embed_loss_softmax_0', 'dur_loss', 'unit_acc', 'grad_norm', 'total_loss'} <= set(log), sorted(log)
    for k in ('embed_loss_softmax_0', 'dur_loss', 'unit_acc', 'grad_norm', 'total_loss'):
        assert torch.is_tensor(log[k]) and np.isfinite(float(log[k])), (k, log[k])
    assert 0.0 <= float(log['unit_acc']) <= 1.0
    # an untrained head: close to log K (the logits are small)
    assert abs(float(log['embed_loss_softmax_0']) - math.log(UE.K_MODEL)) < 1.0, float(log['embed_loss_softmax_0'])
    after = task.state_dict()
    moved = {k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k])}
    assert any(k.startswith('predictor.decoders.0.2.') for k in moved) and any(k.startswith('predictor.word_emb') for k in moved), sorted(moved)[:8]
    assert all(torch.equal(v, tr.autoencoder.state_dict()[k]) for k, v in frozen.items()), 'the autoencoder is frozen'
    # the same labels as frames: a fresh trainer (same seed), the emb batch
    task2, tr2, _ = build_trainer(dev, tmpdir)
    log2 = tr2.train_step(_batch(dev, centers), 0)['loss']
    for k in ('embed_loss_softmax_0', 'unit_acc', 'total_loss', 'dur_loss'):
        assert same_bits(log[k].cpu().numpy(), log2[k].cpu().numpy()), (k, float(log[k]), float(log2[k]))


def check_trainer_refusals(dev, tmpdir):
    import _embcases as E
    _, emb_task = E.build(dev, False)
    task, tr, _ = build_trainer(dev, tmpdir, autoencoder=emb_task.autoencoder)
    with _raises(TypeError, 'frozen codebook'):
        tr.train_step(_batch(dev), 0)
    assert tr.use_graphs is False
    tr.use_graphs = False
    with _raises(NotImplementedError, 'hipGraph'):
        tr.use_graphs = True
    task, tr, _ = build_trainer(dev, tmpdir)
    b = _batch(dev)
    del b['units']
    with _raises(KeyError, 'units'):
        tr.train_step(b, 0)


def check_head_width(dev):
    """What the convolution kernels make of a head that is no multiple of 8 wide (K = 100, 500 are real unit sizes): the
    predictor's output projection runs as a kernel-size-1 ConvLayer.  It takes both: a head may be exactly K wide, and one built
    ceil8(K) wide works as well (``classes=K``).  Asserted here so that a change shows."""
    from _util import small_predictor_cfg
    from msmctts_amd.networks import find_modules
    from msmctts_amd import synthetic
    b = synthetic.make_text_unit_batch(batch_size=2, frames=12, n_units=20, n_symbols=(20, 5, 2), phonemes=(3, 5), seed=7700, device=dev)
    widths = {}
    for width in (20, 24):
        pc = small_predictor_cfg()
        pc.update(n_pred_size=width, n_pred_scale=[1])
        torch.manual_seed(7701)
        (_, p), = find_modules({'predictor': pc})
        p = p.to(dev).train()
        try:
            out = p(text=b['text'], text_length=b['text_length'], dur=b['dur'], feat_length=[b['units_length']])['feat'][0]
            widths[width] = tuple(out.shape)
        except (RuntimeError, NotImplementedError, ValueError, AssertionError) as e:
            widths[width] = '%s: %s' % (type(e).__name__, str(e)[:120])
    print('head widths:', widths)
    assert widths == {20: (2, 12, 20), 24: (2, 12, 24)}, widths
    return widths


# ---- (f) feature presence -----------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'msmc_hip.h')) as f:
        header = f.read()
    for name in ('msmc_unit_ce_workspace', 'msmc_unit_ce_fwd', 'msmc_unit_ce_bwd', 'msmc_unit_argmax'):
        assert name + '(' in header, name
        assert name in lib.exported_symbols()
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
    assert os.path.isfile(os.path.join(root, 'msmc-tts_amd', 'csrc', 'unit_ce.hip'))
    from msmctts_amd.hip.unit_ce import masked_cross_entropy, unit_argmax  # noqa: F401
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansVQGANEmb
    from msmctts_amd.synthetic import make_text_unit_batch  # noqa: F401
    assert all(callable(getattr(KMeansVQGANEmb, name)) for name in ('compute_embedding_loss', 'decode_units'))
    from msmctts_amd.trainers import unit_predictor_trainer
    from msmctts_amd.trainers.msmctts_trainer import PredictorTrainer
    from msmctts_amd.utils.utils import module_search
    cls = module_search('UnitPredictorTrainer', os.path.dirname(unit_predictor_trainer.__file__), 'msmctts_amd.trainers')
    assert cls is unit_predictor_trainer.UnitPredictorTrainer and issubclass(cls, PredictorTrainer)
    assert os.path.isfile(os.path.join(root, 'tools', 'bench_unit_ce.py'))
