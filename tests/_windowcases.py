"""Shared cases of the window-gather kernel pair (csrc/window.hip, msmc_window_gather_fwd / _bwd, hip/window.py):
tests/test_window_emu.py runs them on the kernel interpreter, tests/test_gpu_window.py on the GPU.

Reference of every comparison: the stock chain the kernels replace -- ``torch.stack`` of zero-padded slices, ``.to(out_dtype)``
-- and its autograd gradient, evaluated on the CPU from the same input bits.  The comparison is BIT-EXACT: both sides only copy
and round once (bf16 -> fp32 is exact, fp32 -> bf16 rounds to nearest even on both sides), and a gradient element receives at
most one contribution (utterances are named once), so no sum is reordered.  Signed zeros compare equal.
"""
import ctypes

import torch

E_SHAPE = -2

# B, T, C, W, windows (utterance, first row)
CASES = (
    (1, 1, 8, 1, [(0, 0)]),                          # smallest shape
    (3, 37, 8, 5, [(0, 0), (2, 32)]),                # a subset of utterances; a window ending exactly at T
    (4, 40, 256, 8, [(0, 3), (1, 32), (3, 0)]),      # wide C
    (2, 9, 80, 4, [(1, 7)]),                         # two rows past T: zeros out, their gradient dropped
    (2, 13, 3, 4, [(0, 9), (1, 0)]),                 # scalar path
    (2, 50, 1, 20, [(0, 30), (1, 5)]),               # waveform shape
)
IDS = ['%dx%dx%d W%d' % c[:4] for c in CASES]
DTYPES = ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16))
DTYPE_IDS = ['fp32-fp32', 'fp32-bf16', 'bf16-bf16']
_DT = {torch.float32: 0, torch.bfloat16: 1}


def inputs(n, x_dtype, out_dtype):
    B, T, C, W, wins = CASES[n]
    gen = torch.Generator().manual_seed(900 + n)
    x = torch.randn(B, T, C, generator=gen).to(x_dtype)
    go = torch.randn(len(wins), W, C, generator=gen).to(out_dtype)
    return x, go


def chain(x, wins, W, out_dtype, go):
    """the stock chain and its autograd gradient on the CPU -> (out [n, W, C] in out_dtype, x.grad in x's dtype)"""
    x = x.clone().requires_grad_(True)
    T = x.shape[1]
    rows = []
    for u, s in wins:
        piece = x[u, s:min(s + W, T)]
        rows.append(torch.nn.functional.pad(piece, (0, 0, 0, W - piece.shape[0])))
    out = torch.stack(rows, dim=0).to(out_dtype)
    out.backward(go)
    return out.detach(), x.grad


def same_bits(a, b):
    """bit-equal up to the sign of zero (x + 0 of the stock gradient accumulation turns -0 into +0)"""
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.cpu() == b.cpu()).all())


def check_forward_backward(dev, n, pair):
    from msmctts_amd.hip import window
    B, T, C, W, wins = CASES[n]
    x_dtype, out_dtype = DTYPES[pair]
    x, go = inputs(n, x_dtype, out_dtype)
    want, want_gx = chain(x, wins, W, out_dtype, go)
    xd = x.clone().to(dev).requires_grad_(True)
    out = window.window_gather(xd, wins, W, out_dtype)
    assert out.dtype == out_dtype and tuple(out.shape) == (len(wins), W, C)
    assert torch.equal(out.detach().cpu(), want), 'forward differs from stack + cast'
    out.backward(go.to(dev))
    assert xd.grad.dtype == x_dtype and same_bits(xd.grad, want_gx), 'gradient differs from the chain autograd'
    # two identical calls; the table as a device tensor
    again = window.window_gather(xd.detach(), wins, W, out_dtype)
    table = torch.tensor(wins, dtype=torch.int32).to(dev)
    tensor_form = window.window_gather(xd.detach().requires_grad_(True), table, W, out_dtype)
    assert torch.equal(out.detach().view(torch.uint8), again.view(torch.uint8)), 'a repeated call changed bits'
    assert torch.equal(out.detach().view(torch.uint8), tensor_form.detach().view(torch.uint8)), 'list and tensor forms differ'
    g1 = tensor_form.grad_fn.apply(go.to(dev))[0]
    g2 = tensor_form.grad_fn.apply(go.to(dev))[0]
    assert torch.equal(g1.view(torch.uint8), g2.view(torch.uint8)) and torch.equal(g1.view(torch.uint8), xd.grad.view(torch.uint8))


def check_backward_writes_every_element(dev, n, pair):
    """the C entry directly, gx pre-filled with NaN: no NaN remains, rows outside every window are exactly 0, rows inside a window
    equal the reference"""
    from msmctts_amd.hip import lib
    B, T, C, W, wins = CASES[n]
    x_dtype, out_dtype = DTYPES[pair]
    x, go = inputs(n, x_dtype, out_dtype)
    _, want_gx = chain(x, wins, W, out_dtype, go)
    g = go.to(dev)
    table = torch.tensor(wins, dtype=torch.int32).to(dev)
    gx = torch.full((B, T, C), float('nan'), dtype=x_dtype).to(dev)
    rc = lib.get().msmc_window_gather_bwd(lib.ptr(g), _DT[out_dtype], lib.ptr(table), lib.ptr(gx), _DT[x_dtype], B, T, C, len(wins), W,
                                          lib.stream(g))
    assert rc == 0, rc
    gx = gx.cpu()
    assert not bool(torch.isnan(gx).any()), 'an element of gx was not written'
    covered = torch.zeros(B, T, dtype=torch.bool)
    for u, s in wins:
        covered[u, s:min(s + W, T)] = True
    assert bool((gx[~covered] == 0).all()), 'a row outside every window is not zero'
    assert torch.equal(gx[covered], want_gx[covered]), 'a row inside a window differs from the reference'


def check_hostile_tables(dev):
    """the table is device data: utterances outside [0, B), starts far outside [0, T) and a repeated utterance read and write
    nothing outside the buffers (guard rows around every buffer stay untouched); out-of-range entries give zeros"""
    from msmctts_amd.hip import lib
    B, T, C, W = 3, 11, 8, 4
    wins = [(-1, 0), (1, -2), (7, 3)]
    big = [(0, 2 ** 31 - 2), (1, -2 ** 31), (1, 9)]                # int32 extremes; utterance 1 twice
    gen = torch.Generator().manual_seed(950)
    for table_rows in (wins, big):
        n = len(table_rows)
        table = torch.tensor(table_rows, dtype=torch.int32).to(dev)
        xg = torch.randn(B + 2, T, C, generator=gen)                # one guard utterance on each side
        x_all = xg.to(dev)
        x = x_all[1:B + 1]
        out_all = torch.full((n + 2, W, C), 7.0).to(dev)
        out = out_all[1:n + 1]
        rc = lib.get().msmc_window_gather_fwd(lib.ptr(x), 0, lib.ptr(table), lib.ptr(out), 0, B, T, C, n, W, lib.stream(x))
        assert rc == 0, rc
        got = out_all.cpu()
        assert bool((got[0] == 7).all()) and bool((got[-1] == 7).all()), 'forward wrote outside out'
        for j, (u, s) in enumerate(table_rows):
            for t in range(W):
                ok = 0 <= u < B and 0 <= s + t < T
                want = xg[1 + u, s + t] if ok else torch.zeros(C)
                assert torch.equal(got[1 + j, t], want), (table_rows, j, t)
        go = torch.randn(n, W, C, generator=gen)
        gx_all = torch.full((B + 2, T, C), 7.0).to(dev)
        gx = gx_all[1:B + 1]
        g = go.to(dev)
        rc = lib.get().msmc_window_gather_bwd(lib.ptr(g), 0, lib.ptr(table), lib.ptr(gx), 0, B, T, C, n, W, lib.stream(g))
        assert rc == 0, rc
        got = gx_all.cpu()
        assert bool((got[0] == 7).all()) and bool((got[-1] == 7).all()), 'backward wrote outside gx'
        assert not bool((got[1:B + 1] == 7).any()), 'an element of gx was not written'
        allowed = torch.cat((go.reshape(-1), torch.zeros(1)))
        assert bool(torch.isin(got[1:B + 1].reshape(-1), allowed).all()), 'gx holds a value that is neither a gradient nor zero'
    # the wrapper and the table (1, -2): rows -2, -1 are zeros, rows 0, 1 are data
    from msmctts_amd.hip import window
    x = torch.randn(B, T, C, generator=gen)
    out = window.window_gather(x.to(dev), [(1, -2)], W).cpu()
    assert bool((out[0, :2] == 0).all()) and torch.equal(out[0, 2:], x[1, :2])


class _raises(object):
    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc) and self.text in str(val), (tp, val)
        return True


def check_rejected_arguments(dev):
    """W < 1, n < 1, n > B, C < 1, T < 1 return the shape error and launch nothing (the NaN-filled outputs stay NaN); the wrapper
    raises; a Python list that is not strictly increasing raises ValueError"""
    from msmctts_amd.hip import lib, window
    B, T, C, W, n = 2, 9, 8, 4, 2
    x = torch.randn(B, T, C).to(dev)
    table = torch.tensor([(0, 0), (1, 2), (1, 3)], dtype=torch.int32).to(dev)
    out = torch.full((3, W, C), float('nan')).to(dev)
    gx = torch.full((B, T, C), float('nan')).to(dev)
    L = lib.get()
    for b_, t_, c_, n_, w_ in ((B, T, C, n, 0), (B, T, C, n, -3), (B, T, C, 0, W), (B, T, C, 3, W), (B, T, 0, n, W), (B, 0, C, n, W),
                               (B, T, -8, n, W)):
        rc = L.msmc_window_gather_fwd(lib.ptr(x), 0, lib.ptr(table), lib.ptr(out), 0, b_, t_, c_, n_, w_, lib.stream(x))
        assert rc == E_SHAPE, (rc, b_, t_, c_, n_, w_)
        rc = L.msmc_window_gather_bwd(lib.ptr(out), 0, lib.ptr(table), lib.ptr(gx), 0, b_, t_, c_, n_, w_, lib.stream(x))
        assert rc == E_SHAPE, (rc, b_, t_, c_, n_, w_)
    assert bool(torch.isnan(out.cpu()).all()) and bool(torch.isnan(gx.cpu()).all()), 'a rejected call launched'
    with _raises(RuntimeError, 'msmc_window_gather_fwd failed with code -2'):
        window.window_gather(x, [(0, 0)], 0)
    with _raises(RuntimeError, 'msmc_window_gather_fwd failed with code -2'):
        window.window_gather(x, table, W)                                     # n = 3 > B = 2
    o = window.window_gather(x.clone().requires_grad_(True), [(0, 0), (1, 2)], W)
    o.grad_fn.args = (B, T, C, 0, torch.float32)
    with _raises(RuntimeError, 'msmc_window_gather_bwd failed with code -2'):
        o.grad_fn.apply(torch.zeros(2, W, C).to(dev))
    for bad in ([(1, 0), (0, 0)], [(0, 0), (0, 3)]):
        with _raises(ValueError, 'strictly increasing'):
            window.window_gather(x, bad, W)
    with _raises(TypeError, 'int32 [n, 2]'):
        window.window_gather(x, torch.zeros(2, 2, dtype=torch.int64).to(dev), W)


def check_feature_present():
    from msmctts_amd.hip import lib
    assert {'msmc_window_gather_fwd', 'msmc_window_gather_bwd'} <= set(lib.exported_symbols())
    for name in ('msmc_window_gather_fwd', 'msmc_window_gather_bwd'):
        assert isinstance(getattr(lib.get(), name), ctypes._CFuncPtr)
