"""Shared cases of the BatchNorm kernels (csrc/norm.hip msmc_bn_*): tests/test_bn_emu.py runs them on the kernel interpreter,
tests/test_gpu_bn.py on the GPU.

Reference of every comparison: the BatchNorm formulas in fp64 (numpy) from the same input bits.

Bounds.  E(q) for a quantity q (y or gx) = 4 x the max abs error of torch's own fp32 CPU operator (F.batch_norm and its autograd
backward) against fp64 on the same case, with a floor of 4 fp32 ulps of the largest |q| -- the margin is for another order of the
sums.  bf16 (bf16 in and out; the fp64 reference from the bf16-rounded input): 2^-8 |q64| + E(q), one bf16 rounding of the output
on top of the fp32 arithmetic.  The saved statistics and the running buffers are held to what E(y) means for them: an error dm
of a channel's mean moves y by dm * rstd, so |dm| <= E(y) / rstd; a relative error r of rstd moves y by r |y|, so
|d rstd| / rstd <= E(y) / max|y|; the variance carries twice the relative error of rstd, and a blended buffer adds its own final
rounding (4 ulps of its largest entry).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SHAPES = [(2, 8), (33, 64), (150, 256), (4097, 256), (257, 1024)]
EPS, MOMENTUM = 1e-5, 0.1
MEASURED = []          # (case, quantity, kernel error, bound): printed by the tests, recorded in profiles/quantiser_norm.md


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def make_inputs(N, C, dtype, g_dtype, seed, cancel=False):
    rng = np.random.default_rng(seed)
    if cancel:
        x = 100.0 + 0.1 * rng.standard_normal((N, C))
    else:
        x = rng.standard_normal((N, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1.0, 1.0, C)
    x = torch.from_numpy(x).to(dtype)
    g = torch.from_numpy(rng.standard_normal((N, C))).to(g_dtype)
    rm = torch.from_numpy(0.1 * rng.standard_normal(C)).float()
    rv = torch.from_numpy(rng.uniform(0.5, 1.5, C)).float()
    return x, g, rm, rv


def reference64(x, g, rm, rv, training):
    """fp64 formulas; two consecutive training calls for the running buffers"""
    x, g, rm, rv = (t.double().numpy() for t in (x, g, rm, rv))
    N = x.shape[0]
    if training:
        mean, var = x.mean(0), x.var(0)
        unb = var * N / (N - 1)
        for _ in range(2):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
            rv = (1 - MOMENTUM) * rv + MOMENTUM * unb
    else:
        mean, var, unb = rm, rv, rv
    rstd = 1.0 / np.sqrt(var + EPS)
    xh = (x - mean) * rstd
    gx = rstd * (g - g.mean(0) - xh * (g * xh).mean(0)) if training else g * rstd
    return dict(y=xh, gx=gx, mean=mean, rstd=rstd, rm=rm, rv=rv, unb=unb)


def torch_fp32_error(x, g, rm, rv, training, ref):
    """max abs error of torch's own fp32 operator on the CPU against fp64: (of y, of gx)"""
    xf = x.float().cpu().clone().requires_grad_(True)
    y = F.batch_norm(xf, rm.clone(), rv.clone(), None, None, training, MOMENTUM, EPS)
    y.backward(g.float().cpu())
    return (float(np.abs(y.detach().double().numpy() - ref['y']).max()),
            float(np.abs(xf.grad.double().numpy() - ref['gx']).max()))


def bounds(x, g, rm, rv, training, ref):
    ty, tg = torch_fp32_error(x, g, rm, rv, training, ref)
    ey = max(4 * ty, 4 * ulp32(np.abs(ref['y']).max()))
    eg = max(4 * tg, 4 * ulp32(np.abs(ref['gx']).max()))
    return ey, eg, ty, tg


def module(C, rm, rv, dev, training):
    bn = nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM, affine=False).to(dev)
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    return bn.train(training)


def run_kernels(x, g, bn, out_fp32, calls=2):
    """``calls`` consecutive forward + backward passes over the same input through the Python op: [(y, gx, mean, rstd)]"""
    from msmctts_amd.hip import norm as hipnorm
    out = []
    for _ in range(calls):
        xi = x.clone().unsqueeze(0).requires_grad_(True)
        y = hipnorm.batch_norm(xi, bn, out_fp32=out_fp32)
        saved = y.grad_fn.saved_tensors
        y.backward(g.unsqueeze(0))
        mean, rstd = (saved[1], saved[2]) if bn.training else (None, saved[0])
        out.append((y.detach()[0], xi.grad[0], mean, rstd))
    return out


def check_case(dev, N, C, dtype, out_fp32, training, cancel=False):
    g_dtype = torch.float32 if out_fp32 else dtype
    x, g, rm, rv = make_inputs(N, C, dtype, g_dtype, seed=N * 7 + C, cancel=cancel)
    ref = reference64(x, g, rm, rv, training)
    ey, eg, ty, tg = bounds(x, g, rm, rv, training, ref)
    bn = module(C, rm, rv, dev, training)
    from msmctts_amd.hip import norm as hipnorm
    assert hipnorm.batch_norm_usable(x.to(dev).unsqueeze(0), bn)
    runs = run_kernels(x.to(dev), g.to(dev), bn, out_fp32)
    (y, gx, mean, rstd), (y2, gx2, _, _) = runs
    assert y.dtype == (torch.float32 if out_fp32 else dtype) and gx.dtype == dtype
    assert torch.equal(y, y2) and torch.equal(gx, gx2)              # same input, same bits

    case = '%dx%d %s%s %s%s' % (N, C, 'bf16' if dtype == torch.bfloat16 else 'fp32', '->fp32' if out_fp32 and dtype != torch.float32 else '',
                                'train' if training else 'eval', ' cancel' if cancel else '')
    ymax = np.abs(ref['y']).max()

    def within(name, got, want, tol):
        err = np.abs(got.detach().double().cpu().numpy() - want)
        worst = int(np.argmax(err - tol)) if np.ndim(tol) else int(np.argmax(err))
        e, b = float(err.reshape(-1)[worst]), float(np.broadcast_to(tol, err.shape).reshape(-1)[worst])
        MEASURED.append((case, name, e, b))
        print('bn %-34s %-5s err %.3e  bound %.3e  (torch fp32: y %.3e gx %.3e)' % (case, name, e, b, ty, tg))
        assert (err <= tol).all(), '%s %s: err %.3e > bound %.3e' % (case, name, e, b)

    r8 = 2.0 ** -8
    within('y', y, ref['y'], (r8 * np.abs(ref['y']) if y.dtype == torch.bfloat16 else 0.0) + ey)
    within('gx', gx, ref['gx'], (r8 * np.abs(ref['gx']) if dtype == torch.bfloat16 else 0.0) + eg)
    within('rstd', rstd, ref['rstd'], ey * ref['rstd'] / ymax)
    if training:
        within('mean', mean, ref['mean'], ey / ref['rstd'])
        within('rmean', bn.running_mean, ref['rm'], ey / ref['rstd'] + 4 * ulp32(np.abs(ref['rm']).max()))
        within('rvar', bn.running_var, ref['rv'], 2 * ey / ymax * ref['unb'] + 4 * ulp32(np.abs(ref['rv']).max()))
        assert int(bn.num_batches_tracked) == 2
    else:
        assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv)
        assert int(bn.num_batches_tracked) == 0
    return bn, runs


def check_determinism(dev, N=4097, C=256, dtype=torch.float32):
    """two modules from the same buffers, two passes each: y, gx and the running buffers bit for bit"""
    x, g, rm, rv = make_inputs(N, C, dtype, dtype, seed=11)
    res = []
    for _ in range(2):
        bn = module(C, rm, rv, dev, True)
        runs = run_kernels(x.to(dev), g.to(dev), bn, False)
        res.append((runs, bn))
    (ra, ba), (rb, bb) = res
    for (ya, ga, ma, sa), (yb, gb, mb, sb) in zip(ra, rb):
        assert torch.equal(ya, yb) and torch.equal(ga, gb) and torch.equal(ma, mb) and torch.equal(sa, sb)
    assert torch.equal(ba.running_mean, bb.running_mean) and torch.equal(ba.running_var, bb.running_var)
    assert int(ba.num_batches_tracked) == int(bb.num_batches_tracked) == 2


def check_refusals(dev):
    from msmctts_amd.hip import lib, norm as hipnorm
    L = lib.get()
    E_SHAPE = -2

    def fwd(N, C):
        x = torch.zeros(max(N, 1), C, device=dev)
        y, mean, rstd = torch.empty_like(x), torch.empty(C, device=dev), torch.empty(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        ws = torch.empty(1 << 16, device=dev)
        rc = L.msmc_bn_fwd(lib.ptr(x), lib.ptr(y), lib.ptr(mean), lib.ptr(rstd), lib.ptr(rm), lib.ptr(rv), lib.ptr(nbt), lib.ptr(ws),
                           ws.numel() * 4, N, C, EPS, MOMENTUM, 0, 0, lib.stream(x))
        if dev != 'cpu':
            torch.cuda.synchronize()
        assert int(nbt) == 0
        return rc
    assert fwd(16, 12) == E_SHAPE and fwd(16, 2048) == E_SHAPE and fwd(1, 64) == E_SHAPE
    assert L.msmc_bn_workspace(16, 12) == 0 and L.msmc_bn_workspace(16, 64) > 0
    x = torch.zeros(4, 12, device=dev)
    rc = L.msmc_bn_eval_fwd(lib.ptr(x), lib.ptr(x), lib.ptr(x), lib.ptr(torch.empty_like(x)), None, 4, 12, EPS, 0, 0, lib.stream(x))
    assert rc == E_SHAPE
    bn = nn.BatchNorm1d(64, affine=False).to(dev).train()
    try:
        hipnorm.batch_norm(torch.zeros(1, 1, 64, device=dev), bn)
    except ValueError as e:
        assert 'more than 1 value per channel' in str(e)
    else:
        raise AssertionError('N = 1 in training must raise ValueError')
    assert int(bn.num_batches_tracked) == 0
    # what the predicate refuses: the module forms the kernels do not cover
    x = torch.zeros(1, 4, 64, device=dev)
    assert hipnorm.batch_norm_usable(x, bn)
    assert not hipnorm.batch_norm_usable(x, nn.BatchNorm1d(64, affine=True).to(dev))
    assert not hipnorm.batch_norm_usable(x, nn.BatchNorm1d(64, affine=False, momentum=None).to(dev))
    assert not hipnorm.batch_norm_usable(x, nn.BatchNorm1d(64, affine=False, track_running_stats=False).to(dev))
    assert not hipnorm.batch_norm_usable(x.double(), bn)
    assert not hipnorm.batch_norm_usable(torch.zeros(1, 4, 12, device=dev), nn.BatchNorm1d(12, affine=False).to(dev))
