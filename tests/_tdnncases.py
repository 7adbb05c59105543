"""Shared cases of the speaker reference encoder's kernels (csrc/tdnn.hip msmc_relu_bn_* / msmc_se_* / msmc_asp_*):
tests/test_tdnn_emu.py runs them on the kernel interpreter, tests/test_gpu_tdnn.py on the GPU.

Reference of every comparison: the operator's formulas in fp64 (numpy) from the same input bits.

Bounds (the rule of tests/_bncases.py).  E(q) for a quantity q = 4 x the max abs error of torch's own fp32 CPU operator chain
(and its autograd backward) against fp64 on the same case, with a floor of 4 fp32 ulps of the largest |q| -- the margin is for
another order of the sums.  bf16 activations (the fp64 reference from the bf16-rounded inputs): 2^-8 |q64| + E(q).  Saved
statistics and running buffers of the BatchNorm are held to what E(y) means for them, as in _bncases.py, with |gamma| divided out.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1
E_SHAPE = -2
MEASURED = []          # (case, quantity, kernel error, bound): printed by the tests, recorded in profiles/ecapa.md

RBN_SHAPES = [(2, 8), (33, 64), (4097, 256), (257, 1024)]
RBN_SLICE = (150, 32, 256, 64)          # N rows, C channels at offset 64 of a 256-wide row
SE_SHAPES = [(1, 1, 8), (2, 37, 64), (3, 1025, 256)]
# (B, T, C) -> seed for which every fp64 residual is exactly 0 or >= 1e-4, for the fp32 and the bf16-rounded inputs alike
ASP_CASES = {(1, 1, 8): 0, (2, 37, 64): 0, (3, 130, 192): 0, (2, 1025, 768): 0, (1, 33, 1536): 0}


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def f64(t):
    return t.detach().double().cpu().numpy()


def _name(dtype):
    return 'bf16' if dtype == torch.bfloat16 else 'fp32'


def _bound(torch_val, ref):
    """E(q): 4 x torch's fp32 error, floor 4 ulps of the largest magnitude"""
    return max(4 * float(np.abs(f64(torch_val) - ref).max()), 4 * ulp32(np.abs(ref).max()))


def within(case, name, got, want, tol, rel8=False):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(f64(got).reshape(want.shape) - want)
    tol = tol + (2.0 ** -8 * np.abs(want) if rel8 else 0.0)
    worst = int(np.argmax(err - tol))
    e, b = float(err.reshape(-1)[worst]), float(np.broadcast_to(tol, err.shape).reshape(-1)[worst])
    MEASURED.append((case, name, e, b))
    print('tdnn %-38s %-6s err %.3e  bound %.3e' % (case, name, e, b))
    assert (err <= tol).all(), '%s %s: err %.3e > bound %.3e' % (case, name, e, b)


# ---- ReLU + affine BatchNorm -------------------------------------------------------------------------------------------------
def rbn_inputs(N, C, dtype, seed, wide=None, offset=0):
    rng = np.random.default_rng(seed)
    W = C if wide is None else wide
    xw = rng.standard_normal((N, W)) * rng.uniform(0.5, 2.0, W) + rng.uniform(-1.0, 1.0, W)
    xw[:, offset + 3] = -np.abs(xw[:, offset + 3]) - 0.1            # one channel all negative: relu == 0, variance 0
    xw = torch.from_numpy(xw).to(dtype)
    g = torch.from_numpy(rng.standard_normal((N, C))).to(dtype)
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, C)).float()
    beta = torch.from_numpy(0.3 * rng.standard_normal(C)).float()
    rm = torch.from_numpy(0.1 * rng.standard_normal(C)).float()
    rv = torch.from_numpy(rng.uniform(0.5, 1.5, C)).float()
    return xw, g, gamma, beta, rm, rv


def rbn_reference64(x, g, gamma, beta, rm, rv, training):
    x, g, gamma, beta, rm, rv = (f64(t) for t in (x, g, gamma, beta, rm, rv))
    N = x.shape[0]
    r = np.maximum(x, 0.0)
    if training:
        mean, var = r.mean(0), r.var(0)
        unb = var * N / (N - 1)
        for _ in range(2):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
            rv = (1 - MOMENTUM) * rv + MOMENTUM * unb
    else:
        mean, var, unb = rm, rv, rv
    rstd = 1.0 / np.sqrt(var + EPS)
    xh = (r - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    inner = (g - dbeta / N - xh * dgamma / N) if training else g
    return dict(y=gamma * xh + beta, gx=(x > 0) * gamma * rstd * inner, dgamma=dgamma, dbeta=dbeta, mean=mean, rstd=rstd,
                rm=rm, rv=rv, unb=unb, xh=xh)


def rbn_torch32(x, g, gamma, beta, rm, rv, training):
    xf = x.float().clone().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.batch_norm(F.relu(xf), rm.clone(), rv.clone(), ga, be, training, MOMENTUM, EPS)
    y.backward(g.float())
    return dict(y=y, gx=xf.grad, dgamma=ga.grad, dbeta=be.grad)


def rbn_module(C, gamma, beta, rm, rv, dev, training):
    bn = nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    return bn.train(training)


def check_relu_bn(dev, N, C, dtype, training, wide=None, offset=0):
    from msmctts_amd.hip import tdnn as hiptdnn
    xw, g, gamma, beta, rm, rv = rbn_inputs(N, C, dtype, seed=N * 7 + C, wide=wide, offset=offset)
    x = xw[:, offset:offset + C]
    ref = rbn_reference64(x, g, gamma, beta, rm, rv, training)
    t32 = rbn_torch32(x, g, gamma, beta, rm, rv, training)
    E = {k: _bound(t32[k], ref[k]) for k in t32}
    bn = rbn_module(C, gamma, beta, rm, rv, dev, training)
    xd, gd = xw.to(dev), g.to(dev)
    runs = []
    for _ in range(2):
        bn.zero_grad()
        xi = xd.clone().requires_grad_(True)
        xs = xi[:, offset:offset + C]
        assert hiptdnn.relu_batch_norm_usable(xs, bn) and (wide is None) == xs.is_contiguous()
        y = hiptdnn.relu_batch_norm(xs, bn)
        saved = y.grad_fn.saved_tensors
        y.backward(gd)
        runs.append((y.detach(), xi.grad[:, offset:offset + C], bn.weight.grad.clone(), bn.bias.grad.clone(), saved[2], saved[3]))
    (y, gx, dga, dbe, mean, rstd), second = runs
    assert y.dtype == dtype and gx.dtype == dtype and y.is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(runs[0][:4], second[:4]))                 # same input, same bits
    if wide is not None:                                   # nothing outside the slice receives gradient
        assert float(xi.grad[:, :offset].abs().max()) == 0.0 and float(xi.grad[:, offset + C:].abs().max()) == 0.0
    case = 'relu_bn %dx%d%s %s %s' % (N, C, '' if wide is None else '/%d' % wide, _name(dtype), 'train' if training else 'eval')
    b16 = dtype == torch.bfloat16
    within(case, 'y', y, ref['y'], E['y'], b16)
    within(case, 'gx', gx, ref['gx'], E['gx'], b16)
    within(case, 'dgamma', dga, ref['dgamma'], E['dgamma'])
    within(case, 'dbeta', dbe, ref['dbeta'], E['dbeta'])
    assert not training or float(y[:, 3].float().sub(beta[3].to(dev)).abs().max()) <= (2.0 ** -8 * abs(float(beta[3])) if b16 else 0.0)
    assert float(gx[:, 3].abs().max()) == 0.0              # the all-negative channel: y == beta in training, no gradient
    ga = np.abs(f64(gamma))
    ey = E['y'] / ga                                       # what E(y) means for xhat
    xmax = max(np.abs(ref['xh']).max(), 1.0)
    within(case, 'rstd', rstd, ref['rstd'], ey * ref['rstd'] / xmax)
    if training:
        within(case, 'mean', mean, ref['mean'], ey / ref['rstd'])
        within(case, 'rmean', bn.running_mean, ref['rm'], ey / ref['rstd'] + 4 * ulp32(np.abs(ref['rm']).max()))
        within(case, 'rvar', bn.running_var, ref['rv'], 2 * ey / xmax * ref['unb'] + 4 * ulp32(np.abs(ref['rv']).max()))
        assert int(bn.num_batches_tracked) == 2
    else:
        assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv)
        assert int(bn.num_batches_tracked) == 0


def check_relu_bn_refusals(dev):
    from msmctts_amd.hip import lib, tdnn as hiptdnn
    L = lib.get()

    def fwd(N, C, ld=None):
        ld = C if ld is None else ld
        x = torch.zeros(max(N, 1), ld, device=dev)
        y, v = torch.empty_like(x), [torch.ones(max(C, 8), device=dev) for _ in range(6)]
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        ws = torch.empty(1 << 16, device=dev)
        rc = L.msmc_relu_bn_fwd(lib.ptr(x), ld, lib.ptr(v[0]), lib.ptr(v[1]), lib.ptr(y), ld, lib.ptr(v[2]), lib.ptr(v[3]),
                                lib.ptr(v[4]), lib.ptr(v[5]), lib.ptr(nbt), lib.ptr(ws), ws.numel() * 4, N, C, EPS, MOMENTUM, 0,
                                lib.stream(x))
        if dev != 'cpu':
            torch.cuda.synchronize()
        assert int(nbt) == (1 if rc == 0 else 0)
        return rc
    assert fwd(16, 12) == E_SHAPE and fwd(16, 2048) == E_SHAPE and fwd(1, 64) == E_SHAPE and fwd(16, 64, ld=68) == E_SHAPE
    assert fwd(16, 64) == 0 and fwd(16, 64, ld=72) == 0
    assert L.msmc_relu_bn_workspace(16, 12) == 0 and L.msmc_relu_bn_workspace(16, 64) > 0
    bn = nn.BatchNorm1d(64).to(dev).train()
    with _raises(ValueError, 'more than 1 value per channel'):
        hiptdnn.relu_batch_norm(torch.zeros(1, 1, 64, device=dev), bn)
    assert int(bn.num_batches_tracked) == 0
    x = torch.zeros(1, 4, 64, device=dev)
    assert hiptdnn.relu_batch_norm_usable(x, bn)
    assert not hiptdnn.relu_batch_norm_usable(x, nn.BatchNorm1d(64, affine=False).to(dev))
    assert not hiptdnn.relu_batch_norm_usable(x, nn.BatchNorm1d(64, momentum=None).to(dev))
    assert not hiptdnn.relu_batch_norm_usable(x.double(), bn)
    with _raises(RuntimeError, 'msmc_relu_bn'):
        hiptdnn.relu_batch_norm(torch.zeros(1, 4, 12, device=dev), nn.BatchNorm1d(12).to(dev))


class _raises(object):
    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc) and self.text in str(val), (tp, val)
        return True


# ---- squeeze-excitation + residual ------------------------------------------------------------------------------------------------
def se_inputs(B, T, C, dtype, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, T, C)) + rng.uniform(-0.5, 0.5, C)).to(dtype)
    res = torch.from_numpy(rng.standard_normal((B, T, C))).to(dtype)
    g = torch.from_numpy(rng.standard_normal((B, T, C))).to(dtype)
    H = C // 2
    W1 = torch.from_numpy(rng.standard_normal((H, C)) / np.sqrt(C)).float()
    W2 = torch.from_numpy(rng.standard_normal((C, H)) / np.sqrt(H)).float()
    b1 = torch.from_numpy(0.3 * rng.standard_normal(H)).float()
    b2 = torch.from_numpy(0.3 * rng.standard_normal(C)).float()
    return x, res, g, W1, b1, W2, b2


def se_reference64(x, res, g, W1, b1, W2, b2):
    x, res, g, W1, b1, W2, b2 = (f64(t) for t in (x, res, g, W1, b1, W2, b2))
    T = x.shape[1]
    s = x.mean(1)
    h = np.maximum(s @ W1.T + b1, 0.0)
    gate = 1.0 / (1.0 + np.exp(-(h @ W2.T + b2)))
    dgate = (g * x).sum(1)
    dz2 = dgate * gate * (1 - gate)
    dz1 = (dz2 @ W2) * (h > 0)
    return dict(y=res + x * gate[:, None, :], gx=g * gate[:, None, :] + (dz1 @ W1)[:, None, :] / T, gres=g,
                dW1=dz1.T @ s, db1=dz1.sum(0), dW2=dz2.T @ h, db2=dz2.sum(0))


def se_torch32(x, res, g, W1, b1, W2, b2):
    xf, rf = x.float().clone().requires_grad_(True), res.float().clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in (W1, b1, W2, b2)]
    gate = torch.sigmoid(F.linear(F.relu(F.linear(xf.mean(1), ps[0], ps[1])), ps[2], ps[3]))
    y = rf + xf * gate.unsqueeze(1)
    y.backward(g.float())
    return dict(y=y, gx=xf.grad, gres=rf.grad, dW1=ps[0].grad, db1=ps[1].grad, dW2=ps[2].grad, db2=ps[3].grad)


def se_layers(C, W1, b1, W2, b2, dev):
    l1, l2 = nn.Linear(C, C // 2).to(dev), nn.Linear(C // 2, C).to(dev)
    with torch.no_grad():
        for p, v in ((l1.weight, W1), (l1.bias, b1), (l2.weight, W2), (l2.bias, b2)):
            p.copy_(v)
    return l1, l2


def check_se(dev, B, T, C, dtype):
    from msmctts_amd.hip import tdnn as hiptdnn
    inp = se_inputs(B, T, C, dtype, seed=B * 1000 + T * 3 + C)
    ref, t32 = se_reference64(*inp), se_torch32(*inp)
    E = {k: _bound(t32[k], ref[k]) for k in t32}
    x, res, g = (t.to(dev) for t in inp[:3])
    l1, l2 = se_layers(C, *inp[3:], dev)
    runs = []
    for _ in range(2):
        l1.zero_grad()
        l2.zero_grad()
        xi, ri = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
        assert hiptdnn.se_residual_usable(xi, l1, l2)
        y = hiptdnn.se_residual(xi, ri, l1, l2)
        y.backward(g)
        runs.append(dict(y=y.detach(), gx=xi.grad, gres=ri.grad, dW1=l1.weight.grad.clone(), db1=l1.bias.grad.clone(),
                         dW2=l2.weight.grad.clone(), db2=l2.bias.grad.clone()))
    a, b = runs
    assert all(torch.equal(a[k], b[k]) for k in a)                                         # same input, same bits
    assert a['y'].dtype == dtype and a['gx'].dtype == dtype and torch.equal(a['gres'], g)
    case = 'se %dx%dx%d %s' % (B, T, C, _name(dtype))
    for k in ('y', 'gx', 'dW1', 'db1', 'dW2', 'db2'):
        within(case, k, a[k], ref[k], E[k], dtype == torch.bfloat16 and k in ('y', 'gx'))


def check_se_refusals(dev):
    from msmctts_amd.hip import lib, tdnn as hiptdnn
    L = lib.get()

    def fwd(B, T, C):
        n = max(B * T * C, 8)
        x, v = torch.zeros(n, device=dev), torch.zeros(max(C * C, 64), device=dev)
        y, ws = torch.empty_like(x), torch.empty(1 << 16, device=dev)
        return L.msmc_se_fwd(lib.ptr(x), lib.ptr(x), lib.ptr(v), lib.ptr(v), lib.ptr(v), lib.ptr(v), lib.ptr(y),
                             lib.ptr(v), lib.ptr(v), lib.ptr(v), lib.ptr(ws), ws.numel() * 4, B, T, C, 0, lib.stream(x))
    assert fwd(1, 4, 12) == E_SHAPE and fwd(1, 1, 1032) == E_SHAPE and fwd(1, 0, 8) == E_SHAPE and fwd(1, 4, 16) == 0
    assert L.msmc_se_workspace(1, 4, 12) == 0 and L.msmc_se_workspace(1, 4, 16) > 0
    l1, l2 = nn.Linear(12, 6).to(dev), nn.Linear(6, 12).to(dev)
    x = torch.zeros(1, 4, 12, device=dev)
    assert not hiptdnn.se_residual_usable(x, l1, l2)
    with _raises(RuntimeError, 'msmc_se'):
        hiptdnn.se_residual(x, x, l1, l2)


# ---- attentive statistics pooling -------------------------------------------------------------------------------------------------
def asp_inputs(B, T, C, dtype, seed):
    """x post-ReLU-like; channels 1 and C - 2 all zero; channel 5 with logits of magnitude 80 (a naive exp overflows)"""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, T, C)), 0.0)
    x[:, :, 1] = 0.0
    x[:, :, C - 2] = 0.0
    a = rng.standard_normal((B, T, C))
    a[:, :, 5] = 80.0 + 4.0 * a[:, :, 5]
    g = rng.standard_normal((B, 2 * C))
    return torch.from_numpy(x).to(dtype), torch.from_numpy(a).to(dtype), torch.from_numpy(g).float()


def asp_reference64(x, a, g):
    x, a, g = f64(x), f64(a), f64(g)
    C = x.shape[2]
    e = np.exp(a - a.max(1, keepdims=True))
    al = e / e.sum(1, keepdims=True)
    mean, q = (al * x).sum(1), (al * x * x).sum(1)
    res = q - mean * mean
    std = np.sqrt(np.maximum(res, 1e-9))
    dres = np.where(res < 1e-9, 0.0, g[:, C:] / (2 * std))
    dmean = g[:, :C] - 2 * mean * dres
    dal = dmean[:, None, :] * x + dres[:, None, :] * x * x
    ga = al * (dal - (al * dal).sum(1, keepdims=True))
    gx = al * (dmean[:, None, :] + 2 * dres[:, None, :] * x)
    return dict(out=np.concatenate([mean, std], 1), gx=gx, ga=ga, res=res)


def asp_torch32(x, a, g):
    xf, af = x.float().clone().requires_grad_(True), a.float().clone().requires_grad_(True)
    al = torch.softmax(af, dim=1)
    mean = torch.sum(al * xf, dim=1)
    residuals = torch.sum(al * xf ** 2, dim=1) - mean ** 2
    out = torch.cat([mean, torch.sqrt(residuals.clamp(min=1e-9))], dim=1)
    out.backward(g)
    return dict(out=out, gx=xf.grad, ga=af.grad)


def asp_condition(ref, C):
    """no element at the clamp's kink: every fp64 residual exactly 0 (the planted channels; T == 1) or >= 1e-4"""
    res = ref['res']
    assert ((res == 0.0) | (res >= 1e-4)).all(), 'residual in (0, 1e-4): min positive %.3e' % res[res != 0].min()
    assert (res[:, 1] == 0.0).all() and (res[:, C - 2] == 0.0).all()


def check_asp(dev, B, T, C, dtype):
    from msmctts_amd.hip import tdnn as hiptdnn
    x, a, g = asp_inputs(B, T, C, dtype, ASP_CASES[(B, T, C)])
    ref, t32 = asp_reference64(x, a, g), asp_torch32(x, a, g)
    asp_condition(ref, C)
    E = {k: _bound(t32[k], ref[k]) for k in t32}
    runs = []
    for _ in range(2):
        xi, ai = x.to(dev).clone().requires_grad_(True), a.to(dev).clone().requires_grad_(True)
        assert hiptdnn.attentive_stats_pool_usable(xi, ai)
        out = hiptdnn.attentive_stats_pool(xi, ai)
        out.backward(g.to(dev))
        runs.append(dict(out=out.detach(), gx=xi.grad, ga=ai.grad))
    p, q = runs
    assert all(torch.equal(p[k], q[k]) for k in p)                                         # same input, same bits
    assert p['out'].dtype == torch.float32 and p['gx'].dtype == dtype and p['ga'].dtype == dtype
    assert bool(torch.isfinite(p['out']).all())
    case = 'asp %dx%dx%d %s' % (B, T, C, _name(dtype))
    for k in ('out', 'gx', 'ga'):
        within(case, k, p[k], ref[k], E[k], dtype == torch.bfloat16)


def check_asp_refusals(dev):
    from msmctts_amd.hip import lib, tdnn as hiptdnn
    L = lib.get()

    def fwd(B, T, C):
        x = torch.zeros(max(B * T * C, 8), device=dev)
        out, st, ws = torch.empty(max(2 * B * C, 8), device=dev), torch.empty(max(4 * B * C, 8), device=dev), torch.empty(1 << 16, device=dev)
        return L.msmc_asp_fwd(lib.ptr(x), lib.ptr(x), lib.ptr(out), lib.ptr(st), lib.ptr(ws), ws.numel() * 4, B, T, C, 0, lib.stream(x))
    assert fwd(1, 4, 12) == E_SHAPE and fwd(1, 1, 1544) == E_SHAPE and fwd(1, 0, 8) == E_SHAPE and fwd(1, 4, 16) == 0
    assert L.msmc_asp_workspace(1, 4, 12) == 0 and L.msmc_asp_workspace(1, 4, 16) > 0
    x = torch.zeros(1, 4, 12, device=dev)
    assert not hiptdnn.attentive_stats_pool_usable(x, x) and not hiptdnn.attentive_stats_pool_usable(x.double(), x.double())
    with _raises(RuntimeError, 'msmc_asp'):
        hiptdnn.attentive_stats_pool(x, x)
