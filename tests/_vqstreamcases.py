"""Shared cases of the streamed exact codeword search (csrc/vq_stream.inc, msmc_vq_search_stream, and msmc_vq_search where no
head's codebook fits LDS): tests/test_vq_stream_emu.py runs them on the kernel interpreter, tests/test_gpu_vq_stream.py on the GPU.

References:
* where a resident kernel takes the shape: msmc_vq_search itself, BIT-EXACT (same distance expression, same fp32 summation
  order, same tie rule -- the chunking must not show);
* where only the streamed kernel takes the shape: the same distance ``(|x|^2 - 2 x.e_k) + |e_k|^2`` in float64.  The fp32 chain
  rounds once per product-sum step: d steps of relative 2^-24 on partial sums bounded by |x||e| for the dot product (doubled),
  the same for the two norms, three more roundings to combine -- within ``4 d 2^-24 (|x| + max|e|)^2`` per distance (the bound
  the issue sets).  A (frame, head) whose float64 gap between the best and the second-best codeword exceeds that bound must have
  the float64 index; the others (at most 2 %, asserted) may have either.  quant / diff given the index are exact fp32
  expressions: ``x + (e - x)`` and ``(e - x)^2`` summed over the heads in order, divided by H.
"""
import ctypes
import functools

import numpy as np
import torch

E_SHAPE = -2

# ---- 1. bit identity with the resident kernel ----------------------------------------------------------------------------------
SAME_SHAPES = ((4, 64, 64), (1, 256, 64), (2, 128, 128), (8, 32, 512))          # H, d, K
SAME_N = (1, 16, 17, 37)
SAME_PARAMS = [(s, n) for s in range(len(SAME_SHAPES)) for n in SAME_N]
SAME_IDS = ['H%d d%d K%d N%d' % (SAME_SHAPES[s] + (n,)) for s, n in SAME_PARAMS]
# ---- 3. shapes only the streamed kernel takes ------------------------------------------------------------------------------------
LARGE_SHAPES = ((1, 256, 160), (1, 256, 512), (2, 128, 512), (1, 512, 96))
LARGE_N = (17, 37)
LARGE_PARAMS = [(s, n) for s in range(len(LARGE_SHAPES)) for n in LARGE_N]
LARGE_IDS = ['H%d d%d K%d N%d' % (LARGE_SHAPES[s] + (n,)) for s, n in LARGE_PARAMS]
MAX_LEFT_OUT = 0.02


@functools.lru_cache(maxsize=None)
def problem(H, d, K, N, seed):
    """seeded N(0, 1) frames [N, H d] and codebook [H, d, K] (host tensors, computed once, never modified)"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(N, H * d, generator=gen), torch.randn(H, d, K, generator=gen)


def search(dev, x, embed, chunk=None, alias=False):
    """the C entries directly: chunk None = msmc_vq_search, an int = msmc_vq_search_stream -> (rc, quant, diff, ind) on the host"""
    from msmctts_amd.hip import lib, vq
    H, d, K = embed.shape
    N, D = x.shape
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    xd = x.clone().to(dev)
    quant = xd if alias else torch.full((N, D), float('nan')).to(dev)
    diff = torch.full((N, d), float('nan')).to(dev)
    ind = torch.full((N, H), -7, dtype=torch.int64).to(dev)
    L = lib.get()
    if chunk is None:
        rc = L.msmc_vq_search(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(quant), lib.ptr(diff), lib.ptr(ind), N, D, H, K,
                              lib.stream(xd))
    else:
        rc = L.msmc_vq_search_stream(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(quant), lib.ptr(diff), lib.ptr(ind), N, D, H, K,
                                     chunk, lib.stream(xd))
    return rc, quant.cpu(), diff.cpu(), ind.cpu()


def last_kernel():
    from msmctts_amd.hip import lib
    return lib.get().msmc_vq_last_kernel().decode()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_same_bits_as_resident(dev, s, N):
    H, d, K = SAME_SHAPES[s]
    x, embed = problem(H, d, K, N, 4100 + s)
    rc, q0, d0, i0 = search(dev, x, embed)
    assert rc == 0 and last_kernel() != 'vq_search_stream_kernel', (rc, last_kernel())
    for chunk in (16, 48, 0):
        if chunk > K:
            continue
        rc, q1, d1, i1 = search(dev, x, embed, chunk)
        assert rc == 0 and last_kernel() == 'vq_search_stream_kernel', (rc, last_kernel())
        assert torch.equal(i1, i0), ('ind', chunk)
        assert same_bits(q1, q0), ('quant', chunk)
        assert same_bits(d1, d0), ('diff', chunk)
    if N == 37:                                     # quant aliasing x, once per shape
        rc, q2, d2, i2 = search(dev, x, embed, 16, alias=True)
        assert rc == 0 and torch.equal(i2, i0) and same_bits(q2, q0) and same_bits(d2, d0), 'quant aliasing x'


def check_lds_tile_family_same_bits(dev):
    """d % 16 != 0 (and d = 512): msmc_vq_search runs the LDS-tile kernel, whose channel order is 0 .. d-1 -- the streamed
    kernel's second family must give its bits"""
    for H, d, K, N in ((2, 20, 32, 37), (1, 512, 32, 17)):
        x, embed = problem(H, d, K, N, 4200 + d)
        rc, q0, d0, i0 = search(dev, x, embed)
        assert rc == 0 and last_kernel() == 'vq_search_kernel', (rc, last_kernel())
        for chunk in (16, 0):
            rc, q1, d1, i1 = search(dev, x, embed, chunk)
            assert rc == 0 and last_kernel() == 'vq_search_stream_kernel'
            assert torch.equal(i1, i0) and same_bits(q1, q0) and same_bits(d1, d0), (H, d, K, chunk)


# ---- 2. first minimum across chunks ---------------------------------------------------------------------------------------------
def check_first_minimum_across_chunks(dev, H, d, K):
    """codeword 5 copied to 21 and 37 (other chunks of 16), codeword 15 to 16 (next to it, across a chunk boundary): the copies are
    the same bits, so every frame is at exactly the same fp32 distance from all of them -- frames next to codeword 5 / 15 must get
    5 / 15, in every head"""
    gen = torch.Generator().manual_seed(4300 + H)
    embed = torch.randn(H, d, K, generator=gen)
    embed[:, :, 21] = embed[:, :, 5]
    embed[:, :, 37] = embed[:, :, 5]
    embed[:, :, 16] = embed[:, :, 15]
    N = 34
    which = torch.tensor([5, 15] * (N // 2))
    x = torch.cat([embed[h][:, which].t() for h in range(H)], dim=1).contiguous()      # [N, H d]
    x = x + 1e-3 * torch.randn(N, H * d, generator=gen)
    for chunk in (16, 0, None):
        rc, q, df, ind = search(dev, x, embed, chunk)
        assert rc == 0
        assert torch.equal(ind, which.view(N, 1).expand(N, H)), (chunk, ind.t())


# ---- 3. shapes only the streamed kernel takes ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference64(H, d, K, N, seed):
    """float64 distances -> (index [N, H], decided [N, H]: the gap to the second best exceeds the fp32 bound of the chain)"""
    x, embed = problem(H, d, K, N, seed)
    xh = x.double().view(N, H, d)
    e = embed.double()
    dist = (xh.pow(2).sum(-1, keepdim=True) - 2 * torch.einsum('nhd,hdk->nhk', xh, e)) + e.pow(2).sum(1).unsqueeze(0)
    two = dist.topk(2, dim=-1, largest=False)
    gap = two.values[..., 1] - two.values[..., 0]
    bound = 4 * d * 2.0 ** -24 * (xh.norm(dim=-1) + e.norm(dim=1).max(dim=-1).values.unsqueeze(0)) ** 2
    return two.indices[..., 0], gap > bound


def exact_outputs(x, embed, ind):
    """quant / diff of the kernels' epilogue given the indices: exact fp32 expressions"""
    H, d, K = embed.shape
    N = x.shape[0]
    xh = x.view(N, H, d)
    rows = torch.stack([embed[h].t()[ind[:, h]] for h in range(H)], dim=1)          # [N, H, d]
    e = rows - xh
    quant = (xh + e).reshape(N, H * d)
    acc = e[:, 0] * e[:, 0]
    for h in range(1, H):
        acc = acc + e[:, h] * e[:, h]
    return quant, acc / float(H) if H > 1 else acc


def check_large_shape(dev, s, N):
    H, d, K = LARGE_SHAPES[s]
    seed = 4400 + s
    x, embed = problem(H, d, K, N, seed)
    want, decided = reference64(H, d, K, N, seed)
    left_out = 1.0 - decided.double().mean().item()
    assert left_out <= MAX_LEFT_OUT, 'the float64 reference leaves %.3f of the pairs undecided' % left_out
    rc, q0, d0, i0 = search(dev, x, embed)
    assert rc == 0, 'msmc_vq_search refused H=%d d=%d K=%d: %d' % (H, d, K, rc)
    assert last_kernel() == 'vq_search_stream_kernel', last_kernel()
    rc, q1, d1, i1 = search(dev, x, embed, 16)
    assert rc == 0
    assert torch.equal(i1, i0) and same_bits(q1, q0) and same_bits(d1, d0), 'chunk 16 differs from the launcher choice'
    assert int(i0.min()) >= 0 and int(i0.max()) < K
    assert torch.equal(i0[decided], want[decided]), 'index differs from float64 on a decided pair'
    wq, wd = exact_outputs(x, embed, i0)
    assert same_bits(q0, wq), 'quant is not x + (e - x) of the chosen row'
    assert same_bits(d0, wd), 'diff is not the head-ordered mean of (e - x)^2'


# ---- 4. module level ------------------------------------------------------------------------------------------------------------
MODULES = (('Quantize', 256, 160, 1), ('MultiHeadQuantize', 256, 512, 2))
MODULE_IDS = ['%s(%d, %d) H%d' % m for m in MODULES]


def _restated_forward(x, lens, heads, ind, decay, eps, training):
    """reference modules.py:24-67 in plain torch, per head on its slice of the channels, with the arg-max replaced by the given
    indices; buffers in float64 -> (quant, diff, new heads); x requires grad"""
    B, T, D = x.shape
    H = len(heads)
    d = D // H
    quants, diffs, new = [], [], []
    for h, (embed, cs, ea) in enumerate(heads):
        xh = x[..., h * d:(h + 1) * d]
        K = embed.shape[1]
        q = torch.nn.functional.embedding(ind[..., h], embed.t())
        if training:
            valid = torch.cat([xh[i, :int(lens[i])] for i in range(B)], dim=0).detach().double()
            hot = torch.cat([torch.nn.functional.one_hot(ind[i, :int(lens[i]), h], K) for i in range(B)], dim=0).double()
            cs2 = cs.double() * decay + (1 - decay) * hot.sum(0)
            ea2 = ea.double() * decay + (1 - decay) * (valid.t() @ hot)
            n = cs2.sum()
            new.append((ea2 / ((cs2 + eps) / (n + K * eps) * n).unsqueeze(0), cs2, ea2))
        else:
            new.append((embed.double(), cs.double(), ea.double()))
        diffs.append((q.detach() - xh).pow(2))
        quants.append(xh + (q - xh).detach())
    return torch.cat(quants, dim=-1), sum(diffs) / H, new


def check_module(dev, m):
    from _parity import close
    from msmctts_amd.networks.vqgantts.modules import MultiHeadQuantize, Quantize
    name, D, K, H = MODULES[m]
    d = D // H
    gen = torch.Generator().manual_seed(4500 + m)
    q = Quantize(D, K) if H == 1 else MultiHeadQuantize(D, K, H)
    subs = [q] if H == 1 else list(q.quantizers)
    heads = []
    for sub in subs:
        e = torch.randn(d, K, generator=gen)
        sub.embed.copy_(e)
        sub.embed_avg.copy_(e)
        sub.cluster_size.fill_(0.5)
        heads.append((e.clone(), torch.full((K,), 0.5), e.clone()))
    q = q.to(dev)
    subs = [q] if H == 1 else list(q.quantizers)
    B, T = 3, 12
    x = torch.randn(B, T, D, generator=gen)
    lens = torch.tensor([12, 7, 3], dtype=torch.int64)
    w = torch.arange(B * T * d).view(B, T, d) / float(B * T * d)
    for training in (True, False):
        q.train(training)
        # float64 decision on the codebook as it stands, with the gap rule of the large-shape check
        xh = x.double().view(B * T, H, d)
        e64 = torch.stack([h_[0] for h_ in heads]).double()
        dist = (xh.pow(2).sum(-1, keepdim=True) - 2 * torch.einsum('nhd,hdk->nhk', xh, e64)) + e64.pow(2).sum(1).unsqueeze(0)
        two = dist.topk(2, dim=-1, largest=False)
        bound = 4 * d * 2.0 ** -24 * (xh.norm(dim=-1) + e64.norm(dim=1).max(dim=-1).values.unsqueeze(0)) ** 2
        decided = ((two.values[..., 1] - two.values[..., 0]) > bound).view(B, T, H)
        want_ind = two.indices[..., 0].view(B, T, H)
        assert 1.0 - decided.double().mean().item() <= MAX_LEFT_OUT
        xd = x.clone().to(dev).requires_grad_(True)
        qq, dd, ii = q(xd, lens.to(dev), update=True)
        got_ind = ii.cpu().view(B, T, H)
        assert torch.equal(got_ind[decided], want_ind[decided]), name + ' indices'
        ind = torch.where(decided, want_ind, got_ind)
        xr = x.clone().requires_grad_(True)
        q0, d0, new = _restated_forward(xr, lens, heads, ind, q.decay if H == 1 else subs[0].decay, subs[0].eps, training)
        scale = float(q0.detach().abs().max())
        close(qq, q0, 5e-6 * max(1.0, scale), what=name + ' quant')
        close(dd, d0, 5e-6 * max(1.0, scale * scale), 1e-5, what=name + ' diff')
        (qq.sum() * 0.5 + (dd * w.to(dev)).sum()).backward()
        (q0.sum() * 0.5 + (d0 * w).sum()).backward()
        close(xd.grad, xr.grad, 5e-6 * max(1.0, scale), 1e-5, what=name + ' grad')
        for h, sub in enumerate(subs):
            close(sub.embed, new[h][0], 1e-5 * max(1.0, float(new[h][0].abs().max())), 1e-5, what=name + ' embed')
            close(sub.cluster_size, new[h][1], 1e-6, 1e-6, what=name + ' cluster_size')
            close(sub.embed_avg, new[h][2], 1e-5, 1e-6, what=name + ' embed_avg')
        if training:         # the product's buffers are the reference of the next round: both sides continue from the same state
            heads = [(sub.embed.detach().cpu().clone(), sub.cluster_size.detach().cpu().clone(), sub.embed_avg.detach().cpu().clone())
                     for sub in subs]


# ---- 5. one train step end to end -----------------------------------------------------------------------------------------------
def large_codebook_config():
    """the small model of _parity's step checks with a single-head quantiser no resident kernel takes (d = 256, K = 160).
    n_model_size follows embedding_dims: the second stage's post-processor is ``Linear(2 * embedding_dims, ...)`` on the
    concatenation of the residual (n_model_size wide) and the quantised frames (reference msmc_vqgan.py), so the two widths
    must agree in every configuration the reference can build -- as they do in its own YAMLs (256 / 256)."""
    from _util import SMALL_TRAINER, small_task_cfg
    from msmctts_amd.utils.config import Config
    task = small_task_cfg()
    task['_name'] = 'MSMCTTS'
    task['autoencoder']['n_model_size'] = 256
    task['autoencoder']['quantizer_config'].update(n_heads=1, embedding_dims=256, embedding_sizes=160)
    return Config({'id': 'small-large-codebook', 'task': task, 'trainer': dict(SMALL_TRAINER, _name='VQGANTrainer'),
                   'optimizer': {'_default': dict(_name='AdamW', learning_rate=2e-4, betas=[0.8, 0.99], eps=1e-8, weight_decay=0.0)},
                   'dataset': dict(samplerate=24000, feature=['mel', 'wav'], frameshift=[300, 1])})


def build_trainer_for_steps(dev, graphed=False):
    import random
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    cfg = large_codebook_config()
    torch.manual_seed(4600)
    task = build_task(cfg, mode='train')
    for mod in task.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    task = task.to(dev).train()
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.model = task
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True) if graphed or dev != 'cpu' else build_optimizer(task, cfg.optimizer)
    tr.use_graphs = graphed
    tr.rng = random.Random(3)
    return task, tr


def step_batch(dev):
    from msmctts_amd.synthetic import make_batch
    batch = make_batch(3, 24, 80, 300, seed=5, device=dev)
    batch['mel_length_host'] = batch['mel_length'].tolist()
    return batch


def check_train_steps(dev):
    """one warm-up-phase and one GAN-phase step, eager: finite losses; parameters and codebooks move"""
    batch = step_batch(dev)
    for iteration in (0, 6):
        task, tr = build_trainer_for_steps(dev)
        before = {k: v.detach().clone() for k, v in task.state_dict().items()}
        task.zero_grad()
        log = tr.train_step(batch, iteration)
        assert last_kernel() == 'vq_search_stream_kernel', last_kernel()
        for k, v in log['loss'].items():
            assert np.isfinite(float(v)), (iteration, k, float(v))
        after = task.state_dict()
        moved = [k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k])]
        assert any(k.endswith('.embed') for k in moved), 'no codebook changed'
        assert any(k.startswith('autoencoder.encoder') for k in moved), 'no encoder parameter changed'
        for k in after:
            if after[k].dtype.is_floating_point:
                assert bool(torch.isfinite(after[k]).all()), k


def check_graphed_step_matches_eager(dev):
    """the GAN-phase step replayed from hipGraphs against the eager step (tolerances of test_gpu_parity.graphed_vs_eager)"""
    from _parity import close
    batch = step_batch(dev)
    results = []
    for graphed in (False, True):
        task, tr = build_trainer_for_steps(dev, graphed)
        if not tr.replays(6):
            task.zero_grad()
        log = tr.train_step(batch, 6)
        results.append(({k: float(v) for k, v in log['loss'].items()}, {k: v.detach().clone() for k, v in task.state_dict().items()}))
    (el, es), (gl, gs) = results
    assert set(el) == set(gl)
    for k in el:
        assert abs(el[k] - gl[k]) <= 2e-3 * max(1.0, abs(el[k])), (k, el[k], gl[k])
    for k in es:
        if es[k].dtype.is_floating_point:
            close(gs[k], es[k], 2e-3, 1e-3, k)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    """K % 16, d % 4 and a forced chunk that is no multiple of 16 return the shape error and launch nothing (the NaN-filled outputs
    stay NaN); N = 0 returns 0 and writes nothing; the wrapper raises"""
    from msmctts_amd.hip import lib, vq
    for H, d, K, chunk in ((1, 64, 24, 0), (1, 6, 32, 0), (1, 64, 64, 20), (1, 64, 64, -16), (1, 64, 64, 272)):
        gen = torch.Generator().manual_seed(4700)
        x, embed = torch.randn(5, H * d, generator=gen), torch.randn(H, d, K, generator=gen)
        rc, q, df, ind = search(dev, x, embed, chunk)
        assert rc == E_SHAPE, (H, d, K, chunk, rc)
        assert bool(torch.isnan(q).all()) and bool(torch.isnan(df).all()) and bool((ind == -7).all()), 'a refused call launched'
        if chunk == 0:
            rc, q, df, ind = search(dev, x, embed)
            assert rc == E_SHAPE, (H, d, K, rc)
    # a forced chunk that does not fit LDS: 2 x 112 rows of 260 floats + norms > 160 KiB
    x, embed = problem(1, 256, 512, 17, 4401)
    rc, q, df, ind = search(dev, x, embed, 112)
    assert rc == E_SHAPE and bool(torch.isnan(q).all()), rc
    # N = 0: guard rows around empty outputs stay untouched
    embed = problem(1, 256, 160, 17, 4400)[1]
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    guard = torch.full((2, 256), 7.0).to(dev)
    gi = torch.full((2, 1), -7, dtype=torch.int64).to(dev)
    L = lib.get()
    for chunk in (0, 16):
        rc = L.msmc_vq_search_stream(lib.ptr(guard), lib.ptr(et), lib.ptr(en), lib.ptr(guard), lib.ptr(guard), lib.ptr(gi), 0, 256, 1, 160,
                                     chunk, lib.stream(guard))
        assert rc == 0
    assert bool((guard.cpu() == 7).all()) and bool((gi.cpu() == -7).all())
    with _raises(RuntimeError, 'msmc_vq_search_stream failed with code -2'):
        vq.vq_search(torch.zeros(4, 256).to(dev), et, en, stream_chunk=20)


def check_wrapper_threads_the_chunk(dev):
    """hip/vq.py: stream_chunk=None goes through msmc_vq_search, an int through msmc_vq_search_stream -- same bits, and the
    backward of the streamed form is the element-wise kernel's"""
    from msmctts_amd.hip import vq
    x, embed = problem(4, 64, 64, 37, 4100)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    xa = x.clone().to(dev).requires_grad_(True)
    xb = x.clone().to(dev).requires_grad_(True)
    qa, da, ia = vq.vq_search(xa, et, en, shortlist=False)
    assert last_kernel() != 'vq_search_stream_kernel'
    qb, db, ib = vq.vq_search(xb, et, en, stream_chunk=16)
    assert last_kernel() == 'vq_search_stream_kernel'
    assert torch.equal(ia.cpu(), ib.cpu()) and same_bits(qa.detach().cpu(), qb.detach().cpu()) and same_bits(da.detach().cpu(), db.detach().cpu())
    (qa.sum() + (da * 0.25).sum()).backward()
    (qb.sum() + (db * 0.25).sum()).backward()
    assert same_bits(xa.grad.cpu(), xb.grad.cpu())


class _raises(object):
    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc) and self.text in str(val), (tp, val)
        return True


def check_feature_present():
    from msmctts_amd.hip import lib
    assert 'msmc_vq_search_stream' in lib.exported_symbols()
    assert isinstance(lib.get().msmc_vq_search_stream, ctypes._CFuncPtr)
