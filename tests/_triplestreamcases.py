"""Shared cases of the streamed triple loss (csrc/triple_stream.inc, msmc_triple_loss_stream, and hip/losses.py triple_loss where
no head's codebook fits LDS): tests/test_triple_stream_emu.py runs them on the kernel interpreter, tests/test_gpu_triple_stream.py
on the GPU.

References:
* where the resident kernel takes the shape: msmc_triple_loss itself, BIT-EXACT (L = 1: the same chain over the channels, codewords
  in ascending k -- the chunking must not show);
* on the large shapes (d = 256 / 512, or K d beyond LDS), where a frame's channels are split over L lanes:
  - an integer lattice (codebook and predictions in {-2 .. 2}, margin 0): every product and every partial sum is an integer below
    2^24 (d 16 <= 8192 per distance, K 8192 per loss before the exact division by d), so the fp32 result is the float64 result
    in ANY order of summation: bit-equal for 'sum' (1 / d is a power of two), and for 'mean' with K = 512; K = 160 / 96 round
    1 / K, the product with the loss and the gradient scale: relative 2^-22;
  - real values against the same expressions in float64 with a derived budget.  One distance (|p|^2 - 2 p.e) + |e|^2 in fp32 is
    within b = 4 d 2^-24 (|p| + max|e|)^2 of the exact one (the bound of tests/_vqstreamcases.py reference64), pos likewise, so a
    hinge term t_k + margin is off by at most 2 b; a term with |t_k + margin| <= b on the float64 side ("undecided") may be
    counted on one side only.  loss: scale (2 b / d) (n_active64 + n_undecided + 1).  gradient, per channel:
    scale (2 / d) (sum_{k undecided, k != trg} |e_k - e_trg| + K 2^-23 max_k |e_k - e_trg|), the second term for the fp32
    accumulation of up to K rows.  No frame is excluded.
"""
import ctypes
import functools

import numpy as np
import torch

E_SHAPE = -2
RESIDENT, STREAMED = 'triple_loss_kernel', 'triple_loss_stream_kernel'

# ---- 1. bit identity with the resident kernel ----------------------------------------------------------------------------------
SAME_SHAPES = ((1, 64, 64), (4, 64, 256), (2, 32, 48))              # H, d, K
SAME_N = (1, 37, 300)
SAME_PARAMS = [(s, n) for s in range(len(SAME_SHAPES)) for n in SAME_N]
SAME_IDS = ['H%d d%d K%d N%d' % (SAME_SHAPES[s] + (n,)) for s, n in SAME_PARAMS]
# ---- 2-4. shapes only the streamed kernel takes ----------------------------------------------------------------------------------
LARGE_SHAPES = ((1, 256, 512), (2, 128, 512), (1, 256, 160), (1, 512, 96))
LARGE_N = (37, 300)
LARGE_PARAMS = [(s, n) for s in range(len(LARGE_SHAPES)) for n in LARGE_N]
LARGE_IDS = ['H%d d%d K%d N%d' % (LARGE_SHAPES[s] + (n,)) for s, n in LARGE_PARAMS]
LATTICE_CHUNKS = (24, 16, 0)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def last_kernel():
    from msmctts_amd.hip import lib
    return lib.get().msmc_loss_last_kernel().decode()


def run(dev, p, trg, embed, margin, mean, chunk=None):
    """the C entries directly: chunk None = msmc_triple_loss, an int = msmc_triple_loss_stream -> (rc, lossh, gp) on the host;
    the outputs start as NaN"""
    from msmctts_amd.hip import lib, vq
    H, d, K = embed.shape
    N, D = p.shape
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    pd, td = p.clone().to(dev), trg.clone().to(dev)
    lossh = torch.full((N, H), float('nan')).to(dev)
    gp = torch.full((N, D), float('nan')).to(dev)
    L = lib.get()
    args = (lib.ptr(pd), lib.ptr(td), lib.ptr(et), lib.ptr(en), lib.ptr(lossh), lib.ptr(gp), N, D, H, K, float(margin), int(mean))
    if chunk is None:
        rc = L.msmc_triple_loss(*args, lib.stream(pd))
    else:
        rc = L.msmc_triple_loss_stream(*args, chunk, lib.stream(pd))
    return rc, lossh.cpu(), gp.cpu()


@functools.lru_cache(maxsize=None)
def near_problem(H, d, K, N, spread, seed):
    """inputs as in _parity.check_triple_loss: N(0, 1) codebook [H, d, K], random targets, predictions = target row + spread * noise
    (host tensors, computed once, never modified)"""
    gen = torch.Generator().manual_seed(seed)
    embed = torch.randn(H, d, K, generator=gen)
    trg = torch.randint(0, K, (N, H), generator=gen)
    near = torch.cat([embed[h].t()[trg[:, h]] for h in range(H)], dim=-1)
    return (near + spread * torch.randn(N, H * d, generator=gen)).contiguous(), trg, embed


def check_same_bits_as_resident(dev, s, N):
    H, d, K = SAME_SHAPES[s]
    for spread in (0.05, 3.0):
        p, trg, embed = near_problem(H, d, K, N, spread, 5100 + s)
        for mean in (0, 1):
            rc, l0, g0 = run(dev, p, trg, embed, 1e-6, mean)
            assert rc == 0 and last_kernel() == RESIDENT, (rc, last_kernel())
            assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(g0).all())
            for chunk in (16, 40, K):
                rc, l1, g1 = run(dev, p, trg, embed, 1e-6, mean, chunk)
                assert rc == 0 and last_kernel() == STREAMED, (rc, last_kernel())
                assert same_bits(l1, l0), ('lossh', spread, mean, chunk, (l1 - l0).abs().max().item())
                assert same_bits(g1, g0), ('gp', spread, mean, chunk, (g1 - g0).abs().max().item())


# ---- 2. chunk invariance on the large shapes -----------------------------------------------------------------------------------
def check_chunk_invariance(dev, s, N):
    H, d, K = LARGE_SHAPES[s]
    for spread, mean in ((0.05, 0), (3.0, 1)):
        p, trg, embed = near_problem(H, d, K, N, spread, 5200 + s)
        rc, l0, g0 = run(dev, p, trg, embed, 1e-6, mean, 0)
        assert rc == 0 and last_kernel() == STREAMED, (rc, last_kernel())
        assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(g0).all())
        for chunk in (16, 24):
            rc, l1, g1 = run(dev, p, trg, embed, 1e-6, mean, chunk)
            assert rc == 0 and last_kernel() == STREAMED, (rc, last_kernel())
            assert same_bits(l1, l0) and same_bits(g1, g0), ('chunk %d differs from the launcher choice' % chunk, spread, mean)


# ---- float64 evaluation of the kernel's expressions ------------------------------------------------------------------------------
def reference64(p, trg, embed, margin, mean):
    """-> dict of float64 tensors: loss [N, H], gp [N, H d], t [N, H, K] (pos - dist), active [N, H, K], b [N, H]"""
    H, d, K = embed.shape
    N = p.shape[0]
    x = p.double().view(N, H, d)
    e = embed.double()                                                   # [H, d, K]
    rows = e.permute(0, 2, 1)                                            # [H, K, d]
    et = torch.stack([rows[h][trg[:, h].clamp(0, K - 1)] for h in range(H)], dim=1)      # [N, H, d]
    dist = (x.pow(2).sum(-1, keepdim=True) - 2 * torch.einsum('nhd,hdk->nhk', x, e)) + e.pow(2).sum(1).unsqueeze(0)
    pos = (x - et).pow(2).sum(-1, keepdim=True)
    t = pos - dist
    v = t + margin
    active = (t != 0) & (v > 0)
    scale = 1.0 / K if mean else 1.0
    loss = (active * v / d).sum(-1) * scale
    act = active.double()
    gsum = torch.einsum('nhk,hkd->nhd', act, rows) - act.sum(-1, keepdim=True) * et
    gp = (2.0 / d) * scale * gsum
    b = 4 * d * 2.0 ** -24 * (x.norm(dim=-1) + e.norm(dim=1).max(dim=-1).values.unsqueeze(0)) ** 2
    return dict(loss=loss, gp=gp.reshape(N, H * d), t=t, active=active, b=b, et=et, rows=rows, scale=scale)


# ---- 3. exact on an integer lattice -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_problem(H, d, K, N, seed):
    """codebook and predictions in {-2 .. 2}; targets planted at the chunk boundaries of the forced chunks (16, 24) and at both ends
    of K; codeword 5 duplicated at K - 2 (an exact tie with the target for targets 5 and K - 2: t_k == 0 at k != trg); frames
    9 .. 11 are exactly a non-target codeword (distance 0 to it: the largest hinge term), frames 12 .. 14 exactly the target"""
    gen = torch.Generator().manual_seed(seed)
    embed = torch.randint(-2, 3, (H, d, K), generator=gen).float()
    embed[:, :, K - 2] = embed[:, :, 5]
    trg = torch.randint(0, K, (N, H), generator=gen)
    planted = (0, 15, 16, 23, 24, K - 1, 5, K - 2, 5)
    for i, k in enumerate(planted[:N]):
        trg[i] = k
    rows = torch.cat([embed[h].t()[trg[:, h]] for h in range(H)], dim=-1)
    # sparse integer noise: a few channels moved by +-1 (near: small hinge sets) or every channel redrawn (far)
    noise = torch.randint(-1, 2, (N, H * d), generator=gen).float() * (torch.rand(N, H * d, generator=gen) < 0.05)
    p = (rows + noise).clamp(-2, 2)
    far = torch.arange(N) % 3 == 2
    p[far] = torch.randint(-2, 3, (int(far.sum()), H * d), generator=gen).float()
    for n in range(9, min(N, 12)):
        other = (trg[n] + 7) % (K - 2)               # (never the target, never its duplicate)
        p[n] = torch.cat([embed[h][:, other[h]] for h in range(H)])
    for n in range(12, min(N, 15)):
        p[n] = rows[n]
    return p.contiguous(), trg, embed


def check_lattice(dev, s, N):
    H, d, K = LARGE_SHAPES[s]
    p, trg, embed = lattice_problem(H, d, K, N, 5300 + s)
    assert float(p.abs().max()) <= 2 and float(embed.abs().max()) <= 2
    for mean in (0, 1):
        ref = reference64(p, trg, embed, 0.0, mean)
        if N > 14:
            assert bool((ref['t'][9:12].amax(-1) > 0).all()) and bool((ref['loss'][12:15] >= 0).all())
            tie = ref['t'][6, :, K - 2]
            assert bool((tie == 0).all()), 'the duplicate of the target is not an exact tie'
        assert float(ref['active'].double().sum(-1).mean()) > 1, 'the lattice case has no hinge terms'
        want_l, want_g = ref['loss'].float(), ref['gp'].float()
        exact = (not mean) or (K & (K - 1)) == 0
        for chunk in LATTICE_CHUNKS:
            rc, l1, g1 = run(dev, p, trg, embed, 0.0, mean, chunk)
            assert rc == 0 and last_kernel() == STREAMED, (rc, last_kernel())
            if exact:
                assert same_bits(l1, want_l), ('lossh', mean, chunk, (l1 - want_l).abs().max().item())
                assert same_bits(g1, want_g), ('gp', mean, chunk, (g1 - want_g).abs().max().item())
            else:
                rel = 2.0 ** -22
                assert bool(((l1.double() - ref['loss']).abs() <= rel * ref['loss'].abs()).all()), ('lossh', mean, chunk)
                assert bool(((g1.double() - ref['gp']).abs() <= rel * ref['gp'].abs()).all()), ('gp', mean, chunk)


# ---- 4. real values against float64 with the derived budget -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clustered_problem(H, d, K, N, seed):
    """codebook: 8 centres + 0.3 * noise; predictions e_trg + alpha (e_other - e_trg) + spread * noise, alpha ~ U(0, 1), spreads
    0.05 / 0.5 / 3.0 by frame"""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.randn(H, d, 8, generator=gen)
    embed = centres[:, :, torch.arange(K) % 8] + 0.3 * torch.randn(H, d, K, generator=gen)
    trg = torch.randint(0, K, (N, H), generator=gen)
    other = torch.randint(0, K, (N, H), generator=gen)
    alpha = torch.rand(N, H, 1, generator=gen)
    et = torch.stack([embed[h].t()[trg[:, h]] for h in range(H)], dim=1)
    eo = torch.stack([embed[h].t()[other[:, h]] for h in range(H)], dim=1)
    spread = torch.tensor([0.05, 0.5, 3.0])[torch.arange(N) % 3].view(N, 1, 1)
    p = et + alpha * (eo - et) + spread * torch.randn(N, H, d, generator=gen)
    return p.reshape(N, H * d).contiguous(), trg, embed.contiguous()


def budgets(ref, margin):
    """(loss budget [N, H], gradient budget [N, H d]) of the module docstring, from the float64 side alone"""
    H, K, d = ref['rows'].shape
    N = ref['t'].shape[0]
    b = ref['b']
    und = (ref['t'] + margin).abs() <= b.unsqueeze(-1)                                  # [N, H, K]
    n_act = ref['active'].double().sum(-1)
    loss_b = ref['scale'] * (2 * b / d) * (n_act + und.double().sum(-1) + 1)
    delta = (ref['rows'].unsqueeze(0) - ref['et'].unsqueeze(2)).abs()                   # [N, H, K, d] (the target's own row: 0)
    grad_b = ref['scale'] * (2.0 / d) * (torch.einsum('nhk,nhkd->nhd', und.double(), delta) + K * 2.0 ** -23 * delta.amax(2))
    return loss_b, grad_b.reshape(N, H * d), und


def check_real_values(dev, s, N, report=None):
    """measured, interpreter and MI355X alike: the loss uses under 0.2 % of its budget, the gradient at most 0.45 of its budget (the
    split kernels add the active rows with a compensated sum; a plain fp32 chain over ~435 active rows reached 2.9 x the budget)"""
    H, d, K = LARGE_SHAPES[s]
    p, trg, embed = clustered_problem(H, d, K, N, 5400 + s)
    for mean in (0, 1):
        ref = reference64(p, trg, embed, 1e-6, mean)
        loss_b, grad_b, und = budgets(ref, 1e-6)
        rc, l1, g1 = run(dev, p, trg, embed, 1e-6, mean, 0)
        assert rc == 0 and last_kernel() == STREAMED, (rc, last_kernel())
        le = (l1.double() - ref['loss']).abs()
        ge = (g1.double() - ref['gp']).abs()
        figures = dict(shape=(H, d, K, N), mean=mean, loss_err_over_budget=float((le / loss_b).max()),
                       grad_err_over_budget=float((ge / grad_b).max()), mean_active=float(ref['active'].double().sum(-1).mean()),
                       frames_with_undecided=float((und & (ref['t'] != 0)).any(-1).any(-1).double().mean()))
        print(figures)
        if report is not None:
            report.append(figures)
        assert bool((le <= loss_b).all()), figures
        assert bool((ge <= grad_b).all()), figures


# ---- 5. module level ------------------------------------------------------------------------------------------------------------
MODULES = (('Quantize', 256, 512, 1), ('MultiHeadQuantize', 256, 512, 2))
MODULE_IDS = ['%s(%d, %d) H%d' % m for m in MODULES]


def check_module(dev, m):
    from msmctts_amd.networks.vqgantts.modules import MultiHeadQuantize, Quantize
    from oracle import predictor as op
    name, D, K, H = MODULES[m]
    d = D // H
    B, T = 3, 37
    p, trg, embed = clustered_problem(H, d, K, B * T, 5500 + m)
    q = Quantize(D, K) if H == 1 else MultiHeadQuantize(D, K, H)
    for h, sub in enumerate([q] if H == 1 else list(q.quantizers)):
        sub.embed.copy_(embed[h])
    q = q.to(dev)
    gen = torch.Generator().manual_seed(5600 + m)
    wts = torch.rand(B, T, generator=gen)
    trg_in = (trg[:, 0].view(B, T) if H == 1 else trg.view(B, T, H)).to(dev)
    for reduction in ('sum', 'mean'):
        ref = reference64(p, trg, embed, 1e-6, reduction == 'mean')
        loss_b, grad_b, _ = budgets(ref, 1e-6)
        # the oracle (reference expressions, per head, then the head mean) evaluated in float64
        p64 = p.double().view(B, T, D).requires_grad_(True)
        want = sum(op.triple_loss(c, trg[:, h].view(B, T), embed[h].double(), reduction)
                   for h, c in enumerate(torch.chunk(p64, H, dim=-1))) / H
        (want * wts.double()).sum().backward()
        p1 = p.view(B, T, D).clone().to(dev).requires_grad_(True)
        got = q.compute_triple_loss(p1, trg_in, reduction=reduction)
        assert last_kernel() == STREAMED, last_kernel()
        assert got.shape == (B, T)
        (got * wts.to(dev)).sum().backward()
        le = (got.detach().cpu().double() - want.detach()).abs().view(B * T)
        assert bool((le <= loss_b.sum(-1) / H).all()), (name, reduction, float((le / (loss_b.sum(-1) / H)).max()))
        ge = (p1.grad.cpu().double() - p64.grad).abs().view(B * T, D)
        gb = grad_b * wts.double().view(B * T, 1) / H
        assert bool((ge <= gb).all()), (name, reduction, float((ge / gb).max()))
    # reduction='none' keeps the stock chain: the [B, T, K] tensor
    none = q.compute_triple_loss(p.view(B, T, D).to(dev), trg_in, reduction='none')
    assert none.shape == (B, T, K)
    want = sum(op.triple_loss(c, trg[:, h].view(B, T), embed[h], 'none') for h, c in enumerate(torch.chunk(p.view(B, T, D), H, dim=-1))) / H
    assert float((none.cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


# ---- 6. predictor step --------------------------------------------------------------------------------------------------------------
def build_predictor_step(dev, graphed=False):
    """a tiny PredictorTrainer whose frozen autoencoder has the single-head 256 x 160 quantiser of
    _vqstreamcases.large_codebook_config (no resident triple-loss kernel takes it) -> (task, trainer, autoencoder task, batch)"""
    from _util import PREDICTOR_TRAINER, load_npz, small_predictor_cfg, t
    from _vqstreamcases import large_codebook_config
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    z = load_npz('small_predictor.npz')
    pc = small_predictor_cfg()
    pc['n_pred_size'] = 256
    cfg = Config({'id': 'small_predictor_large_codebook',
                  'task': {'_name': 'MSMCTTS', '_mode': 'train_predictor', 'predictor': pc},
                  'trainer': dict(PREDICTOR_TRAINER, _name='PredictorTrainer'),
                  'optimizer': {'_default': dict(_name='Adam', learning_rate=2e-4, betas=[0.9, 0.98], eps=1e-9, weight_decay=0)},
                  'dataset': dict(samplerate=24000, feature=['mel', 'wav'], frameshift=[300, 1])})
    torch.manual_seed(5700)
    atask = build_task(large_codebook_config(), mode='train')
    task = build_task(cfg, mode='train')
    for mod in list(task.modules()) + list(atask.modules()):
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    atask = atask.to(dev)
    task = task.to(dev).train()
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.autoencoder = atask.autoencoder
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True) if graphed or dev != 'cpu' else build_optimizer(task, cfg.optimizer)
    tr.use_graphs = graphed
    batch = {k[len('batch.'):]: t(v).to(dev) for k, v in z.items() if k.startswith('batch.')}
    return task, tr, atask, batch


def check_predictor_step(dev):
    """one eager step: the 'triple_sum' terms of both stages against oracle.predictor.embedding_loss on the product's own
    predictions (teacher-forced forward, no dropout), at the tolerance of _parity.check_predictor_step"""
    from _parity import TOL
    from _util import PREDICTOR_TRAINER
    from oracle import predictor as op
    task, tr, atask, batch = build_predictor_step(dev)
    atask.autoencoder.eval()
    with torch.no_grad():
        qs = atask.autoencoder.analysis(batch['mel'], batch['mel_length'].int())
        fo = task.predictor(text=batch['text'], text_length=batch['text_length'], dur=batch['dur'],
                            feat=[f.float() for f in qs['quantizer_outputs']], feat_length=qs['quantizer_lengths'])
    P_ae = {k: v.detach().cpu() for k, v in atask.state_dict().items()}
    targets = {k: [x.detach().cpu() for x in v] for k, v in qs.items() if k in ('quantizer_outputs', 'quantizer_indices')}
    want = op.embedding_loss(P_ae, 'autoencoder.quantizer', 1, [f.detach().float().cpu() for f in fo['feat']],
                             [l.cpu() for l in fo['feat_length']], targets, PREDICTOR_TRAINER['training_methods'],
                             PREDICTOR_TRAINER['loss_weights'])
    task.zero_grad()
    log = tr.train_step({k: v.clone() for k, v in batch.items()}, 0)
    assert last_kernel() == STREAMED, last_kernel()
    keys = [k for k in want if k.startswith('embed_loss_triple_sum_')]
    assert len(keys) == 2, sorted(want)
    for k in keys + [k for k in want if k.startswith('embed_loss_mse_')]:
        got, v = float(log['loss'][k]), float(want[k])
        assert np.isfinite(got) and abs(got - v) <= TOL * max(1.0, abs(v)), (k, got, v)


def check_graphed_predictor_step_matches_eager(dev):
    """the step replayed from hipGraphs gives the eager step's losses bit for bit (same kernels, same inputs, same order)"""
    results = []
    for graphed in (False, True):
        task, tr, atask, batch = build_predictor_step(dev, graphed)
        if not tr.replays(0):
            task.zero_grad()
        log = tr.train_step({k: v.clone() for k, v in batch.items()}, 0)
        assert last_kernel() == STREAMED, last_kernel()
        if graphed:
            assert tr._graphs is not None
        results.append({k: torch.as_tensor(v).detach().float().cpu().reshape(1) for k, v in log['loss'].items()})
    eager, replayed = results
    assert set(eager) == set(replayed)
    for k in eager:
        assert same_bits(eager[k], replayed[k]), (k, float(eager[k]), float(replayed[k]))


# ---- 7. refusals and the empty input ------------------------------------------------------------------------------------------------
def check_refusals(dev):
    from msmctts_amd.hip import lib, vq
    gen = torch.Generator().manual_seed(5800)

    def refused(H, d, K, chunk, N=5):
        p = torch.randn(N, H * d, generator=gen)
        rc, l, g = run(dev, p, torch.zeros(N, H, dtype=torch.int64), torch.randn(H, d, K, generator=gen), 1e-6, 0, chunk)
        assert rc == E_SHAPE, (H, d, K, chunk, rc)
        assert bool(torch.isnan(l).all()) and bool(torch.isnan(g).all()), 'a refused call launched'
    refused(1, 160, 32, 0)                  # d outside the supported sizes
    refused(1, 64, 64, -1)                  # chunk out of range
    refused(1, 256, 512, 96)                # two buffers of 96 x 257 floats: 193 KiB
    refused(1, 256, 512, None)              # msmc_triple_loss itself still refuses what does not fit LDS
    refused(1, 512, 96, None)
    # a misaligned p
    p, trg, embed = near_problem(1, 64, 64, 37, 0.05, 5100)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    flat = torch.zeros(37 * 64 + 4).to(dev)
    off = flat[1:1 + 37 * 64].view(37, 64)
    assert off.data_ptr() % 16 == 4
    lossh = torch.full((37, 1), float('nan')).to(dev)
    gp = torch.full((37, 64), float('nan')).to(dev)
    td = trg.to(dev)
    L = lib.get()
    rc = L.msmc_triple_loss_stream(ctypes.c_void_p(off.data_ptr()), lib.ptr(td), lib.ptr(et), lib.ptr(en), lib.ptr(lossh), lib.ptr(gp),
                                   37, 64, 1, 64, 1e-6, 0, 16, lib.stream(td))
    assert rc == E_SHAPE and bool(torch.isnan(lossh.cpu()).all()) and bool(torch.isnan(gp.cpu()).all())
    # N = 0: 0 and nothing written
    for chunk in (0, 16):
        rc = L.msmc_triple_loss_stream(lib.ptr(flat), lib.ptr(td), lib.ptr(et), lib.ptr(en), lib.ptr(lossh), lib.ptr(gp), 0, 64, 1, 64,
                                       1e-6, 0, chunk, lib.stream(td))
        assert rc == 0
    assert bool(torch.isnan(lossh.cpu()).all()) and bool(torch.isnan(gp.cpu()).all())


def check_wrapper_routes(dev):
    """hip/losses.py triple_loss: chunk=None takes the resident entry where it fits and the streamed one otherwise, an int forces the
    streamed entry; same bits and the same backward where both take the shape"""
    from msmctts_amd.hip import losses, vq
    p, trg, embed = near_problem(4, 64, 256, 37, 3.0, 5101)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    pa = p.clone().to(dev).requires_grad_(True)
    pb = p.clone().to(dev).requires_grad_(True)
    la = losses.triple_loss(pa, trg.to(dev), et, en, 'sum')
    assert last_kernel() == RESIDENT
    lb = losses.triple_loss(pb, trg.to(dev), et, en, 'sum', chunk=24)
    assert last_kernel() == STREAMED
    assert same_bits(la.detach().cpu(), lb.detach().cpu())
    w = torch.arange(37 * 4).view(37, 4).float().to(dev) / 100
    (la * w).sum().backward()
    (lb * w).sum().backward()
    assert same_bits(pa.grad.cpu(), pb.grad.cpu())
    p, trg, embed = near_problem(1, 256, 160, 37, 3.0, 5202)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    losses.triple_loss(p.to(dev), trg.to(dev), et, en, 'mean')
    assert last_kernel() == STREAMED


# ---- 8. the symbols ---------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    assert 'msmc_triple_loss_stream' in lib.exported_symbols()
    assert 'msmc_loss_last_kernel' in lib.debug_symbols()
    assert isinstance(lib.get().msmc_triple_loss_stream, ctypes._CFuncPtr)
    assert isinstance(lib.get().msmc_loss_last_kernel, ctypes._CFuncPtr)
