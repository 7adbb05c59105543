"""The normalised quantiser (``norm: True``: nn.BatchNorm1d behind every stage's pre-processor, reference
vqgantts/msmc_vqgan.py:115-123) on the kernels: on the interpreter where it is bound (``cpu``) and on the GPU (``cuda``, -m gpu).

The comparison target is the module's own stock-operator path (``use_hip = False`` set by hand) and the fp64 evaluation of the
same pre-processor.  Bound of every compared tensor: 4 x the measured max abs error of the stock fp32 path against fp64 on the same
case, with a floor of 4 fp32 ulps of the tensor's largest entry (the margin is for another order of the sums) -- the rule of
tests/_bncases.py with the stock path as the fp32 yardstick."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch

from _bncases import ulp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')


@pytest.fixture(params=['cpu', pytest.param('cuda', marks=pytest.mark.gpu)])
def dev(request):
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    if request.param == 'cpu':
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
        lib.use_library_for_tests(EMU)
    else:
        lib._lib, lib._host_pointers_ok = lib.load(), False
    yield request.param
    lib._lib, lib._host_pointers_ok = saved


def quantiser(n_model_size=32, **kw):
    from msmctts_amd.networks.vqgantts.msmc_vqgan import MultiStageQuantizer
    args = dict(upsample_scales=[1], embedding_sizes=32, embedding_dims=64, n_heads=4, dropout=0.0, norm=True)
    args.update(kw)
    torch.manual_seed(3)
    return MultiStageQuantizer(n_model_size, **args)


def test_norm_true_selects_the_kernels_and_the_library_exports_them():
    """fails on the parent commit: ``use_hip = not norm`` there, and no msmc_bn_* entry point"""
    from msmctts_amd.hip import lib
    assert quantiser().use_hip is True
    assert 'msmc_bn_fwd' in lib.exported_symbols()
    handle = lib.load()
    for name in ('msmc_bn_workspace', 'msmc_bn_fwd', 'msmc_bn_eval_fwd', 'msmc_bn_bwd', 'msmc_bn_eval_bwd'):
        assert hasattr(handle, name), name


def test_state_dict_keys_are_the_plain_ones_plus_the_batchnorm_buffers():
    plain = set(quantiser(upsample_scales=[2, 1], norm=False).state_dict())
    normed = set(quantiser(upsample_scales=[2, 1], norm=True).state_dict())
    extra = {'preprocessor.%d.3.%s' % (i, k) for i in range(2) for k in ('running_mean', 'running_var', 'num_batches_tracked')}
    assert plain < normed and normed - plain == extra


def _bound(stock, ref64):
    return max(4 * float(np.abs(stock - ref64).max()), 4 * ulp32(np.abs(ref64).max()))


def _np(t):
    return t.detach().double().cpu().numpy()


def test_single_stage_matches_the_stock_path(dev):
    hip = quantiser().to(dev).train()
    stock = copy.deepcopy(hip)
    stock.use_hip = False
    pre64 = copy.deepcopy(hip.preprocessor[0]).double()
    rng = np.random.default_rng(5)
    emb = torch.from_numpy(rng.standard_normal((3, 50, 32))).float().to(dev)
    w = torch.from_numpy(rng.standard_normal((3, 50, 64))).float().to(dev)
    lengths = torch.tensor([50, 37, 8], dtype=torch.int32, device=dev)
    bufs = ('running_mean', 'running_var', 'num_batches_tracked')

    for training in (True, False):               # the evaluation call follows the training call: its statistics are the blended ones
        got = {}
        for name, q in (('hip', hip), ('stock', stock)):
            q.train(training)
            q.zero_grad()
            seen = []
            handle = q.quantizer[0].register_forward_hook(lambda m, inp, out: seen.append(inp[0]))
            e = emb.clone().requires_grad_(True)
            q([(e, lengths)])
            handle.remove()
            q_in, = seen
            assert q_in.dtype == torch.float32
            (q_in * w).sum().backward()
            pre = q.preprocessor[0]
            got[name] = dict(q_in=_np(q_in), emb=_np(e.grad), w0=_np(pre[0].weight.grad), b0=_np(pre[0].bias.grad),
                             w2=_np(pre[2].weight.grad), b2=_np(pre[2].bias.grad),
                             **{k: _np(getattr(pre[3], k)) for k in bufs})
        pre64.train(training)
        pre64.zero_grad()
        e = emb.double().clone().requires_grad_(True)
        q64 = pre64(e.transpose(1, 2)).transpose(1, 2)
        (q64 * w.double()).sum().backward()
        ref = dict(q_in=_np(q64), emb=_np(e.grad), w0=_np(pre64[0].weight.grad), b0=_np(pre64[0].bias.grad),
                   w2=_np(pre64[2].weight.grad), b2=_np(pre64[2].bias.grad), **{k: _np(getattr(pre64[3], k)) for k in bufs})
        assert ref['num_batches_tracked'] == got['hip']['num_batches_tracked'] == got['stock']['num_batches_tracked'] == 1
        for k in ('q_in', 'running_mean', 'running_var', 'emb', 'w0', 'b0', 'w2', 'b2'):
            bound = _bound(got['stock'][k], ref[k])
            err = float(np.abs(got['hip'][k] - ref[k]).max())
            print('quantiser norm %s %-5s %-12s err %.3e  bound %.3e  (stock path: %.3e)'
                  % (dev, 'train' if training else 'eval', k, err, bound, float(np.abs(got['stock'][k] - ref[k]).max())))
            assert err <= bound, (k, training, err, bound)


def test_two_stage_bf16_smoke(dev):
    # (later stages concatenate the residual and the codewords: the reference's widths need n_model_size == embedding_dims)
    q = quantiser(64, upsample_scales=[2, 1], dropout=0.1).to(dev).train()
    q.hip_dtype = torch.bfloat16
    rng = np.random.default_rng(6)
    fine = torch.from_numpy(rng.standard_normal((2, 24, 64))).to(torch.bfloat16).to(dev)
    coarse = torch.from_numpy(rng.standard_normal((2, 12, 64))).to(torch.bfloat16).to(dev)
    lf = torch.tensor([24, 17], dtype=torch.int32, device=dev)
    out = q([(fine, lf), (coarse, torch.ceil(lf / 2).int())])
    assert out['residual_output'].shape[:2] == (2, 24) and torch.isfinite(out['residual_output'].float()).all()
    for quant, ind, T in zip(out['quantizer_outputs'], out['quantizer_indices'], (12, 24)):
        assert torch.isfinite(quant.float()).all()
        assert tuple(ind.shape) == (2, T, 4) and int(ind.min()) >= 0 and int(ind.max()) < 32
    assert torch.isfinite(out['predictor_diffs']['total_loss'].float())
    for pre in q.preprocessor:
        assert int(pre[3].num_batches_tracked) == 1


@pytest.mark.gpu
def test_one_graphed_bf16_trainer_step_with_norm():
    """the small trainer configuration of the GPU step tests (tests/_parity.py) with ``norm: True``, bf16, the warm-up-phase
    step captured and replayed three times: the BatchNorm buffers are static tensors the replays advance"""
    import random
    import _parity
    from _util import load_npz, t
    from msmctts_amd.synthetic import make_batch
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.hip import lib
    lib._lib, lib._host_pointers_ok = lib.load(), False
    cfg = _parity.small_config()
    cfg.task.autoencoder.quantizer_config.norm = True
    task = build_task(cfg, mode='train')
    missing, unexpected = task.load_state_dict({k: t(v) for k, v in load_npz('small_state.npz').items()}, strict=False)
    assert not unexpected and all('.preprocessor.' in k and '.3.' in k for k in missing), (missing, unexpected)
    for m in task.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    task = task.to('cuda').train()
    stages = [pre[3] for pre in task.autoencoder.quantizer.preprocessor]
    assert len(stages) == 2 and task.autoencoder.quantizer.use_hip
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.model = task
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True)
    tr.use_graphs, tr.amp_dtype, tr.rng = True, torch.bfloat16, random.Random(3)
    batch = make_batch(3, 24, 80, 300, seed=5, device='cuda')
    batch['mel_length_host'] = batch['mel_length'].tolist()
    means = []
    for step in range(3):
        assert tr.replays(step)
        log = tr.train_step(batch, step)
        assert all(np.isfinite(float(v)) for v in log['loss'].values()), log
        assert [int(bn.num_batches_tracked) for bn in stages] == [step + 1] * 2
        means.append([bn.running_mean.clone() for bn in stages])
    assert tr._graphs_warm is not None
    for a, b in zip(means[:-1], means[1:]):
        assert all(not torch.equal(x, y) for x, y in zip(a, b))
