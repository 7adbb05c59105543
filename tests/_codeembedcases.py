"""Shared cases of the stored-code path of the main model: csrc/code_embed.hip (msmc_code_gather), its host side
(msmctts_amd/hip/code_embed.py ``code_gather``), ``MultiHeadQuantize.embed_code``, ``MultiStageQuantizer.embed_codes``,
``MSMCVQGANEmb.analysis_codes`` / ``synthesis_codes``, ``EmbPredictorTrainer``, ``NASynTTSEmb.predict``, tools/extract_codes.py and
``synthetic.make_text_emb_batch``.  tests/test_code_embed_emu.py runs them on the kernel interpreter, tests/test_gpu_code_embed.py
on the GPU.

Kernel reference: ``restated`` -- the definition in numpy (the indexed row, the two zero rules, ``Tensor.to`` for bf16) --
compared BIT FOR BIT: the kernel copies and rounds once, nothing is summed.

Model bound: ``analysis`` returns the search kernel's straight-through value o = fl(x + fl(q - x)) (csrc/vq_common.inc), x the
quantiser's input, q the code row.  fl(q - x) is within 2^-24 (|q| + |x|) of q - x, the sum within 2^-24 |o| of its operands' sum
and |o| <= |q| up to that same error: |o - q| <= 2^-24 (|x| + 2 |q|) to first order.  The test allows 2^-23 (|x| + 2 |q|) per
element, a factor of 2 of margin; ``analysis_codes`` itself must equal the ``embed_code`` rows bit for bit.

Trainer reference: the parent chain -- ``PredictorTrainer._forward_backward``'s loss and backward code -- on targets built with
stock ``embed_code`` indexing, every dropout probability 0.  The parent chain is run twice from the same state first: where its two
runs agree bit for bit (they do, on the interpreter and on the GPU: see ``check_trainer_step``'s printed line) the new path must
equal it bit for bit; otherwise the largest difference of those two runs would be allowed.
"""
import ctypes
import io
import os

import numpy as np
import torch

from _embcases import _raises

E_SHAPE = -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- (a) the kernel, directly -----------------------------------------------------------------------------------------------------------
# name: (B, T, H, d, K) -- the path it exercises
CASES = {
    'smallest': (1, 1, 1, 4, 1),
    'vector several heads': (2, 5, 4, 16, 16),
    'shipped wide head': (3, 7, 2, 128, 512),
    'scalar d6': (2, 9, 3, 6, 10),
    'single head T33': (2, 33, 1, 8, 100),
    'bf16 half vector d12': (2, 5, 2, 12, 7),           # d % 4 == 0, d % 8 != 0: fp32 16-byte pieces, bf16 8-byte stores
}
SMALL = list(CASES)
GPU_ONLY = {'strided grid': (8, 2100, 4, 64, 512)}     # more than 8 x 256 blocks of 2048 pieces: workgroups stride over the blocks


def _round_bf16(a):
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy()


def problem(shape, variant, i64):
    """embed_t, ind, lengths.  variant 0: lengths hold T and 0 (B >= 2); variant 1: partial lengths.  Labels outside [0, K) -- -1,
    K and a large positive value -- sit at every fifth position, in valid and in padded rows alike."""
    B, T, H, d, K = shape
    rng = np.random.default_rng(977 + 31 * variant + sum(shape))
    embed_t = rng.standard_normal((H, K, d)).astype(np.float32)
    ind = rng.integers(0, K, (B, T, H)).astype(np.int64)
    big = (1 << 40) + 3 if i64 else (1 << 31) - 1
    flat = ind.reshape(-1)
    for j in range(1, flat.size, 5):
        flat[j] = (-1, K, big, -(1 << 31))[(j // 5) % 4]
    if variant == 0:
        lengths = rng.integers(1, T + 1, (B,))
        lengths[0] = T
        if B > 1:
            lengths[1] = 0
    else:
        lengths = np.maximum(rng.integers(0, T + 1, (B,)) - 1, 0)
        lengths[-1] = -3 if B > 1 else max(T - 1, 0)          # (a negative length: the utterance is all zeros)
    return embed_t, ind.astype(np.int64 if i64 else np.int32), lengths.astype(np.int32)


def restated(embed_t, ind, lengths, bf16):
    """out[b, t, h d + c] = embed_t[h, ind[b, t, h], c] where t < lengths[b] and 0 <= ind < K, +0 elsewhere; bf16: Tensor.to"""
    H, K, d = embed_t.shape
    B, T, _ = ind.shape
    ind = ind.astype(np.int64)
    ok = (ind >= 0) & (ind < K) & (np.arange(T)[None, :, None] < lengths.astype(np.int64)[:, None, None])
    rows = embed_t[np.arange(H)[None, None, :], np.where(ok, ind, 0)]                # [B, T, H, d]
    out = np.where(ok[..., None], rows, np.float32(0)).astype(np.float32).reshape(B, T, H * d)
    return _round_bf16(out) if bf16 else out.view(np.int32)


def _at(dev, values, offset, dtype):
    """a device copy of ``values`` that starts ``offset`` elements into a 16-byte aligned allocation"""
    buf = torch.zeros(values.size + 16, dtype=dtype).to(dev)
    view = buf[offset:offset + values.size].view(values.shape)
    view.copy_(torch.from_numpy(values).to(dtype))
    return view


def run_kernel(dev, embed_t, ind, lengths, bf16, shape=None, offset=0, flags=None):
    """msmc_code_gather on an output pre-filled with NaN -> (rc, the output's bits)"""
    from msmctts_amd.hip import lib
    H, K, d = embed_t.shape
    B, T = ind.shape[:2]
    B, T, H, d, K = (B, T, H, d, K) if shape is None else shape
    e = _at(dev, embed_t, offset, torch.float32)
    i = torch.from_numpy(ind).to(dev)
    ln = torch.from_numpy(lengths).to(dev)
    out = torch.full((ind.shape[0], ind.shape[1], embed_t.shape[0] * embed_t.shape[2]), float('nan'),
                     dtype=torch.bfloat16 if bf16 else torch.float32).to(dev)
    i64, obf = (int(ind.dtype == np.int64), int(bf16)) if flags is None else flags
    rc = lib.get().msmc_code_gather(lib.ptr(i), i64, lib.ptr(ln), lib.ptr(e), lib.ptr(out), obf, B, T, H, d, K, lib.stream(out))
    return rc, out.cpu().view(torch.int16 if bf16 else torch.int32).numpy()


def check_case(dev, name, bf16, i64):
    shape = dict(CASES, **GPU_ONLY)[name]
    for variant in (0, 1):
        embed_t, ind, lengths = problem(shape, variant, i64)
        rc, got = run_kernel(dev, embed_t, ind, lengths, bf16)
        assert rc == 0, (name, rc)
        want = restated(embed_t, ind, lengths, bf16)
        assert same_bits(got, want), '%s variant %d: %d of %d elements differ' % (name, variant, int((got != want).sum()), want.size)
    if shape == CASES['smallest']:
        embed_t, ind, lengths = problem(shape, 0, i64)
        for lab, ln in ((-1, 1), (1, 1), (0, 0)):
            rc, got = run_kernel(dev, embed_t, np.full_like(ind, lab), np.array([ln], dtype=np.int32), bf16)
            assert rc == 0 and not got.any(), (lab, ln, got)


def check_misaligned(dev):
    """a codebook off its 16-byte boundary takes the element path: the same bits"""
    shape = CASES['vector several heads']
    for bf16 in (False, True):
        embed_t, ind, lengths = problem(shape, 0, True)
        rc, got = run_kernel(dev, embed_t, ind, lengths, bf16, offset=1)
        assert rc == 0 and same_bits(got, restated(embed_t, ind, lengths, bf16))


def check_strided_grid(dev):
    """interpreter: 3 CUs -> at most 24 workgroups; 25 blocks of 2048 pieces make them stride"""
    shape = (4, 200, 4, 64, 32)
    embed_t, ind, lengths = problem(shape, 1, False)
    lengths[0] = 200
    rc, got = run_kernel(dev, embed_t, ind, lengths, False)
    assert rc == 0 and same_bits(got, restated(embed_t, ind, lengths, False))


def check_refusals(dev):
    """MSMC_E_SHAPE for each refused argument, the output untouched"""
    shape = CASES['vector several heads']
    embed_t, ind, lengths = problem(shape, 0, True)
    for bf16 in (False, True):
        nan = run_kernel(dev, embed_t, ind, lengths, bf16, shape=(0,) + shape[1:])[1]
        for pos in range(5):
            for bad in (0, -1):
                s = list(shape)
                s[pos] = bad
                rc, got = run_kernel(dev, embed_t, ind, lengths, bf16, shape=tuple(s))
                assert rc == E_SHAPE and same_bits(got, nan), (s, rc)
        for flags in ((2, int(bf16)), (1, 2), (-1, int(bf16)), (1, -1)):
            rc, got = run_kernel(dev, embed_t, ind, lengths, bf16, flags=flags)
            assert rc == E_SHAPE and same_bits(got, nan), flags
        assert np.isnan(torch.from_numpy(nan).view(torch.bfloat16 if bf16 else torch.float32).float().numpy()).all()


def check_host_layer(dev):
    """``code_gather``: both label types, both outputs, a [B, T] single head, the stock chain's bits, the argument checks"""
    from msmctts_amd.hip import code_embed
    for name in ('vector several heads', 'scalar d6', 'single head T33'):
        for i64 in (False, True):
            embed_t, ind, lengths = problem(CASES[name], 1, i64)
            e, i, ln = torch.from_numpy(embed_t).to(dev), torch.from_numpy(ind).to(dev), torch.from_numpy(lengths).to(dev)
            assert code_embed.usable(i, e)
            for dt, view in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
                got = code_embed.code_gather(i, ln, e, dt)
                assert got.dtype == dt and not got.requires_grad
                want = restated(embed_t, ind, lengths, dt == torch.bfloat16)
                assert same_bits(got.cpu().view(view).numpy(), want), (name, i64, dt)
                stock = code_embed.code_gather_stock(i, ln, e, dt)
                assert same_bits(stock.cpu().view(view).numpy(), want), (name, i64, dt)
            if embed_t.shape[0] == 1:
                assert torch.equal(code_embed.code_gather(i[..., 0], ln.long(), e), code_embed.code_gather(i, ln, e))
    with _raises(ValueError, 'ind: expected'):
        code_embed.code_gather(i[..., :0], ln, e)
    with _raises(ValueError, 'lengths'):
        code_embed.code_gather(i, ln[:1], e)
    with _raises(TypeError, 'integer'):
        code_embed.code_gather(i.float(), ln, e)
    with _raises(TypeError, 'fp32 / bf16'):
        code_embed.code_gather(i, ln, e, torch.float16)
    with _raises(RuntimeError, 'msmc_code_gather failed with code -2'):
        code_embed.code_gather(i[:, :0], ln, e)
    assert not code_embed.usable(i.float(), e) and not code_embed.usable(i, e.double())
    if dev != 'cpu':                                # host tensors on the product build: the stock chain, the same values
        assert not code_embed.usable(i.cpu(), e.cpu())
        assert torch.equal(code_embed.code_gather(i.cpu(), ln.cpu(), e.cpu()), code_embed.code_gather(i, ln, e).cpu())


# ---- (b) model ----------------------------------------------------------------------------------------------------------------------------
# The tiny model: n_model_size 64, downsample_scales [1, 2], 16 codes per head, heads of 32 channels, B = 2, T = 7.  The quantiser's
# post-processor concatenates the residual (n_model_size wide) with the quantised frames and is built 2 x embedding_dims wide
# (reference msmc_vqgan.py:129-136), so a quantiser of more than one stage needs embedding_dims == n_model_size: embedding_dims is
# 64 here -- two heads of 32 channels, one head of 64.
EMB, MODEL, DIMS, MEL, B, T, LENGTHS = 24, 64, 64, 24, 2, 7, (7, 4)
VOCODER = dict(upsample_rates=[5, 4, 2], upsample_kernel_sizes=[11, 8, 4], upsample_initial_channel=32, resblock_kernel_sizes=[3, 7],
               resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]])


def model_config(n_heads=2, norm=False, global_encoder=False):
    fft = dict(max_seq_len=64, n_layers=1, n_head=2, d_k=8, d_v=8, d_inner=64, fft_conv1d_kernel=3, fft_conv1d_padding=1,
               dropout=0.0, attn_dropout=0.0, fused_layernorm=False)
    cfg = {'_name': 'MSMCVQGANEmb', 'emb_dim': EMB, 'pitch_dim': 0, 'energy_dim': 0, 'n_model_size': MODEL,
           'encoder_config': dict(downsample_scales=[1, 2], **fft),
           'quantizer_config': dict(embedding_sizes=16, embedding_dims=DIMS, n_heads=n_heads,
                                    prior_config=dict(kernel_size=5, dilation_rate=1, n_layers=1), norm=norm, dropout=0.0),
           'frame_decoder_config': dict(fft), 'pred_mel': True, 'mel_dim': MEL, 'decoder_config': dict(VOCODER)}
    if global_encoder:
        cfg['global_encoder_config'] = {'_name': 'ECAPA_TDNN'}
    return cfg


def build_model(dev, seed=51, **kw):
    from msmctts_amd.networks import find_modules
    torch.manual_seed(seed)
    (_, m), = find_modules({'autoencoder': model_config(**kw)})
    return m.to(dev).eval()


def frames(dev, seed=52):
    gen = torch.Generator().manual_seed(seed)
    length = torch.tensor(LENGTHS, dtype=torch.int64)
    emb = torch.where(torch.arange(T)[None, :, None] < length[:, None, None], torch.randn(B, T, EMB, generator=gen), torch.zeros(()))
    return emb.to(dev), length.to(dev)


def check_model(dev, n_heads=2, norm=False):
    m = build_model(dev, n_heads=n_heads, norm=norm)
    emb, length = frames(dev)
    seen = []
    hooks = [q.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().float().clone())) for q in m.quantizer.quantizer]
    with torch.no_grad():
        qs = m.analysis(emb, length.int())
    for h in hooks:
        h.remove()
    assert len(seen) == 2
    before = int(m.quantizer.quantizer[0]._packed()[0]._version)
    with torch.no_grad():
        qc = m.analysis_codes(qs['quantizer_indices'], qs['quantizer_lengths'])
    assert set(qc) == {'quantizer_outputs', 'quantizer_indices', 'quantizer_lengths'}
    for i in range(2):
        ind, ln = qs['quantizer_indices'][i], qs['quantizer_lengths'][i]
        assert tuple(ind.shape) == ((B, (T, 4)[1 - i]) if n_heads == 1 else (B, (T, 4)[1 - i], n_heads))
        assert torch.equal(qc['quantizer_indices'][i], ind) and torch.equal(qc['quantizer_lengths'][i], ln)
        q = m.quantizer.quantizer[i]
        rows = q.embed_code(ind)                                                   # [B, T_i, DIMS], stock indexing
        valid = (torch.arange(ind.shape[1], device=ln.device)[None, :] < ln[:, None])[..., None]
        got, ana, x = qc['quantizer_outputs'][i], qs['quantizer_outputs'][i].float(), seen[i]
        assert got.dtype == torch.float32 and got.shape == rows.shape
        assert torch.equal(got, torch.where(valid, rows, torch.zeros((), device=rows.device))), 'stage %d: not the embed_code rows' % i
        bound = 2.0 ** -23 * (x.abs() + 2 * rows.abs())
        over = ((ana - got).abs() > bound) & valid
        print('stage %d: max |analysis - codes| %.3e, max bound %.3e' % (i, float(((ana - got).abs() * valid).max()), float(bound.max())))
        assert not bool(over.any()), 'stage %d: %d elements beyond 2^-23 (|x| + 2 |q|)' % (i, int(over.sum()))
        bf = m.quantizer.embed_codes(qs['quantizer_indices'], qs['quantizer_lengths'], torch.bfloat16)['quantizer_outputs'][i]
        assert torch.equal(bf, got.to(torch.bfloat16))
    # the prepared codebook is kept in eval mode ...
    cache = m.quantizer._code_cache
    kept = [cache[i][1] for i in range(2)]
    m.analysis_codes(qs['quantizer_indices'], qs['quantizer_lengths'])
    assert all(cache[i][1] is kept[i] for i in range(2)) and int(m.quantizer.quantizer[0]._packed()[0]._version) == before
    # ... and dropped when the codebook changes in place
    m.quantizer.quantizer[1]._packed()[0].mul_(2.0)
    qd = m.analysis_codes(qs['quantizer_indices'], qs['quantizer_lengths'])
    assert cache[1][1] is not kept[1] and cache[0][1] is kept[0]
    assert torch.equal(qd['quantizer_outputs'][1], qc['quantizer_outputs'][1] * 2.0)
    m.train()
    with _raises(RuntimeError, 'eval mode'):
        m.analysis_codes(qs['quantizer_indices'], qs['quantizer_lengths'])
    m.eval()
    with _raises(ValueError, 'stages'):
        m.analysis_codes(qs['quantizer_indices'][:1], qs['quantizer_lengths'][:1])


def check_multi_head_embed_code():
    """CPU, no kernels: the new method against per-head indexing"""
    from msmctts_amd.networks.vqgantts.modules import MultiHeadQuantize
    torch.manual_seed(3)
    q = MultiHeadQuantize(12, 5, 3)
    ind = torch.randint(0, 5, (2, 4, 3))
    got = q.embed_code(ind)
    assert tuple(got.shape) == (2, 4, 12)
    for h in range(3):
        assert torch.equal(got[..., 4 * h:4 * h + 4], q.quantizers[h].embed.t()[ind[..., h]])


def check_synthesis_codes(dev):
    m = build_model(dev, global_encoder=True)
    emb, length = frames(dev)
    ref = torch.randn(B, 9, MEL, generator=torch.Generator().manual_seed(53)).to(dev)
    with torch.no_grad():
        qs = m.analysis(emb, length.int())
        qc = m.analysis_codes(qs['quantizer_indices'], qs['quantizer_lengths'])
        want = m.synthesis(qc['quantizer_outputs'], qs['quantizer_lengths'], ref)
        got = m.synthesis_codes(qs['quantizer_indices'], qs['quantizer_lengths'], ref)
    assert tuple(got.shape) == (B, T * 40, 1) and torch.equal(got, want)
    with _raises(AssertionError):
        m.synthesis_codes(qs['quantizer_indices'], qs['quantizer_lengths'])
    from msmctts_amd.networks.vqgantts.msmc_vqgan import MSMCVQGAN
    assert callable(MSMCVQGAN.analysis_codes)


# ---- (c) trainer --------------------------------------------------------------------------------------------------------------------------
def predictor_config():
    from _util import small_predictor_cfg
    pc = small_predictor_cfg()
    pc.update(n_pred_size=DIMS, n_pred_scale=[2, 1])
    return pc


def build_trainer(dev, name='EmbPredictorTrainer', autoencoder=None, methods=('mse', 'triple_sum'), global_encoder=False):
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer as make
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    trainer = dict(_name=name, grad_clip_thresh=10.0, training_methods=list(methods), loss_weights=[[1.0] * len(methods)] * 2,
                   lambda_dur=1.0)
    cfg = Config({'id': 'small_emb_predictor',
                  'task': {'_name': 'NASynTTSEmb', '_mode': 'train_predictor', 'predictor': predictor_config()},
                  'trainer': trainer,
                  'optimizer': {'_default': dict(_name='Adam', learning_rate=2e-4, betas=[0.9, 0.98], eps=1e-9, weight_decay=0)},
                  'dataset': dict(samplerate=16000, feature=['codes_0', 'codes_1'], frameshift=[80, 40])})
    torch.manual_seed(7800)
    task = build_task(cfg, mode='train').to(dev).train()
    for mod in task.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, 'dropout') and isinstance(getattr(mod, 'dropout'), float):
            mod.dropout = 0.0
    tr = make(cfg, task, num_gpus=0, rank=0)
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True) if dev != 'cpu' else build_optimizer(task, cfg.optimizer)
    tr.autoencoder = build_model(dev, global_encoder=global_encoder) if autoencoder is None else autoencoder
    return task, tr


def code_batch(dev, tr):
    """both forms of ``make_text_emb_batch`` on the same lengths, text and durations: (frames batch, code batch)"""
    from msmctts_amd import synthetic
    kw = dict(batch_size=B, frames=T, emb_dim=EMB, n_symbols=(20, 5, 2), phonemes=(3, 5), seed=7801, device=dev)
    fb = synthetic.make_text_emb_batch(**kw)
    cb = synthetic.make_text_emb_batch(n_codes=16, downsample_scales=(1, 2), n_heads=2, **kw)
    assert torch.equal(fb['emb_length'], cb['codes_length']) and torch.equal(fb['dur'], cb['dur'])
    return fb, cb


def parent_chain(tr, batch, qs):
    """``PredictorTrainer._forward_backward`` behind its ``analysis`` call, on the targets ``qs``"""
    from msmctts_amd.hip import norm as hipnorm
    from msmctts_amd.trainers.msmctts_trainer import _one_like
    feed = {k: batch[k] for k in ('text', 'text_length', 'dur')}
    feed['feat'] = [f.float() for f in qs['quantizer_outputs']]
    feed['feat_length'] = qs['quantizer_lengths']
    hipnorm.advance_seed(feed['feat'][0].device)
    with tr._amp():
        output = tr.model.predictor(**feed)
    output['feat'] = [f.float() for f in output['feat']]
    losses = {'total_loss': 0}
    emb = tr.autoencoder.compute_embedding_loss(output['feat'], output['feat_length'], qs, methods=tr.training_methods,
                                                loss_weights=tr.loss_weights)
    losses['total_loss'] = losses['total_loss'] + emb.pop('total_loss')
    losses.update(emb)
    dur = tr.dur_loss(output, feed)
    losses['total_loss'] = losses['total_loss'] + dur.pop('total_loss')
    losses.update(dur)
    tr.optimizer.zero_grad(['predictor'])
    losses['total_loss'].backward(gradient=_one_like(losses['total_loss']))
    return losses


def _grads(task):
    return {k: p.grad.detach().clone() for k, p in task.predictor.named_parameters() if p.grad is not None}


def stock_targets(tr, cb):
    """the code batch's quantiser states with stock ``embed_code`` indexing (zeros on padded rows and for labels outside [0, K))"""
    ae = tr.autoencoder
    lengths = tr.stage_lengths(cb['codes_length'])
    outs = []
    for i, ln in enumerate(lengths):
        ind = cb['codes_%d' % i]
        rows = ae.quantizer.quantizer[i].embed_code(ind.clamp(0, 15))
        ok = ((ind >= 0) & (ind < 16)).repeat_interleave(DIMS // 2, dim=-1) & (torch.arange(ind.shape[1], device=ind.device)[None, :, None] < ln[:, None, None])
        outs.append(torch.where(ok, rows, torch.zeros((), device=rows.device)))
    return {'quantizer_outputs': tuple(outs), 'quantizer_indices': tuple(cb['codes_%d' % i] for i in range(2)), 'quantizer_lengths': lengths}


def check_trainer_step(dev):
    task, tr = build_trainer(dev)
    assert type(tr).__name__ == 'EmbPredictorTrainer' and tr.training_methods == ['mse', 'triple_sum']
    fb, cb = code_batch(dev, tr)
    lengths = tr.stage_lengths(cb['codes_length'])
    assert [l.tolist() for l in lengths] == [[4, (cb['codes_length_host'][1] + 1) // 2], cb['codes_length_host']]
    assert all(l.dtype == torch.int32 for l in lengths)
    with torch.no_grad():
        qs = stock_targets(tr, cb)
    tr.autoencoder.eval()
    a = parent_chain(tr, cb, qs)
    ga = _grads(task)
    b = parent_chain(tr, cb, qs)
    gb = _grads(task)
    slack = max(float((ga[k] - gb[k]).abs().max()) for k in ga)
    lslack = max(abs(float(a[k].detach()) - float(b[k].detach())) for k in a)
    print('parent chain, two runs from the same state: max gradient difference %.3e, max loss difference %.3e' % (slack, lslack))
    got = tr._forward_backward(cb)
    gg = _grads(task)
    keys = {'total_loss', 'embed_loss_mse_0', 'embed_loss_mse_1', 'embed_loss_triple_sum_0', 'embed_loss_triple_sum_1', 'dur_loss'}
    assert set(got) == keys == set(a), sorted(got)
    for k in keys:
        if lslack == 0.0:
            assert same_bits(got[k].detach().cpu().numpy(), a[k].detach().cpu().numpy()), (k, float(got[k]), float(a[k]))
        else:
            assert abs(float(got[k]) - float(a[k])) <= lslack, (k, float(got[k]), float(a[k]))
    assert set(gg) == set(ga) and len(gg) > 10
    for k in ga:
        if slack == 0.0:
            assert torch.equal(gg[k], ga[k]), k
        else:
            assert float((gg[k] - ga[k]).abs().max()) <= slack, k
    # int16 / int32 codes as the extraction tool stores them, and a [B, T, 1]-free batch without the host list: the same step
    small = {k: (v.to(torch.int16) if k.startswith('codes_') and k[6:].isdigit() else v) for k, v in cb.items() if k != 'codes_length_host'}
    again = tr._forward_backward(small)
    assert all(same_bits(again[k].detach().cpu().numpy(), got[k].detach().cpu().numpy()) for k in keys)
    # a whole step: clipped, the predictor moves, the autoencoder does not
    before = {k: v.detach().clone() for k, v in task.state_dict().items()}
    frozen = {k: v.detach().clone() for k, v in tr.autoencoder.state_dict().items()}
    log = tr.train_step(cb, 0)['loss']
    assert set(log) == keys | {'grad_norm'} and all(np.isfinite(float(v)) for v in log.values())
    after = task.state_dict()
    moved = {k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k])}
    assert any(k.startswith('predictor.decoders.1.2.') for k in moved) and any(k.startswith('predictor.word_emb') for k in moved)
    assert all(torch.equal(v, tr.autoencoder.state_dict()[k]) for k, v in frozen.items()), 'the autoencoder is frozen'
    return slack


def check_trainer_frames(dev):
    """a frames batch: the same keys, finite, and the losses of the parent chain on ``analysis``'s targets; frames win over codes"""
    task, tr = build_trainer(dev)
    fb, cb = code_batch(dev, tr)
    tr.autoencoder.eval()
    with torch.no_grad():
        qs = tr.autoencoder.analysis(fb['emb'], fb['emb_length'].int())
    want = parent_chain(tr, fb, qs)
    got = tr._forward_backward(fb)
    both = tr._forward_backward(dict(cb, **fb))
    assert set(got) == set(want) == {'total_loss', 'embed_loss_mse_0', 'embed_loss_mse_1', 'embed_loss_triple_sum_0',
                                      'embed_loss_triple_sum_1', 'dur_loss'}
    for k in want:
        assert np.isfinite(float(got[k]))
        assert same_bits(got[k].detach().cpu().numpy(), want[k].detach().cpu().numpy()), (k, float(got[k]), float(want[k]))
        assert same_bits(both[k].detach().cpu().numpy(), got[k].detach().cpu().numpy()), k
    # pitch / energy reach analysis
    seen = {}
    real = tr.autoencoder.analysis
    tr.autoencoder.analysis = lambda emb, n, pitch=None, energy=None: (seen.update(pitch=pitch, energy=energy), real(emb, n))[1]
    tr._forward_backward(dict(fb, pitch=fb['emb'][..., :1], energy=fb['emb'][..., 1:2]))
    del tr.autoencoder.analysis
    assert seen['pitch'] is not None and tuple(seen['energy'].shape) == (B, T, 1)


def check_trainer_refusals(dev):
    task, tr = build_trainer(dev)
    fb, cb = code_batch(dev, tr)
    assert tr.use_graphs is False
    tr.use_graphs = False
    with _raises(NotImplementedError, 'hipGraph'):
        tr.use_graphs = True
    few = {k: v for k, v in cb.items() if k != 'codes_1'}
    with _raises(ValueError, 'stages'):
        tr.train_step(few, 0)
    with _raises(ValueError, 'stages'):
        tr.train_step(dict(cb, codes_2=cb['codes_1']), 0)
    wide = dict(cb, codes_0=torch.cat((cb['codes_0'], cb['codes_0'][..., :1]), dim=-1))
    with _raises(ValueError, 'heads'):
        tr.train_step(wide, 0)
    with _raises(ValueError, 'heads'):
        tr.train_step(dict(cb, codes_1=cb['codes_1'][..., 0]), 0)
    with _raises(KeyError, 'codes_'):
        tr.train_step({k: cb[k] for k in ('text', 'text_length', 'dur')}, 0)

    class NoCodes(torch.nn.Module):
        def compute_embedding_loss(self, *a, **k):
            raise AssertionError('not reached')
    tr.autoencoder = NoCodes()
    with _raises(TypeError, 'analysis_codes'):
        tr.train_step(cb, 0)


def check_trainer_names(dev):
    from msmctts_amd.trainers.emb_predictor_trainer import EmbPredictorTrainer, NASynEmbFSTrainer
    from msmctts_amd.trainers.msmctts_trainer import PredictorTrainer
    assert NASynEmbFSTrainer is EmbPredictorTrainer and issubclass(EmbPredictorTrainer, PredictorTrainer)
    for name in ('EmbPredictorTrainer', 'NASynEmbFSTrainer'):
        _, tr = build_trainer(dev, name=name, methods=('mse',))
        assert type(tr) is EmbPredictorTrainer and tr.grad_clip_thresh == 10.0 and tr.dur_loss.lambda_dur == 1.0


def check_text_emb_batch():
    """CPU, no kernels: both forms of ``make_text_emb_batch``"""
    from msmctts_amd import synthetic
    kw = dict(batch_size=3, frames=9, emb_dim=6, n_symbols=(20, 5, 2), phonemes=(3, 5), seed=5)
    f = synthetic.make_text_emb_batch(tracks=True, **kw)
    assert set(f) == {'text', 'text_length', 'dur', 'emb', 'emb_length', 'pitch', 'energy'}
    assert tuple(f['emb'].shape) == (3, 9, 6) and int(f['emb_length'].max()) == 9 and torch.equal(f['dur'].sum(-1), f['emb_length'])
    valid = torch.arange(9)[None, :] < f['emb_length'][:, None]
    assert not bool(f['emb'][~valid].any()) and not bool(f['pitch'][~valid].any()) and tuple(f['energy'].shape) == (3, 9, 1)
    assert torch.equal(synthetic.make_text_emb_batch(**kw)['emb'], f['emb'])
    c = synthetic.make_text_emb_batch(n_codes=11, downsample_scales=(1, 4), n_heads=3, **kw)
    assert set(c) == {'text', 'text_length', 'dur', 'codes_0', 'codes_1', 'codes_length', 'codes_length_host'}
    assert torch.equal(c['codes_length'], f['emb_length']) and c['codes_length_host'] == f['emb_length'].tolist()
    assert tuple(c['codes_1'].shape) == (3, 9, 3) and tuple(c['codes_0'].shape) == (3, 3, 3) and c['codes_0'].dtype == torch.int64
    coarse = torch.ceil(c['codes_length'] / 4).long()
    for codes, ln in ((c['codes_1'], c['codes_length']), (c['codes_0'], coarse)):
        ok = (torch.arange(codes.shape[1])[None, :] < ln[:, None])
        assert bool((codes[~ok] == -1).all()) and int(codes[ok].min()) >= 0 and int(codes[ok].max()) < 11


# ---- (d) task and tool ----------------------------------------------------------------------------------------------------------------------
def check_task_predict(dev):
    """text -> waveform through an autoencoder with a global encoder: ``ref`` reaches ``synthesis``"""
    task, tr = build_trainer(dev, global_encoder=True)
    task.autoencoder = tr.autoencoder
    task.eval()
    fb, _ = code_batch(dev, tr)
    ref = torch.randn(B, 9, MEL, generator=torch.Generator().manual_seed(54)).to(dev)
    feed = {k: fb[k] for k in ('text', 'text_length', 'dur')}
    with torch.no_grad():
        out = task.predict(dict(feed, ref=ref, emb=fb['emb'], emb_length=fb['emb_length']))
        assert len(out['wav']) == B and [int(w.shape[0]) for w in out['wav']] == [n * 40 for n in LENGTHS]
        assert all(bool(torch.isfinite(w).all()) for w in out['wav']) and tuple(out['embedding'].shape) == (B, T, DIMS)
        with _raises(AssertionError):
            task.predict(feed)
        # without a global encoder: the parent's behaviour
        task.autoencoder = build_model(dev)
        plain = task.predict(feed)
        assert len(plain['wav']) == B and [int(w.shape[0]) for w in plain['wav']] == [n * 40 for n in LENGTHS]


def check_extract_codes(dev, tmpdir):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import extract_codes
    finally:
        sys.path.pop(0)
    from msmctts_amd.hip import units
    m = build_model(dev)
    tmpdir = str(tmpdir)
    os.makedirs(os.path.join(tmpdir, 'feats'))
    rng = np.random.default_rng(55)
    ids, feats = [('utt%d' % i, 'spk') for i in range(3)], []
    for (name, _), n in zip(ids, (7, 4, 5)):
        feats.append(rng.standard_normal((n, EMB)).astype(np.float32))
        np.save(os.path.join(tmpdir, 'feats', name + '.npy'), feats[-1])
    out = io.StringIO()
    counts = extract_codes.extract(m, ids, os.path.join(tmpdir, 'feats', '{0}.npy'), os.path.join(tmpdir, 'out'), jobs=2, out=out)
    lines = out.getvalue().strip().split('\n')
    assert len(lines) == 4 and sorted(counts) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    total = {k: np.zeros(16, dtype=np.int64) for k in counts}
    for group in (ids[:2], ids[2:]):                          # the tool's own batches: zero-padded to the longest
        n = [feats[ids.index(a)].shape[0] for a in group]
        emb = torch.zeros(len(group), max(n), EMB)
        for b, a in enumerate(group):
            emb[b, :n[b]] = torch.from_numpy(feats[ids.index(a)])
        with torch.no_grad():
            qs = m.analysis(emb.to(dev), torch.tensor(n, dtype=torch.int32).to(dev))
        for i in range(2):
            ind, ln = qs['quantizer_indices'][i].cpu().numpy(), qs['quantizer_lengths'][i].cpu().tolist()
            for b, a in enumerate(group):
                stored = np.load(os.path.join(tmpdir, 'out', 'codes_%d' % i, a[0] + '.npy'))
                assert stored.dtype == np.int16 and stored.shape == (ln[b], 2), (stored.dtype, stored.shape)
                assert ln[b] == (n[b] if i == 1 else (n[b] + 1) // 2)
                assert np.array_equal(stored, ind[b, :ln[b]])
                for h in range(2):
                    total[(i, h)] += np.bincount(stored[:, h], minlength=16)
    for line, key in zip(lines, sorted(counts)):
        assert np.array_equal(counts[key], total[key])
        used, entropy = units.usage_summary(total[key])
        assert line == '%d %d %s %s' % (key[0], key[1], used, entropy), (line, used, entropy)


def check_dataset_reads_codes(tmpdir):
    """CPU, no kernels: the dataset classes read ``codes_<i>`` files as integer features padded with -1"""
    from msmctts_amd.datasets.tts_dataset import TTSDataset
    tmpdir = str(tmpdir)
    rng = np.random.default_rng(2)
    rows_text, rows_dur, stored = [], [], {}
    for sub in ('codes_0', 'codes_1'):
        os.makedirs(os.path.join(tmpdir, sub))
    for uid, n_ph, n in (('a', 4, 26), ('b', 6, 40)):
        stored[uid] = [rng.integers(0, 16, (n // 2, 2)).astype(np.int16), rng.integers(0, 16, (n, 2)).astype(np.int16)]
        for i in range(2):
            np.save(os.path.join(tmpdir, 'codes_%d' % i, uid + '.npy'), stored[uid][i])
        cuts = np.sort(rng.choice(np.arange(1, n), n_ph - 1, replace=False))
        rows_text.append('%s|%s' % (uid, ' '.join(str(v) for v in rng.integers(1, 20, n_ph))))
        rows_dur.append('%s|%s' % (uid, ' '.join(str(v) for v in np.diff(np.concatenate(([0], cuts, [n]))))))
    for name, rows in (('id.list', ['a', 'b']), ('text.list', rows_text), ('dur.list', rows_dur)):
        with open(os.path.join(tmpdir, name), 'w') as f:
            f.write('\n'.join(rows) + '\n')
    ds = TTSDataset(id_list=os.path.join(tmpdir, 'id.list'), feature=['text', 'dur', 'codes_0', 'codes_1'], samplerate=16000,
                    dimension=[1, 1, 2, 2], frameshift=[None, None, 640, 320],
                    feature_path=[os.path.join(tmpdir, 'text.list'), os.path.join(tmpdir, 'dur.list'),
                                  os.path.join(tmpdir, 'codes_0', '{}.npy'), os.path.join(tmpdir, 'codes_1', '{}.npy')],
                    padding_value=[0, 0, -1, -1], training=False)
    batch = ds.collate_fn([ds[0], ds[1]])
    assert batch['text_length'].tolist() == [6, 4]                                  # sorted by text length: b, a
    assert tuple(batch['codes_1'].shape) == (2, 40, 2) and tuple(batch['codes_0'].shape) == (2, 20, 2)
    assert batch['codes_1'].dtype == torch.int16 and batch['codes_length'].tolist() == [40, 26]
    assert batch['dur'].sum(1).tolist() == [40, 26]
    assert np.array_equal(batch['codes_1'][1, :26].numpy(), stored['a'][1]) and np.array_equal(batch['codes_0'][0].numpy(), stored['b'][0])
    assert bool((batch['codes_1'][1, 26:] == -1).all()) and bool((batch['codes_0'][1, 13:] == -1).all())


# ---- (e) feature presence -----------------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    with open(os.path.join(ROOT, 'include', 'msmc_hip.h')) as f:
        header = f.read()
    assert 'msmc_code_gather(' in header and 'msmc_code_gather' in lib.exported_symbols()
    assert isinstance(lib.get().msmc_code_gather, ctypes._CFuncPtr)
    assert os.path.isfile(os.path.join(ROOT, 'msmc-tts_amd', 'csrc', 'code_embed.hip'))
    from msmctts_amd.hip.code_embed import code_gather, usable  # noqa: F401
    from msmctts_amd.networks.vqgantts.msmc_vqgan import MSMCVQGAN, MultiStageQuantizer
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import MSMCVQGANEmb
    from msmctts_amd.synthetic import make_text_emb_batch  # noqa: F401
    assert callable(MultiStageQuantizer.embed_codes) and callable(MSMCVQGAN.analysis_codes)
    assert all(callable(getattr(MSMCVQGANEmb, name)) for name in ('analysis_codes', 'synthesis_codes'))
    from msmctts_amd.trainers import emb_predictor_trainer
    from msmctts_amd.utils.utils import module_search
    for name in ('EmbPredictorTrainer', 'NASynEmbFSTrainer'):
        cls = module_search(name, os.path.dirname(emb_predictor_trainer.__file__), 'msmctts_amd.trainers')
        assert cls is emb_predictor_trainer.EmbPredictorTrainer
    assert all(os.path.isfile(os.path.join(ROOT, 'tools', f)) for f in ('extract_codes.py', 'bench_code_embed.py'))
