"""Shared cases of ``EmbVQGANTrainer`` (trainers/emb_vqgan_trainer.py): tests/test_emb_trainer_emu.py runs them on the kernel
interpreter, tests/test_gpu_emb_trainer.py on the GPU.

Reference of every comparison: ``reference_step`` below, the reference's train_step (msmctts/trainers/emb_vqgan_trainer.py:29-172)
restated on stock torch operators -- window sampling from the python RNG, windows by slicing and ``torch.stack``, masked MSE /
L1 / MSE loss terms, two separate discriminator passes per step, ``clip_grad_norm_`` and ``torch.optim.AdamW`` -- applied to a
``copy.deepcopy`` of the same task with the same RNG seed.  Both sides run the same network kernels, so they differ in the
window path (hip/window.py's ``window_gather`` against slice + stack) and in the loss arithmetic (the fused loss kernels, the
single D([fake; real]) pass).

Bar: the project's fp32 bar (tests/_attn32cases.py FP32_BAR / check_block_stack): max |a - b| <= 1e-3 x max |b| per tensor, for
every entry of the loss dictionary and every parameter gradient (read from ``.grad`` after the step; both sides clip in place).

Sizes: the small model of the train-step cases of tests/test_product_emu.py (tests/_util.py small_task_cfg) at the smallest
widths the attention (head 64) and ECAPA kernels take: n_model_size 64, mel_dim 80; B = 3, T = 24, lengths (24, 17, 5) with
frame_lengths = 8 (the last utterance is shorter than a window), two quantiser stages, dropout 0, sample_batch_size = 2.

Gradients that are identically zero.  Three biases of the ECAPA encoder sit in front of an operation that is invariant to
them: ``pooling.linear2.bias`` (a constant over time in front of the softmax over time), ``bn1.bias`` and ``linear.bias`` (a
constant over the batch in front of ``bn2``, whose batch mean removes it).  Their gradient is a sum over frames / utterances
that cancels exactly; what either side holds is the rounding residue of that sum (about 1e-10 here), and a residue has no
magnitude of its own to divide by.  Such a bias's gradient is the same sum as its layer's weight gradient with the input
replaced by ones, so the bar is taken against that tensor: both residues must be within 1e-3 x max |weight gradient of the same
layer| (the reference's) of zero, the exact value.
"""
import copy
import random

import torch
import torch.nn.functional as F

FP32_BAR = 1e-3
HOP, T, LENGTHS, EMB_DIM, MEL_DIM, MODEL = 300, 24, (24, 17, 5), 32, 80, 64
TRAINER = dict(_name='EmbVQGANTrainer', grad_clip_thresh=1.0, sample_batch_size=2, sample_lengths=2400,
               frame_loss_supervised_step=2, stft_loss_supervised_step=4, lambda_vq=1, lambda_pr=0.1, lambda_frame=450,
               lambda_fm=2, lambda_stft=45)
PHASE_ITERATION = {0: 1, 1: 3, 2: 6}
ZERO_GRADS = ('autoencoder.global_encoder.pooling.linear2.bias', 'autoencoder.global_encoder.bn1.bias',
              'autoencoder.global_encoder.linear.bias')
OPT = dict(_name='AdamW', learning_rate=2e-4, betas=[0.8, 0.99], eps=1e-8, weight_decay=0.0)


def config(global_encoder, trainer=None):
    from msmctts_amd.utils.config import Config
    fft = dict(max_seq_len=64, n_layers=1, n_head=2, d_k=64, d_v=64, d_inner=64, fft_conv1d_kernel=3, fft_conv1d_padding=1,
               dropout=0.0, attn_dropout=0.0, fused_layernorm=False)
    ae = {'_name': 'MSMCVQGANEmb', 'emb_dim': EMB_DIM, 'pitch_dim': 0, 'energy_dim': 0, 'n_model_size': MODEL,
          'encoder_config': dict(downsample_scales=[1, 4], **fft),
          'quantizer_config': dict(embedding_sizes=16, embedding_dims=MODEL, n_heads=4,
                                   prior_config=dict(kernel_size=5, dilation_rate=1, n_layers=1), norm=False, dropout=0.0),
          'frame_decoder_config': dict(fft), 'pred_mel': True, 'mel_dim': MEL_DIM,
          'decoder_config': dict(upsample_rates=[6, 5, 5, 2], upsample_kernel_sizes=[12, 11, 11, 4], upsample_initial_channel=32,
                                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])}
    if global_encoder:
        ae['global_encoder_config'] = {'_name': 'ECAPA_TDNN'}
    disc = {'_name': 'UnivNetDiscriminator',
            'mrd_config': dict(hop_lengths=[15, 60], hidden_channels=[32, 32], domain='double', mel_scale=True, sample_rate=24000),
            'mpd_config': dict(periods=[2, 3], channels=4, max_channels=16)}
    return Config({'id': 'small_emb', 'task': {'_name': 'NASynTTSEmb', 'autoencoder': ae, 'discriminator': disc},
                   'trainer': dict(TRAINER if trainer is None else trainer), 'optimizer': {'_default': dict(OPT)},
                   'dataset': dict(samplerate=24000, feature=['emb', 'mel', 'wav'], frameshift=[HOP, HOP, 1])})


def build(dev, global_encoder, seed=21):
    from msmctts_amd.tasks import build_task
    cfg = config(global_encoder)
    torch.manual_seed(seed)
    task = build_task(cfg, mode='train')
    for m in task.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return cfg, task.to(dev).train()


def make_batch(dev, seed=22):
    gen = torch.Generator().manual_seed(seed)
    B = len(LENGTHS)
    lengths = torch.tensor(LENGTHS, dtype=torch.int64)
    valid = torch.arange(T)[None, :, None] < lengths[:, None, None]
    emb = torch.where(valid, torch.randn(B, T, EMB_DIM, generator=gen), torch.zeros(()))
    mel = torch.where(valid, torch.randn(B, T, MEL_DIM, generator=gen), torch.full((), -4.0))
    wav = torch.rand(B, T * HOP, 1, generator=gen) * 2 - 1
    wav = torch.where(torch.arange(T * HOP)[None, :, None] < (lengths * HOP)[:, None, None], wav, torch.zeros(()))
    batch = {'emb': emb, 'emb_length': lengths, 'mel': mel, 'wav': wav, 'wav_length': lengths * HOP}
    batch = {k: v.to(dev) for k, v in batch.items()}
    batch['emb_length_host'] = list(LENGTHS)
    return batch


def _pad_mask(lengths, width):
    return torch.arange(width, device=lengths.device)[None, :] >= lengths[:, None]


def reference_windows(rng, lengths, sample_batch_size, frame_lengths):
    """:41-53"""
    seq_indices = range(len(lengths))
    if sample_batch_size > 0:
        seq_indices = list(range(len(lengths)))
        rng.shuffle(seq_indices)
        seq_indices = seq_indices[:sample_batch_size]
        seq_indices.sort()
    windows = []
    for i in seq_indices:
        start = rng.randrange(max(1, lengths[i] - frame_lengths))
        windows.append((i, start, start + frame_lengths))
    return windows


def reference_step(task, tr, opts, batch, iteration, rng):
    """:29-172 on stock operators; ``tr`` supplies only hyper-parameters and the (parameter-free) spectral criterion.
    -> (losses, windows or None, output dictionary)"""
    from msmctts_amd.hip import window as hipwindow
    losses = {}
    emb, emb_length, wav, mel = batch['emb'], batch['emb_length'], batch['wav'], batch['mel']
    mel_length = emb_length
    windows = None
    if iteration > tr.frame_loss_supervised_step:
        windows = reference_windows(rng, emb_length.tolist(), tr.sample_batch_size, tr.frame_lengths)
        target = torch.stack([wav.squeeze(-1)[i, s * tr.frameshift:e * tr.frameshift] for i, s, e in windows], dim=0)
    usable = hipwindow.usable
    try:
        hipwindow.usable = lambda x: False                  # the reference's windows: slices and torch.stack
        output = task.autoencoder(emb, emb_length, batch.get('pitch'), batch.get('energy'), mel=mel, window=windows)
    finally:
        hipwindow.usable = usable
    g_loss = 0
    # VQ loss (reference msmctts_trainer.py:45-71)
    vq = {'vq_loss': 0}
    for i, terms in enumerate(output['encoder_diffs']):
        length = output['encoder_lengths'][i]
        for j, term in enumerate(terms if isinstance(terms, (tuple, list)) else [terms]):
            term = term.float().masked_fill(_pad_mask(length, term.shape[1]).unsqueeze(-1), 0)
            term = term.sum() / length.sum() / term.shape[2]
            vq['latent_loss_%d_%d' % (i, j)] = term
            vq['vq_loss'] = vq['vq_loss'] + tr.vq_criterion.lambda_vq * term
    dd = dict(output['decoder_diffs'])
    vq['vq_loss'] = vq['vq_loss'] + tr.vq_criterion.lambda_pr * dd.pop('total_loss')
    vq.update(dd)
    losses.update(vq)
    g_loss = g_loss + vq['vq_loss']
    if 'mel_outputs' in output:
        ml = F.mse_loss(mel, output['mel_outputs'].float(), reduction='none')
        ml = ml.masked_fill(_pad_mask(mel_length, ml.shape[1]).unsqueeze(-1), 0)
        ml = ml.sum() / mel_length.sum() / ml.shape[2]
        losses['frame_loss'] = ml
        g_loss = g_loss + tr.lambda_frame * ml
    if 'decoder_outputs' in output:
        predict = output['decoder_outputs'].squeeze(-1).float()
        stl = tr.stft_criterion(predict, target)
        if isinstance(stl, dict):
            losses.update(stl)
            stl = sum(stl.values())
        losses['stft_loss'] = stl
        g_loss = g_loss + tr.lambda_stft * stl
    if iteration > tr.stft_loss_supervised_step:
        disc = task.discriminator
        fake_scores, _ = disc(predict.detach())
        real_scores, _ = disc(target)
        d_real = sum(F.mse_loss(s.float(), torch.ones_like(s.float())) for s in real_scores)
        d_fake = sum(F.mse_loss(s.float(), torch.zeros_like(s.float())) for s in fake_scores)
        d_loss = d_real + d_fake
        losses['d_loss_real'], losses['d_loss_fake'], losses['d_loss'] = d_real, d_fake, d_loss
        opts['discriminator'].zero_grad()
        d_loss.backward()
        d_grads = {n: p.grad.detach().clone() for n, p in disc.named_parameters() if p.grad is not None}
        opts['discriminator'].step()
        fake_scores, fake_feats = disc(predict)
        with torch.no_grad():               # (the reference also back-propagates into D here and throws those gradients away)
            real_scores, real_feats = disc(target)
        adv = sum(F.mse_loss(s.float(), torch.ones_like(s.float())) for s in fake_scores)
        fm = sum(F.l1_loss(a.float(), b.float()) for fa, fb in zip(fake_feats, real_feats) for a, b in zip(fa, fb))
        adv = adv + fm * (tr.lambda_fm if tr.lambda_fm != 'auto' else (g_loss / fm).detach())
        g_loss = g_loss + adv
        losses['fm_loss'], losses['adv_loss'], losses['g_loss'] = fm, adv, g_loss
    else:
        d_grads = None
    opts['autoencoder'].zero_grad()
    g_loss.backward()
    torch.nn.utils.clip_grad_norm_(task.autoencoder.parameters(), tr.grad_clip_thresh)
    opts['autoencoder'].step()
    return {k: float(v.detach()) for k, v in losses.items()}, windows, output, d_grads


def _trainer(cfg, task, seed):
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.model = task
    tr.optimizer = build_optimizer(task, cfg.optimizer)
    tr.rng = random.Random(seed)
    return tr


def check_phase(dev, phase, global_encoder):
    """one step of ``phase`` against the restatement: loss dictionary, parameter gradients, windows, window_gather calls"""
    from msmctts_amd.hip import window as hipwindow
    cfg, task = build(dev, global_encoder)
    ref = copy.deepcopy(task)
    iteration = PHASE_ITERATION[phase]
    tr = _trainer(cfg, task, seed=100 + phase)
    assert tr._phase(iteration) == phase
    batch = make_batch(dev)
    calls, outputs = [], []
    real = hipwindow.window_gather
    ae_forward = task.autoencoder.forward
    # the discriminator's gradients of the D step are overwritten by nothing afterwards (the generator step freezes D), but the
    # optimizer step must not have moved them: AdamW leaves .grad alone
    try:
        hipwindow.window_gather = lambda x, *a, **k: (calls.append(tuple(x.shape)), real(x, *a, **k))[1]
        task.autoencoder.forward = lambda *a, **k: (outputs.append(ae_forward(*a, **k)), outputs[-1])[1]
        task.zero_grad()
        log = tr.train_step(batch, iteration)
    finally:
        hipwindow.window_gather = real
        del task.autoencoder.forward
    opts = {name: torch.optim.AdamW(getattr(ref, name).parameters(), lr=OPT['learning_rate'], betas=tuple(OPT['betas']),
                                    eps=OPT['eps'], weight_decay=OPT['weight_decay']) for name in ('autoencoder', 'discriminator')}
    want, windows, ref_out, d_grads = reference_step(ref, tr, opts, batch, iteration, random.Random(100 + phase))
    # windows and the window path
    if phase == 0:
        assert windows is None and tr.last_windows is None and not calls
        assert 'decoder_outputs' not in outputs[0] and 'mel_outputs' in outputs[0]
    else:
        assert tr.last_windows == [(i, s) for i, s, _ in windows], (tr.last_windows, windows)
        assert len(windows) == TRAINER['sample_batch_size'] < len(LENGTHS)
        frames = [c for c in calls if c[-1] == MODEL]
        assert frames == [(len(LENGTHS), T, MODEL)], 'window_gather must cut the vocoder frames once per step: %s' % calls
        assert len(calls) == 2, 'one call for the frames, one for the target waveform: %s' % calls
        assert tuple(outputs[0]['decoder_outputs'].shape) == (len(windows), tr.frame_lengths * HOP, 1)
    # losses
    assert set(log['loss']) == set(want), (sorted(log['loss']), sorted(want))
    expect = {'vq_loss', 'latent_loss_0_0', 'latent_loss_1_0', 'embed_loss_mse_1', 'frame_loss'}
    expect |= {'stft_loss'} if phase > 0 else set()
    expect |= {'d_loss_real', 'd_loss_fake', 'd_loss', 'fm_loss', 'adv_loss', 'g_loss'} if phase == 2 else set()
    assert set(want) == expect, sorted(want)
    failed = []
    for k, v in want.items():
        got = float(log['loss'][k])
        print('emb trainer phase %d ge=%d loss %-18s %.6e  reference %.6e' % (phase, global_encoder, k, got, v))
        if not abs(got - v) <= FP32_BAR * abs(v):
            failed.append('%s: %.6e vs %.6e' % (k, got, v))
    # gradients
    pairs = [('autoencoder.' + n, p.grad, dict(ref.autoencoder.named_parameters())[n].grad)
             for n, p in task.autoencoder.named_parameters()]
    if phase == 2:
        pairs += [('discriminator.' + n, p.grad, d_grads.get(n)) for n, p in task.discriminator.named_parameters()]
    worst, checked = 0.0, 0
    ref_grads = {name: b for name, _, b in pairs}
    for name, a, b in pairs:
        if a is None and b is None:                 # (the vocoder in phase 0)
            continue
        assert a is not None and b is not None, name
        if name in ZERO_GRADS:                      # (module docstring: exactly zero, bar against the layer's weight gradient)
            scale = float(ref_grads[name[:-len('bias')] + 'weight'].abs().max())
            assert scale > 0, name
            for side, g in (('trainer', a), ('reference', b)):
                if not float(g.abs().max()) <= FP32_BAR * scale:
                    failed.append('%s (%s): residue %.3e, weight-gradient scale %.3e' % (name, side, float(g.abs().max()), scale))
            checked += 1
            continue
        err, mag = float((a.double().cpu() - b.double().cpu()).abs().max()), float(b.abs().max())
        checked += 1
        if mag > 0:
            worst = max(worst, err / mag)
        if not err <= FP32_BAR * mag:
            failed.append('%s: max abs err %.3e, scale %.3e' % (name, err, mag))
    print('emb trainer phase %d ge=%d: worst gradient err / scale %.3e over %d tensors' % (phase, global_encoder, worst, checked))
    assert checked > 40 and (phase == 0 or any(n.startswith('autoencoder.decoder.') and a is not None for n, a, _ in pairs))
    assert not failed, failed


class _raises(object):
    def __init__(self, exc, text=''):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc) and self.text in str(val), (tp, val)
        return True


def check_construction(dev):
    """what the parent commit lacks, and the constructor's refusals"""
    from msmctts_amd import synthetic
    from msmctts_amd.datasets import build_dataset  # noqa: F401
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.emb_vqgan_trainer import EmbVQGANTrainer
    from msmctts_amd.utils.utils import module_search
    cfg, task = build(dev, False)
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    assert type(tr) is EmbVQGANTrainer and type(task).__name__ == 'NASynTTSEmb'
    assert (tr.sample_batch_size, tr.frame_loss_supervised_step, tr.stft_loss_supervised_step, tr.lambda_frame) == (2, 2, 4, 450)
    assert tr.frame_lengths == 8 and tr.frameshift == HOP
    assert [tr._phase(i) for i in (0, 2, 3, 4, 5)] == [0, 0, 1, 1, 2]
    import os
    import msmctts_amd.datasets as ds
    assert module_search('EmbDataset', os.path.dirname(ds.__file__), 'msmctts_amd.datasets').__name__ == 'EmbDataset'
    b = synthetic.make_emb_batch(batch_size=3, frames=12, emb_dim=16, mel_dim=8, hop=10, seed=3, rank=0, device=dev)
    assert set(b) == {'emb', 'emb_length', 'mel', 'wav', 'wav_length', 'emb_length_host'}
    assert tuple(b['emb'].shape) == (3, 12, 16) and tuple(b['mel'].shape) == (3, 12, 8) and tuple(b['wav'].shape) == (3, 120, 1)
    assert b['emb_length_host'] == b['emb_length'].tolist() and b['emb_length_host'][0] == 12
    assert b['emb_length_host'] == sorted(b['emb_length_host'], reverse=True)
    assert torch.equal(b['wav_length'], b['emb_length'] * 10)
    with _raises(ValueError, 'stft_loss_supervised_step'):
        build_trainer(config(False, dict(TRAINER, frame_loss_supervised_step=5, stft_loss_supervised_step=4)), task, num_gpus=0)
    with _raises(NotImplementedError, 'hipGraph'):
        tr.use_graphs = True
    assert tr.use_graphs is False
    task.prosody_estimator = torch.nn.Linear(2, 2)
    try:
        with _raises(NotImplementedError, 'prosody'):
            build_trainer(cfg, task, num_gpus=0)
    finally:
        del task.prosody_estimator


def check_model_window_forms(dev):
    """MSMCVQGANEmb.forward: the (utterance, start) table with ``window_frames`` and the reference's triples give the values of
    the slice / stack chain (forward and input gradient, bit for bit: all three only copy frames into the same vocoder)"""
    from msmctts_amd.hip import window as hipwindow
    _, task = build(dev, False)
    m = task.autoencoder
    batch = make_batch(dev)
    triples = [(0, 3, 11), (2, 0, 8)]
    table = torch.tensor([(0, 3), (2, 0)], dtype=torch.int32).to(dev)

    def run(window, frames=None, stock=False):
        usable = hipwindow.usable
        torch.manual_seed(5)
        e = batch['emb'].clone().requires_grad_(True)
        try:
            if stock:
                hipwindow.usable = lambda x: False
            o = m(e, batch['emb_length'], mel=batch['mel'], window=window, window_frames=frames)
        finally:
            hipwindow.usable = usable
        o['decoder_outputs'].pow(2).sum().backward()
        return o['decoder_outputs'].detach().cpu(), e.grad.cpu()
    m.eval()                                                   # (no codebook update between the three passes)
    want = run(triples, stock=True)
    for got in (run(triples), run(table, 8)):
        assert torch.equal(got[0], want[0]) and bool((got[1] == want[1]).all())
    with _raises(TypeError, 'window_frames'):
        m(batch['emb'], batch['emb_length'], mel=batch['mel'], window=triples, window_frames=8)


def check_dataset_collation():
    """EmbDataset.collate_fn: sorted by decreasing emb length, every feature padded with its padding value, one length each"""
    import numpy as np
    from msmctts_amd.datasets.emb_dataset import EmbDataset
    ds = EmbDataset.__new__(EmbDataset)
    ds.padding_value, ds.frameshift = {'emb': 0, 'mel': -4, 'wav': 0}, {'emb': 4, 'mel': 4, 'wav': 1}
    rng = np.random.default_rng(0)
    items = [{'emb': rng.standard_normal((n, 6)).astype(np.float32), 'mel': rng.standard_normal((n, 8)).astype(np.float32),
              'wav': rng.standard_normal((4 * n, 1)).astype(np.float32)} for n in (3, 7, 5)]
    out = ds.collate_fn(items)
    assert set(out) == {'emb', 'emb_length', 'mel', 'mel_length', 'wav', 'wav_length'}
    assert out['emb_length'].tolist() == [7, 5, 3] == out['mel_length'].tolist() and out['wav_length'].tolist() == [28, 20, 12]
    assert tuple(out['emb'].shape) == (3, 7, 6) and tuple(out['mel'].shape) == (3, 7, 8) and tuple(out['wav'].shape) == (3, 28, 1)
    for row, src in enumerate((1, 2, 0)):
        n = items[src]['emb'].shape[0]
        assert torch.equal(out['emb'][row, :n], torch.from_numpy(items[src]['emb'])) and bool((out['emb'][row, n:] == 0).all())
        assert torch.equal(out['mel'][row, :n], torch.from_numpy(items[src]['mel'])) and bool((out['mel'][row, n:] == -4).all())
        assert torch.equal(out['wav'][row, :4 * n], torch.from_numpy(items[src]['wav'])) and bool((out['wav'][row, 4 * n:] == 0).all())
