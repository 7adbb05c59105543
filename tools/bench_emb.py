#!/usr/bin/env python
"""Runs ON the GPU box: the QS-TTS synthesiser's train step (EmbVQGANTrainer over MSMCVQGANEmb) and its window path.

Sizes: examples/qs-tts/configs/synthesizer/msmc_vq_gan_hubertch_aishell3.yaml of the reference -- emb 1024, model 256, two
stages, 16 kHz / hop 200, sample_batch_size 16, sample_lengths 12000 (60 frames) -- with the ``hop_lengths`` resolution
discriminators of the CSMSC configuration (the YAML's ``resolutions`` / ``channels`` kwargs exist nowhere in the reference's
code); B = 16, T = 400.

  window    the kernel pair of csrc/window.hip (forward + backward, 2 launches) next to the stock chain it replaces at the
            same sizes ([16, 400, 256] -> 16 windows of 60 frames): torch.stack of slices + transpose + contiguous + cast, and
            its autograd.  Device events around 200 calls each, the two alternated, three rounds, per dtype pair.
  phase0|phase1|phase2
            ms per eager step of one phase (frames only | vocoder + spectral loss | + adversarial terms): a host clock around
            synchronised blocks of steps, three rounds, after warm-up steps (kernel tuning, lazy buffers).

Without an argument every section runs as a child process of its own under its own ``timeout``; the first one that fails or runs
out of time ends the run.  ``--dtype fp32`` times the steps in fp32 (default: bf16 autocast, as bench.py)."""
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]

SECTIONS = (('window', 180), ('phase0', 300), ('phase1', 300), ('phase2', 300))
B, T, EMB, MODEL, HOP, W = 16, 400, 1024, 256, 200, 60


def config():
    from msmctts_amd.configs import csmsc_config
    cfg = csmsc_config(batch_size=B, sample_lengths=W * HOP)
    ae = cfg['task']['autoencoder']
    ae.update(_name='MSMCVQGANEmb', emb_dim=EMB, pitch_dim=0, energy_dim=0, mel_dim=80)
    ae.pop('in_dim')
    ae['decoder_config'].update(upsample_rates=[5, 5, 4, 2], upsample_kernel_sizes=[11, 11, 8, 4])
    cfg['task']['_name'] = 'NASynTTSEmb'
    cfg['task']['discriminator']['mrd_config']['sample_rate'] = 16000
    cfg['trainer'] = dict(_name='EmbVQGANTrainer', grad_clip_thresh=1.0, sample_batch_size=16, sample_lengths=W * HOP,
                          frame_loss_supervised_step=10, stft_loss_supervised_step=20, lambda_vq=1, lambda_pr=0.1,
                          lambda_frame=450, lambda_fm=2, lambda_stft=45)
    cfg['dataset'] = dict(_name='EmbDataset', samplerate=16000, feature=['emb', 'mel', 'wav'], dimension=[EMB, 80, 1],
                          frameshift=[HOP, HOP, 1], padding_value=[0, -4, 0], pre_load=False, segment_length=-1)
    return cfg


def window(iters=200, rounds=3):
    import torch
    from msmctts_amd.hip import window as hipwindow
    dev = torch.device('cuda:0')
    rng = random.Random(1)
    wins = [(i, rng.randrange(T - W)) for i in range(B)]
    table = hipwindow.as_windows(wins, dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    print('window path: x [%d, %d, %d] -> %d windows of %d frames, forward + backward, us per call' % (B, T, MODEL, B, W))
    for xd, od in ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)):
        x = torch.randn(B, T, MODEL, device=dev).to(xd).requires_grad_(True)
        g = torch.randn(B, 1, W, MODEL, device=dev).to(od)

        def kernels():
            hipwindow.window_gather(x, table, W, od).unsqueeze(1).backward(g)

        def stock():
            y = torch.stack([x[i, s:s + W] for i, s in wins], dim=0).transpose(1, 2)           # the model's window ...
            y.transpose(1, 2).unsqueeze(1).contiguous().to(od).backward(g)                      # ... and the generator's intake
        x.grad = None
        kernels()
        a = x.grad.clone()
        x.grad = None
        stock()
        assert torch.equal(a, x.grad), 'the two paths disagree'
        byts = B * W * MODEL * (x.element_size() + 2 * g.element_size()) + B * T * MODEL * x.element_size()
        for rnd in range(rounds):
            for name, fn in (('kernel pair', kernels), ('stock chain', stock)):
                for _ in range(10):
                    x.grad = None
                    fn()
                ev[0].record()
                for _ in range(iters):
                    x.grad = None
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                us = ev[0].elapsed_time(ev[1]) * 1e3 / iters
                print('  %s -> %s  round %d  %s %8.1f us  (%.2f MB moved by the kernel pair)'
                      % (str(xd)[6:], str(od)[6:], rnd, name, us, byts / 1e6), flush=True)


def phase(which, dtype, steps=10, rounds=3, warm=4):
    import torch
    import msmctts_amd  # noqa: F401
    from msmctts_amd.synthetic import make_emb_batch
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    dev = torch.device('cuda:0')
    cfg = Config(config())
    torch.manual_seed(cfg.seed)
    task = build_task(cfg, mode='train')
    tr = build_trainer(cfg, task, num_gpus=1, rank=0)
    tr.optimizer = build_optimizer(tr.model, cfg.optimizer)
    tr.amp_dtype = torch.bfloat16 if dtype == 'bf16' else None
    tr.rng = random.Random(1234)
    tr.model.train()
    batch = make_emb_batch(B, T, EMB, 80, HOP, seed=1234, rank=0, device=dev)
    iteration = {0: 5, 1: 15, 2: 25}[which]
    assert tr._phase(iteration) == which
    for _ in range(warm):
        log = tr.train_step(batch, iteration)
    torch.cuda.synchronize()
    assert all(float(v) == float(v) for v in log['loss'].values()), 'a loss is NaN'
    for rnd in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.train_step(batch, iteration)
        torch.cuda.synchronize()
        print('  phase %d  %s  round %d  %8.2f ms per eager step (%d steps)' % (which, dtype, rnd, (time.perf_counter() - t0) * 1e3 / steps,
                                                                              steps), flush=True)


def main(argv):
    dtype = 'fp32' if '--dtype=fp32' in argv or argv[-2:] == ['--dtype', 'fp32'] else 'bf16'
    names = [a for a in argv if a in dict(SECTIONS)]
    if names:
        import torch
        assert torch.cuda.is_available(), 'tools/bench_emb.py measures on the GPU'
        torch.cuda.set_device(0)
        for name in names:
            window() if name == 'window' else phase(int(name[-1]), dtype)
        return 0
    for name, limit in SECTIONS:
        rc = subprocess.call(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), name, '--dtype', dtype])
        if rc != 0:
            print('section %s ended with status %d: stopping' % (name, rc), flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
