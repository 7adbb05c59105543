#!/usr/bin/env python
"""Times the stage-target step of a predictor step against ``MSMCVQGANEmb`` from stored codes and from frames, on the GPU:

    python tools/bench_code_embed.py [--out profiles/code_embed.json] [--reps 20] [--rounds 3] [--sections stage,gather,step]

Model: emb 1024, ``n_model_size`` 256, ``downsample_scales`` [1, 4], ``n_heads`` 4, ``embedding_dims`` 256, ``embedding_sizes``
512, the FFT-block stacks of the CSMSC configuration, no pitch / energy encoder; eval mode, ``no_grad``.

  stage   B = 16 / 64, T = 400 / 800, fp32 and bf16 targets.  From frames: ``MSMCVQGANEmb.analysis`` on device-resident
          frames (in_linear, both encoder stages, the code search; for bf16 targets a cast of its outputs).  From codes:
          ``analysis_codes`` on device-resident int64 codes (``embed_codes``: one prepared-codebook lookup and one
          ``msmc_code_gather`` launch per stage).  One call per event pair, median and minimum of ``--reps`` windows.
  gather  ``msmc_code_gather`` alone on the finer stage's shape ([B, T, 4] labels -> [B, T, 256]) next to a device-to-device copy
          of the output's bytes: ``--inner`` launches back to back between one pair of events (steady-state time per launch).
  step    a whole eager ``EmbPredictorTrainer`` step (the CSMSC multi-stage predictor, 'mse' + 'triple_sum', B = 16, T = 400) on a
          frames batch and on a code batch: a host clock around synchronised blocks of steps.

Every section repeats ``--rounds`` times after one untimed pass; all rounds are printed, so the spread between them shows.
The upload of the frames (4 KB per frame) is NOT part of any figure: both batch forms are resident on the device.
Prints markdown tables and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import torch  # noqa: E402

EMB, MODEL, HEADS, K, SCALES = 1024, 256, 4, 512, (1, 4)


def timed(fn, reps, warm=3, inner=1):
    """-> (median, minimum) in microseconds per call; ``inner`` calls back to back between one pair of events"""
    for _ in range(warm * inner):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return round(statistics.median(out), 1), round(min(out), 1)


def autoencoder_config():
    from msmctts_amd.configs import csmsc_config
    ae = csmsc_config(downsample_scales=SCALES, n_heads=HEADS, embedding_sizes=K)['task']['autoencoder']
    ae.update(_name='MSMCVQGANEmb', emb_dim=EMB, pitch_dim=0, energy_dim=0, mel_dim=80)
    ae.pop('in_dim')
    ae['decoder_config'].update(upsample_rates=[5, 5, 4, 2], upsample_kernel_sizes=[11, 11, 8, 4])
    return ae


def build_autoencoder(dev):
    from msmctts_amd.networks import find_modules
    torch.manual_seed(1234)
    (_, m), = find_modules({'autoencoder': autoencoder_config()})
    return m.to(dev).eval()


def batches(dev, B, T, seed=1):
    from msmctts_amd import synthetic
    kw = dict(batch_size=B, frames=T, emb_dim=EMB, seed=seed, device=dev)
    return (synthetic.make_text_emb_batch(**kw),
            synthetic.make_text_emb_batch(n_codes=K, downsample_scales=SCALES, n_heads=HEADS, **kw))


def stage(model, dev, reps):
    rows = []
    for B in (16, 64):
        for T in (400, 800):
            fb, _ = batches(dev, B, T)
            emb, length = fb['emb'], fb['emb_length'].int()
            with torch.no_grad():
                qs = model.analysis(emb, length)
            ind, lens = qs['quantizer_indices'], qs['quantizer_lengths']
            for dt in (torch.float32, torch.bfloat16):
                def frames():
                    with torch.no_grad():
                        out = model.analysis(emb, length)['quantizer_outputs']
                        return out if dt == torch.float32 else [o.to(dt) for o in out]

                def codes():
                    with torch.no_grad():
                        return model.quantizer.embed_codes(ind, lens, dt)['quantizer_outputs']
                r = {'B': B, 'T': T, 'out': str(dt)[6:]}
                r['frames_us'], r['frames_min_us'] = timed(frames, reps)
                r['codes_us'], r['codes_min_us'] = timed(codes, reps)
                r['ratio'] = round(r['frames_us'] / r['codes_us'], 1)
                rows.append(r)
    return rows


def gather(model, dev, reps, inner):
    from msmctts_amd.hip import lib
    from msmctts_amd.hip import vq as hipvq
    rows = []
    embed_t, _ = hipvq.vq_prepare(model.quantizer.quantizer[-1]._packed()[0].detach().contiguous(), frames=0)
    d = embed_t.shape[2]
    for B in (16, 64):
        for T in (400, 800):
            _, cb = batches(dev, B, T)
            ind, length = cb['codes_%d' % (len(SCALES) - 1)].contiguous(), cb['codes_length'].int().contiguous()
            for bf16 in (0, 1):
                dt = torch.bfloat16 if bf16 else torch.float32
                out, src = torch.empty(B, T, HEADS * d, dtype=dt, device=dev), torch.randn(B, T, HEADS * d, device=dev).to(dt)

                def kernel():
                    lib.call('msmc_code_gather', lib.ptr(ind), 1, lib.ptr(length), lib.ptr(embed_t), lib.ptr(out), bf16, B, T, HEADS, d, K,
                             lib.stream(out))
                r = {'B': B, 'T': T, 'out': str(dt)[6:]}
                r['gather_us'], r['gather_min_us'] = timed(kernel, reps, inner=inner)
                r['copy_us'], r['copy_min_us'] = timed(lambda: out.copy_(src), reps, inner=inner)
                nbytes = out.numel() * out.element_size()
                r['gather_GBps'] = round((nbytes + ind.numel() * 8) / r['gather_us'] / 1e3, 1)          # written + labels read
                r['copy_GBps'] = round(2 * nbytes / r['copy_us'] / 1e3, 1)                              # read + written
                rows.append(r)
    return rows


def step(model, dev, steps=5, warm=3, B=16, T=400):
    from msmctts_amd.configs import am_config
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    cfg = am_config(batch_size=B)
    cfg['task']['_name'] = 'NASynTTSEmb'
    cfg['trainer']['_name'] = 'EmbPredictorTrainer'
    cfg = Config(cfg)
    torch.manual_seed(cfg.seed)
    task = build_task(cfg, mode='train').to(dev).train()
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True)
    tr.autoencoder = model
    fb, cb = batches(dev, B, T)
    row = {'B': B, 'T': T}
    for name, batch in (('frames', fb), ('codes', cb)):
        for i in range(warm):
            tr.train_step(batch, i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            tr.train_step(batch, warm + i)
        torch.cuda.synchronize()
        row[name + '_ms'] = round((time.perf_counter() - t0) * 1e3 / steps, 2)
    return [row]


def table(title, rows):
    if not rows:
        return
    cols = [c for c in rows[0] if c != 'round']
    print('\n%s' % title)
    print('| round | ' + ' | '.join(cols) + ' |')
    print('|' + '---|' * (len(cols) + 1))
    for r in rows:
        print('| %d | ' % r['round'] + ' | '.join(str(r[c]) for c in cols) + ' |', flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--inner', type=int, default=50, help='launches per timed window of the gather-alone figures')
    ap.add_argument('--sections', default='stage,gather,step')
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = 'cuda'
    model = build_autoencoder(dev)
    result = {}
    for name in args.sections.split(','):
        fn = {'stage': lambda n: stage(model, dev, n), 'gather': lambda n: gather(model, dev, n, args.inner if n > 2 else 2),
              'step': lambda n: step(model, dev, steps=5 if n > 2 else 1, warm=3 if n > 2 else 1)}[name]
        fn(2)                                      # untimed: every shape once, so that no figure below is a first touch
        rows = []
        for rnd in range(args.rounds):
            rows += [dict(r, round=rnd) for r in fn(args.reps)]
        result[name] = rows
        table(name, rows)
    print(json.dumps({'code_embed': result}))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'code_embed': result}, f, indent=1)
    return result


if __name__ == '__main__':
    main()
