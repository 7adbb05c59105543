#!/usr/bin/env python
"""Times the decoder-input stage of ``KMeansVQGANEmb`` from stored units against the frame path, on the GPU:

    python tools/bench_unit_embed.py [--out profiles/unit_embed.json] [--reps 30]

Frame path (the baseline): the wide nearest-centroid search of ``KMeansQuantizer`` on centroid frames [B, T, d] followed by
``in_linear`` over the frames.  Unit path: ``F.linear(centers, W, b)`` [K, n] and ``unit_embed`` on the labels.  Both forward only
and forward + backward (a random projection of the stage's output, gradients of ``in_linear``).  K = 500 / 2000, d = 768 / 1024,
n = 256, N = B T = 6400 / 51 200 (T = 400).  The embed kernels are also timed alone, next to a device-to-device copy of the
output's bytes on the same card: ``--inner`` launches back to back between one pair of HIP events, so the window holds
hundreds of microseconds of work and the figure is the steady-state time per launch (enqueue hidden behind the queue), not the
time of a single cold launch.  The stage figures are one run per event pair.  Every figure is the median of ``--reps`` timed
windows after 5 untimed ones; the minimum is printed next to it.  The search kernel the frame path ran is recorded per shape
(``msmc_vq_last_kernel``).  One untimed pass over all shapes comes first.  Prints a markdown table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, reps, warm=5, inner=1):
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
    return statistics.median(out), min(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=50, help='launches per timed window of the kernels-alone figures')
    args = ap.parse_args(argv)
    from msmctts_amd.hip import lib, units
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansQuantizer
    dev, n, T = 'cuda', 256, 400
    tmp = tempfile.mkdtemp()

    def run(reps, inner_launches):
        rows = []
        for K in (500, 2000):
            for d in (768, 1024):
                rng = np.random.default_rng(K + d)
                centers = rng.standard_normal((K, d)).astype(np.float32)
                path = os.path.join(tmp, 'c_%d_%d.npy' % (K, d))
                np.save(path, centers)
                quant = KMeansQuantizer(path).to(dev).eval()
                lin = torch.nn.Linear(d, n).to(dev)
                cd = torch.from_numpy(centers).to(dev)
                for N in (6400, 51200):
                    B = N // T
                    ind = torch.from_numpy(rng.integers(0, K, (B, T))).to(dev)
                    length = torch.full((B,), T, dtype=torch.int64, device=dev)
                    emb = cd[ind].contiguous()
                    w = torch.randn(B, T, n, device=dev)

                    def frame_fwd():
                        with torch.no_grad():
                            return lin(quant([(emb, length)])['quantizer_outputs'][-1])

                    def unit_fwd():
                        with torch.no_grad():
                            return units.unit_embed(ind, length, F.linear(cd, lin.weight, lin.bias))

                    def frame_fb():
                        lin.zero_grad(set_to_none=True)
                        (lin(quant([(emb, length)])['quantizer_outputs'][-1]) * w).sum().backward()

                    def unit_fb():
                        lin.zero_grad(set_to_none=True)
                        (units.unit_embed(ind, length, F.linear(cd, lin.weight, lin.bias)) * w).sum().backward()

                    assert float((frame_fwd() - unit_fwd()).abs().max()) <= 1e-3 * float(frame_fwd().abs().max())
                    table = F.linear(cd, lin.weight, lin.bias).detach().contiguous()
                    out = torch.empty(B, T, n, device=dev)
                    gtable = torch.empty(K, n, device=dev)
                    ws = lib.workspace(int(lib.get().msmc_units_embed_workspace(N, n, K)), dev)
                    src = torch.randn(B, T, n, device=dev)

                    def k_fwd():
                        lib.call('msmc_units_embed_fwd', lib.ptr(ind), lib.ptr(length), lib.ptr(table), None, lib.ptr(out), B, T, n, K,
                                 lib.stream(out))

                    def k_bwd():
                        lib.call('msmc_units_embed_bwd', lib.ptr(w), lib.ptr(ind), lib.ptr(length), lib.ptr(gtable), None, lib.ptr(ws),
                                 ws.numel() * 4, B, T, n, K, lib.stream(out))

                    frame_fwd()
                    r = {'K': K, 'd': d, 'N': N, 'frame_search_kernel': lib.get().msmc_vq_last_kernel().decode()}
                    for name, fn in (('frame_fwd', frame_fwd), ('unit_fwd', unit_fwd), ('frame_fwd_bwd', frame_fb), ('unit_fwd_bwd', unit_fb),
                                     ('embed_fwd_kernel', k_fwd), ('embed_bwd_kernels', k_bwd), ('copy', lambda: out.copy_(src))):
                        inner = inner_launches if name in ('embed_fwd_kernel', 'embed_bwd_kernels', 'copy') else 1
                        r[name + '_us'], r[name + '_min_us'] = (round(v, 1) for v in timed(fn, reps, inner=inner))
                    nbytes = N * n * 4
                    r['embed_fwd_GBps'] = round((nbytes + 8 * N) / r['embed_fwd_kernel_us'] / 1e3, 1)        # written + labels read
                    r['embed_bwd_GBps'] = round((nbytes + 8 * N) / r['embed_bwd_kernels_us'] / 1e3, 1)       # gradient read + labels
                    r['copy_GBps'] = round(2 * nbytes / r['copy_us'] / 1e3, 1)                                # read + written
                    rows.append(r)
        return rows

    run(2, 2)                                   # untimed: every shape once, so that no figure below is a first touch
    rows = run(args.reps, args.inner)
    cols = ('K', 'd', 'N', 'frame_search_kernel', 'frame_fwd_us', 'unit_fwd_us', 'frame_fwd_bwd_us', 'unit_fwd_bwd_us', 'embed_fwd_kernel_us',
            'embed_bwd_kernels_us', 'copy_us', 'embed_fwd_GBps', 'embed_bwd_GBps', 'copy_GBps')
    print('| ' + ' | '.join(cols) + ' |')
    print('|' + '---|' * len(cols))
    for r in rows:
        print('| ' + ' | '.join(str(r[c]) for c in cols) + ' |')
    print(json.dumps({'unit_embed': rows}))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'unit_embed': rows}, f, indent=1)
    return rows


if __name__ == '__main__':
    main()
