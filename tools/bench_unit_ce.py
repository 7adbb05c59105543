#!/usr/bin/env python
"""Times ``masked_cross_entropy`` (csrc/unit_ce.hip) against the stock operator chain it replaces, on the GPU:

    python tools/bench_unit_ce.py [--out profiles/unit_ce.json] [--reps 20] [--rounds 3]

Chain (the baseline, the 'softmax' branch of ``MultiStageQuantizer.compute_embedding_loss`` before the kernel):
``F.cross_entropy(reduction='none')``, ``masked_fill`` of the padded frames, ``sum``, divide by the sum of the lengths.  Both paths
on identical inputs -- logits [B, T, K] in fp32 and in bf16, labels in [0, K) (the chain cannot take -1), ragged lengths -- forward
only and forward + backward, K = 500 / 2000, N = B T = 6400 / 51 200 (T = 400).  Device events around one call; the paths are
alternated inside a round and every figure is the median of ``--reps`` calls after 5 untimed ones; ``--rounds`` rounds, each
reported, so that the spread between rounds stands next to the difference between paths.  In the same process: the peak of
``torch.cuda.max_memory_allocated`` over one forward + backward of each path (above what is allocated before the call), and a
device-to-device copy that moves as many bytes as the kernels do -- one read of the logits forward; two reads and one write of
them forward + backward.  One untimed pass over all shapes comes first.  Prints a markdown table and one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, reps, warm=5):
    """-> median in microseconds per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'bench_unit_ce.py measures on the GPU'
    from msmctts_amd.hip.unit_ce import masked_cross_entropy
    from msmctts_amd.utils.utils import get_mask_from_lengths
    dev, T = 'cuda', 400

    def run(reps, rounds):
        rows = []
        for dtype in (torch.float32, torch.bfloat16):
            for K in (500, 2000):
                for N in (6400, 51200):
                    B = N // T
                    gen = torch.Generator().manual_seed(K + N)
                    logits = (torch.randn(B, T, K, generator=gen) * 2).to(dev).to(dtype).requires_grad_(True)
                    target = torch.randint(0, K, (B, T), generator=gen).to(dev)
                    lengths = torch.randint(T // 2, T + 1, (B,), generator=gen).to(dev)

                    def chain():
                        loss = F.cross_entropy(logits.view(-1, K), target.view(-1), reduction='none').view(B, T)
                        return loss.masked_fill(get_mask_from_lengths(lengths, T), 0).sum() / lengths.sum()

                    def kernel():
                        return masked_cross_entropy(logits, target, lengths)

                    def fwd(path):
                        def go():
                            with torch.no_grad():
                                return path()
                        return go

                    def fwd_bwd(path):
                        def go():
                            logits.grad = None
                            path().backward()
                        return go

                    a, b = float(fwd(kernel)()), float(fwd(chain)())
                    assert abs(a - b) <= (1e-3 if dtype == torch.float32 else 1e-2) * abs(b), (a, b)
                    nbytes = N * K * logits.element_size()
                    src_f, dst_f = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
                    src_b, dst_b = (torch.empty(3 * nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
                    paths = (('kernel_fwd', fwd(kernel)), ('chain_fwd', fwd(chain)), ('kernel_fwd_bwd', fwd_bwd(kernel)),
                             ('chain_fwd_bwd', fwd_bwd(chain)), ('copy_fwd', lambda: dst_f.copy_(src_f)), ('copy_fwd_bwd', lambda: dst_b.copy_(src_b)))
                    r = {'dtype': str(dtype).split('.')[-1], 'K': K, 'N': N, 'logits_MB': round(nbytes / 1e6, 1)}
                    for name, _ in paths:
                        r[name + '_us'] = []
                    for _ in range(rounds):
                        for name, fn in paths:
                            r[name + '_us'].append(round(timed(fn, reps), 1))
                    logits.grad = None
                    r['kernel_peak_MB'] = round(peak_bytes(fwd_bwd(kernel)) / 1e6, 1)
                    logits.grad = None
                    r['chain_peak_MB'] = round(peak_bytes(fwd_bwd(chain)) / 1e6, 1)
                    logits.grad = None
                    rows.append(r)
        return rows

    run(1, 1)                                   # untimed: every shape once, so that no figure below is a first touch
    rows = run(args.reps, args.rounds)
    cols = ('dtype', 'K', 'N', 'logits_MB', 'kernel_fwd_us', 'chain_fwd_us', 'copy_fwd_us', 'kernel_fwd_bwd_us', 'chain_fwd_bwd_us',
            'copy_fwd_bwd_us', 'kernel_peak_MB', 'chain_peak_MB')
    print('| ' + ' | '.join(cols) + ' |')
    print('|' + '---|' * len(cols))
    for r in rows:
        print('| ' + ' | '.join(' / '.join(str(v) for v in r[c]) if isinstance(r[c], list) else str(r[c]) for c in cols) + ' |')
    print(json.dumps({'unit_ce': rows}))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'unit_ce': rows}, f, indent=1)
    return rows


if __name__ == '__main__':
    main()
