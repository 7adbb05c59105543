"""Shared cases of the wide nearest-centroid search (csrc/vq_wide.inc, msmc_vq_search_wide), its routing from hip/vq.py and the
quantiser modules, ``KMeansQuantizer`` / ``KMeansVQGANEmb`` (networks/vqgantts/msmc_vqgan_emb.py) and their training by
``EmbVQGANTrainer``: tests/test_kmeans_emu.py runs them on the kernel interpreter, tests/test_gpu_kmeans.py on the GPU.

Kernel reference: the distance ``(|x|^2 - 2 x.e_k) + |e_k|^2`` in float64 with the gap rule of tests/_vqstreamcases.py
(``reference64``): the fp32 chain is within ``4 d 2^-24 (|x| + max|e|)^2`` of it per distance, so a frame whose float64 gap
between the best and the second-best centroid exceeds that bound must have the float64 index; at most 2 % of the frames
(``MAX_LEFT_OUT``, asserted on the reference alone, before the kernel runs) may be undecided.  quant / diff given the index are
exact fp32 expressions (``_vqstreamcases.exact_outputs``) and must match bit for bit.

Inputs.  N(0, 1) frames against N(0, 1) centroids leave 4-5 % of the frames undecided at d = 1024 (the distances concentrate
while the bound grows with d), so only a quarter of the frames are N(0, 1); the others lie between two centroids,
``e_a + t (e_b - e_a) + 0.1 N(0, 1)`` with a != b random and t uniform in [0.25, 0.48]: nearest to a, with b as a competitor
at a gap of 55-100 against a bound of about 1 -- a dropped d-slice or a wrong norm flips the decision.  d = 2048 takes one
eighth of N(0, 1) frames.

The kernel has three instantiations (WC = 1 / 2 / 4 waves sharing a 16-frame tile, chosen from N); every kernel case runs each
of them through the tests' switch ``msmc_vq_wide_set_split`` as well as the launcher's own choice.

Model reference: tests/golden/small_kmeans.npz, written by tests/golden/make_golden_kmeans.py from the reference's own
``KMeansVQGANEmb``; tolerances of ``_parity.close`` as ``_parity.check_emb_autoencoder`` uses them for ``MSMCVQGANEmb`` against
small_emb.npz.
"""
import contextlib
import ctypes
import functools
import os
import pickle
import random

import numpy as np
import torch

import _vqstreamcases as vqs
from _vqstreamcases import E_SHAPE, MAX_LEFT_OUT, exact_outputs, last_kernel, same_bits

WIDE = 'vq_search_wide_kernel'
SPLITS = (0, 1, 2, 4)

# ---- (a) wide shapes against float64 ----------------------------------------------------------------------------------------
WIDE_SHAPES = ((1024, 100), (768, 500), (1024, 1000), (1040, 17), (272, 24), (64, 1), (2048, 40))     # d, K
WIDE_N = 256
SMALL_N = (1, 17, 37)
SMALL_N_SHAPE = 4                   # (272, 24)
EMU_SHAPES = (0, 3, 4, 5)           # the interpreter runs the smaller ones


class KMeansModel(object):
    """what the tests pickle as the k-means model: an object with ``cluster_centers_`` [K, d], as scikit-learn's"""

    def __init__(self, centers):
        self.cluster_centers_ = np.asarray(centers, dtype=np.float32)


@contextlib.contextmanager
def forced_split(wc):
    from msmctts_amd.hip import lib
    lib.get().msmc_vq_wide_set_split(int(wc))
    try:
        yield
    finally:
        lib.get().msmc_vq_wide_set_split(0)


@functools.lru_cache(maxsize=None)
def problem(d, K, N, seed):
    """seeded centroids [1, d, K] and the frame mix of the module docstring [N, d] (host tensors, computed once, never modified)"""
    gen = torch.Generator().manual_seed(seed)
    embed = torch.randn(1, d, K, generator=gen)
    rows = embed[0].t()
    nr = N if K == 1 else N // (8 if d >= 2048 else 4)
    x = torch.randn(N, d, generator=gen)
    if nr < N:
        a = torch.randint(0, K, (N - nr,), generator=gen)
        b = (a + 1 + torch.randint(0, K - 1, (N - nr,), generator=gen)) % K
        t = 0.25 + 0.23 * torch.rand(N - nr, 1, generator=gen)
        x[nr:] = rows[a] + t * (rows[b] - rows[a]) + 0.1 * x[nr:]
    return x.contiguous(), embed


def reference64(x, embed):
    """``_vqstreamcases.reference64`` for one head on given tensors -> (index [N], decided [N]); K = 1: index 0, every frame decided"""
    N, d = x.shape
    K = embed.shape[2]
    if K == 1:
        return torch.zeros(N, dtype=torch.int64), torch.ones(N, dtype=torch.bool)
    xh, e = x.double(), embed[0].double()
    dist = (xh.pow(2).sum(-1, keepdim=True) - 2 * xh @ e) + e.pow(2).sum(0).unsqueeze(0)
    two = dist.topk(2, dim=-1, largest=False)
    gap = two.values[:, 1] - two.values[:, 0]
    bound = 4 * d * 2.0 ** -24 * (xh.norm(dim=-1) + e.norm(dim=0).max()) ** 2
    return two.indices[:, 0], gap > bound


@functools.lru_cache(maxsize=None)
def reference_of(d, K, N, seed):
    return reference64(*problem(d, K, N, seed))


def search(dev, x, embed, alias=False, extra_rows=0, N=None):
    """msmc_vq_search_wide directly -> (rc, quant, diff, ind) on the host; ``extra_rows``: the output buffers are that many rows
    longer than N (NaN / -7 filled)"""
    from msmctts_amd.hip import lib, vq
    _, d, K = embed.shape
    N = x.shape[0] if N is None else N
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    xd = x.clone().to(dev)
    rows = max(N, 0) + extra_rows
    quant = xd if alias else torch.full((rows, d), float('nan')).to(dev)
    diff = torch.full((rows, d), float('nan')).to(dev)
    ind = torch.full((rows, 1), -7, dtype=torch.int64).to(dev)
    L = lib.get()
    rc = L.msmc_vq_search_wide(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(quant), lib.ptr(diff), lib.ptr(ind), N, d, K,
                               lib.stream(xd))
    return rc, quant.cpu(), diff.cpu(), ind.cpu()


def check_against_float64(dev, x, embed, want, decided, splits=SPLITS, alias_too=False):
    K = embed.shape[2]
    for wc in splits:
        with forced_split(wc):
            rc, q, df, ind = search(dev, x, embed)
            assert rc == 0 and last_kernel() == WIDE, (wc, rc, last_kernel())
            assert int(ind.min()) >= 0 and int(ind.max()) < K, (wc, int(ind.min()), int(ind.max()))
            ind = ind[:, 0]
            wrong = (ind != want) & decided
            assert not bool(wrong.any()), 'split %d: index differs from float64 on %d decided frames, first %s' % (
                wc, int(wrong.sum()), wrong.nonzero()[:4].flatten().tolist())
            wq, wd = exact_outputs(x, embed, ind.view(-1, 1))
            assert same_bits(q, wq), 'split %d: quant is not x + (e - x) of the chosen row' % wc
            assert same_bits(df, wd), 'split %d: diff is not (e - x)^2 of the chosen row' % wc
            if alias_too:
                rc, q2, d2, i2 = search(dev, x, embed, alias=True)
                assert rc == 0 and torch.equal(i2[:, 0], ind) and same_bits(q2, q) and same_bits(d2, df), 'split %d: quant aliasing x' % wc


def check_wide_shape(dev, s, N=WIDE_N, splits=SPLITS):
    d, K = WIDE_SHAPES[s]
    seed = 4800 + s
    x, embed = problem(d, K, N, seed)
    want, decided = reference_of(d, K, N, seed)
    left_out = 1.0 - decided.double().mean().item()
    print('wide d=%d K=%d N=%d: the float64 reference leaves %.4f of the frames undecided' % (d, K, N, left_out))
    assert left_out <= MAX_LEFT_OUT, 'the float64 reference leaves %.3f of the frames undecided' % left_out
    check_against_float64(dev, x, embed, want, decided, splits, alias_too=True)


# ---- (b) first minimum ---------------------------------------------------------------------------------------------------------
def check_first_minimum(dev):
    """centroid 5 copied to 69, 261, 330 (other centroid tiles of every instantiation: 64, 128 or 256 centroids per tile) and to
    K - 1 = 599 in the partial last tile; centroid 63 copied to 64 and 255 to 256 (neighbours across a wave's and a tile's
    boundary).  The copies are the same bits, so a frame is at exactly the same fp32 distance from all of them: frames next to
    5 / 63 / 255 must get 5 / 63 / 255"""
    d, K, N = 64, 600, 48
    gen = torch.Generator().manual_seed(4810)
    embed = torch.randn(1, d, K, generator=gen)
    for k in (69, 261, 330, K - 1):
        embed[0, :, k] = embed[0, :, 5]
    embed[0, :, 64] = embed[0, :, 63]
    embed[0, :, 256] = embed[0, :, 255]
    which = torch.tensor([5, 63, 255] * (N // 3))
    x = (embed[0][:, which].t() + 1e-3 * torch.randn(N, d, generator=gen)).contiguous()
    for wc in SPLITS:
        with forced_split(wc):
            rc, q, df, ind = search(dev, x, embed)
            assert rc == 0 and last_kernel() == WIDE
            assert torch.equal(ind[:, 0], which), (wc, ind[:, 0].tolist())


# ---- (c) partial last tile -----------------------------------------------------------------------------------------------------
def check_partial_last_tile(dev, K):
    """every centroid at a norm of 10 to 15, frames 1e-3 N(0, 1): a zero row in a phantom column of the last tile (with a zero
    norm) would be nearer than any centroid.  Every index is below K and the float64 one; frames next to centroid K - 1 get K - 1"""
    d, N = 48, 40
    gen = torch.Generator().manual_seed(4820 + K)
    embed = torch.randn(1, d, K, generator=gen)
    embed = embed / embed.norm(dim=1, keepdim=True) * (10.0 + 5.0 * torch.rand(1, 1, K, generator=gen))
    assert float(embed.norm(dim=1).min()) >= 10.0 - 1e-4
    x = 1e-3 * torch.randn(N, d, generator=gen)
    want, decided = reference64(x, embed)
    assert bool(decided.all()), 'a frame at the origin is undecided between two centroid norms'
    near = (embed[0][:, K - 1].unsqueeze(0) + 1e-3 * torch.randn(N, d, generator=gen)).contiguous()
    for wc in SPLITS:
        with forced_split(wc):
            rc, q, df, ind = search(dev, x, embed)
            assert rc == 0 and int(ind.max()) < K and int(ind.min()) >= 0, (wc, rc, int(ind.max()))
            assert torch.equal(ind[:, 0], want), (wc, ind[:, 0].tolist(), want.tolist())
            assert same_bits(q, exact_outputs(x, embed, ind)[0])
            rc, q, df, ind = search(dev, near, embed)
            assert rc == 0 and bool((ind == K - 1).all()), (wc, ind[:, 0].tolist())


# ---- (d) d slices ---------------------------------------------------------------------------------------------------------------
def check_d_slices(dev, d):
    """centroids identical except in the last 16 channels (the partial last slice of d % 32 == 16), and another set identical
    except in the first 16: the winner is decided there"""
    K, N = 24, 40
    for where in ('last', 'first'):
        gen = torch.Generator().manual_seed(4830 + d + (where == 'first'))
        base = torch.randn(d, 1, generator=gen)
        embed = base.repeat(1, K).unsqueeze(0).contiguous()
        part = slice(d - 16, d) if where == 'last' else slice(0, 16)
        embed[0, part, :] = torch.randn(16, K, generator=gen)
        target = torch.randint(0, K, (N,), generator=gen)
        x = (embed[0][:, target].t() + 0.01 * torch.randn(N, d, generator=gen)).contiguous()
        want, decided = reference64(x, embed)
        assert bool(decided.all()) and torch.equal(want, target) and len(set(target.tolist())) > 8
        check_against_float64(dev, x, embed, want, decided)


# ---- (e) refusals and guards -------------------------------------------------------------------------------------------------------
def check_refusals_and_guards(dev):
    from msmctts_amd.hip import lib, vq
    gen = torch.Generator().manual_seed(4840)
    for d, K, N in ((40, 24, 5), (2064, 24, 5), (64, 0, 5), (64, 24, -1)):
        x = torch.randn(5, d, generator=gen)
        # (a refused call reads nothing: plain buffers of the operands' sizes -- msmc_vq_prepare itself does not take d = 2064)
        et, en = torch.randn(max(K, 1), d, generator=gen).to(dev), torch.ones(max(K, 1)).to(dev)
        xd = x.to(dev)
        quant, diff = torch.full((5, d), float('nan')).to(dev), torch.full((5, d), float('nan')).to(dev)
        ind = torch.full((5, 1), -7, dtype=torch.int64).to(dev)
        rc = lib.get().msmc_vq_search_wide(lib.ptr(xd), lib.ptr(et), lib.ptr(en), lib.ptr(quant), lib.ptr(diff), lib.ptr(ind),
                                           N, d, K, lib.stream(xd))
        assert rc == E_SHAPE, (d, K, N, rc)
        assert bool(torch.isnan(quant.cpu()).all()) and bool(torch.isnan(diff.cpu()).all()) and bool((ind.cpu() == -7).all()), \
            'a refused call launched'
    # N * d * 4 >= 2^32 is refused before anything is read (the pointers are never touched)
    x, embed = problem(64, 1, WIDE_N, 4805)
    et, en = vq.vq_prepare(embed.to(dev), frames=0)
    guard = torch.full((2, 64), 7.0).to(dev)
    gi = torch.full((2, 1), -7, dtype=torch.int64).to(dev)
    L = lib.get()
    rc = L.msmc_vq_search_wide(lib.ptr(guard), lib.ptr(et), lib.ptr(en), lib.ptr(guard), lib.ptr(guard), lib.ptr(gi), 1 << 24, 64, 1,
                               lib.stream(guard))
    assert rc == E_SHAPE, rc
    # N = 0: returns 0, guard rows untouched
    rc = L.msmc_vq_search_wide(lib.ptr(guard), lib.ptr(et), lib.ptr(en), lib.ptr(guard), lib.ptr(guard), lib.ptr(gi), 0, 64, 1,
                               lib.stream(guard))
    assert rc == 0
    assert bool((guard.cpu() == 7).all()) and bool((gi.cpu() == -7).all())
    # N = 37 in oversized buffers: the rows beyond N stay as they were, in every instantiation
    d, K = WIDE_SHAPES[SMALL_N_SHAPE]
    x, embed = problem(d, K, 37, 4800 + SMALL_N_SHAPE)
    for wc in SPLITS:
        with forced_split(wc):
            rc, q, df, ind = search(dev, x, embed, extra_rows=70)
            assert rc == 0
            assert bool(torch.isnan(q[37:]).all()) and bool(torch.isnan(df[37:]).all()) and bool((ind[37:] == -7).all()), wc
            assert not bool(torch.isnan(q[:37]).any()) and not bool(torch.isnan(df[:37]).any()) and bool((ind[:37] >= 0).all()), wc


# ---- (f) routing ---------------------------------------------------------------------------------------------------------------
def check_routing(dev):
    """shapes msmc_vq_search takes keep their kernel and their bits; a single head it refuses runs the wide kernel"""
    from msmctts_amd.hip import vq
    from msmctts_amd.networks.vqgantts.modules import MultiHeadQuantize, Quantize
    gen = torch.Generator().manual_seed(4850)
    for dim, K, kernel in ((1024, 100, WIDE), (64, 24, WIDE), (256, 160, 'vq_search_stream_kernel')):
        q = Quantize(dim, K).to(dev).eval()
        out = q(torch.randn(2, 9, dim, generator=gen).to(dev), torch.tensor([9, 4]).to(dev), update=False)
        assert last_kernel() == kernel, (dim, K, last_kernel())
        assert tuple(out[0].shape) == (2, 9, dim) and tuple(out[2].shape) == (2, 9) and int(out[2].max()) < K
    # 4 heads x 64 x 64: the resident kernel, with the bits of a direct msmc_vq_search
    x, embed = vqs.problem(4, 64, 64, 37, 4100)
    rc, q0, d0, i0 = vqs.search(dev, x, embed)
    assert rc == 0 and last_kernel() not in (WIDE, 'vq_search_stream_kernel')
    resident = last_kernel()
    m = MultiHeadQuantize(256, 64, 4)
    for h, sub in enumerate(m.quantizers):
        sub.embed.copy_(embed[h])
    m = m.to(dev).eval()
    qq, dd, ii = m(x.view(1, 37, 256).to(dev), torch.tensor([37]).to(dev), update=False)
    assert last_kernel() == resident, (last_kernel(), resident)
    assert torch.equal(ii.cpu().view(37, 4), i0) and same_bits(qq.detach().cpu().view(37, 256), q0) and same_bits(dd.detach().cpu().view(37, 64), d0)
    # the wrapper refuses what neither kernel takes
    et, en = vq.vq_prepare(torch.randn(1, 40, 24, generator=gen).to(dev), frames=0)
    with vqs._raises(RuntimeError, 'msmc_vq_search failed with code -2'):
        vq.vq_search(torch.zeros(4, 40).to(dev), et, en)
    # training with update at d > 512: the EMA kernels keep their limit
    q = Quantize(1024, 100).to(dev).train()
    with vqs._raises(RuntimeError, 'msmc_vq_ema_update failed with code -2'):
        q(torch.randn(2, 9, 1024, generator=gen).to(dev), torch.tensor([9, 4]).to(dev), update=True)


def check_module_gradient(dev, dim, K):
    """eval ``Quantize`` on the wide kernel against the restated reference forward: quant, diff and the gradient of
    ``quant.sum() * 0.5 + (diff * w).sum()`` (backward: msmc_vq_backward), tolerances of ``_vqstreamcases.check_module``"""
    from _parity import close
    from msmctts_amd.networks.vqgantts.modules import Quantize
    B, T = 3, 12
    x4, embed = problem(dim, K, B * T, 4860 + K)
    x = x4.view(B, T, dim).clone()
    q = Quantize(dim, K)
    q.embed.copy_(embed[0])
    q = q.to(dev).eval()
    want, decided = reference64(x4, embed)
    assert 1.0 - decided.double().mean().item() <= MAX_LEFT_OUT
    lens = torch.tensor([12, 7, 3], dtype=torch.int64)
    w = torch.arange(B * T * dim).view(B, T, dim) / float(B * T * dim)
    xd = x.clone().to(dev).requires_grad_(True)
    qq, dd, ii = q(xd, lens.to(dev), update=False)
    assert last_kernel() == WIDE, last_kernel()
    got = ii.cpu().view(-1)
    assert torch.equal(got[decided], want[decided]), 'indices'
    ind = torch.where(decided, want, got).view(B, T, 1)
    xr = x.clone().requires_grad_(True)
    heads = [(embed[0].clone(), torch.zeros(K), embed[0].clone())]
    q0, d0, _ = vqs._restated_forward(xr, lens, heads, ind, q.decay, q.eps, False)
    scale = float(q0.detach().abs().max())
    close(qq, q0, 5e-6 * max(1.0, scale), what='quant')
    close(dd, d0, 5e-6 * max(1.0, scale * scale), 1e-5, what='diff')
    (qq.sum() * 0.5 + (dd * w.to(dev)).sum()).backward()
    (q0.sum() * 0.5 + (d0 * w).sum()).backward()
    close(xd.grad, xr.grad, 5e-6 * max(1.0, scale), 1e-5, what='grad')


# ---- (g) model parity ------------------------------------------------------------------------------------------------------------
def _golden():
    from _parity import load_npz
    return load_npz('small_kmeans.npz')


def build_model(dev, tmpdir, form='pickle', load=True):
    """the small KMeansVQGANEmb of the fixture, its centroid file written here (pickle of ``KMeansModel``, or .npy)"""
    from _parity import json_field, load_npz, t
    from msmctts_amd.networks import find_modules
    z = _golden()
    cfg = json_field(z['cfg'])
    centers = z['centers']
    path = os.path.join(str(tmpdir), 'kmeans.' + ('npy' if form == 'npy' else 'pkl'))
    if form == 'npy':
        np.save(path, centers)
    else:
        with open(path, 'wb') as fout:
            pickle.dump(KMeansModel(centers), fout)
    (_, m), = find_modules({'autoencoder': dict(cfg, _name='KMeansVQGANEmb', quantizer_path=path)})
    if load:
        want_keys = [k[len('state.'):] for k in z if k.startswith('state.')]
        assert sorted(m.state_dict().keys()) == sorted(want_keys), set(m.state_dict().keys()) ^ set(want_keys)
        ze = load_npz('small_ecapa.npz')                 # the global encoder's weights: those of the ECAPA fixture, not stored twice

        def val(k):
            a = ze['enc.state.' + k[len('global_encoder.'):]] if k.startswith('global_encoder.') else z['state.' + k]
            return t(a.astype(np.float32) if a.dtype == np.float16 else a)
        m.load_state_dict({k: val(k) for k in want_keys})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return z, m.to(dev)


def check_model_parity(dev, tmpdir):
    from _parity import close, t
    z, m = build_model(dev, tmpdir)
    m.eval()
    emb, lengths, mel = (t(z['batch.' + k]).to(dev) for k in ('emb', 'emb_length', 'mel'))
    centers = torch.from_numpy(z['centers'])
    B, T, d = emb.shape
    want, decided = reference64(emb.cpu().reshape(B * T, d), centers.t().unsqueeze(0).contiguous())
    assert 1.0 - decided.double().mean().item() <= MAX_LEFT_OUT
    assert torch.equal(torch.from_numpy(z['full.encoder_indices.0']).view(-1)[decided], want[decided]), 'the fixture against float64'
    windows = [tuple(int(v) for v in row) for row in z['windows']]

    def indices_match(o):
        assert isinstance(o['encoder_indices'], (tuple, list)) and len(o['encoder_indices']) == 1
        got = o['encoder_indices'][0].cpu()
        assert got.shape == (B, T) and got.dtype == torch.int64
        assert torch.equal(got.view(-1)[decided], want[decided]), 'encoder_indices on decided frames'

    with torch.no_grad():
        o = m(emb, lengths, mel=mel)                                         # window='full'
        assert last_kernel() == WIDE, last_kernel()
        assert set(o) == {'encoder_indices', 'mel_outputs', 'decoder_outputs'}
        indices_match(o)
        close(o['mel_outputs'], z['full.mel_outputs'], what='full mel_outputs')
        close(o['decoder_outputs'], z['full.decoder_outputs'], what='full decoder_outputs')
        o = m(emb, lengths, mel=mel, window=windows)
        indices_match(o)
        close(o['mel_outputs'], z['window.mel_outputs'], what='window mel_outputs')
        close(o['decoder_outputs'], z['window.decoder_outputs'], what='window decoder_outputs')
        table = torch.tensor([(i, s) for i, s, _ in windows], dtype=torch.int32).to(dev)
        o2 = m(emb, lengths, mel=mel, window=table, window_frames=windows[0][2] - windows[0][1])
        assert torch.equal(o2['decoder_outputs'], o['decoder_outputs']), 'the (utterance, start) table against the triples'
        o = m(emb, lengths, mel=mel, window=None)
        assert set(o) == {'encoder_indices', 'mel_outputs'}
        # analysis (eval) -> synthesis, which quantises its inputs again
        qs = m.analysis(emb, lengths)
        assert set(qs) == {'residual_output', 'quantizer_outputs', 'quantizer_diffs', 'quantizer_indices', 'quantizer_lengths',
                           'predictor_diffs'} and qs['residual_output'] is None and qs['predictor_diffs'] is None
        assert torch.equal(qs['quantizer_indices'][0].cpu().view(-1)[decided], want[decided])
        rows = centers[qs['quantizer_indices'][0].cpu().view(-1)].view(B, T, d)
        assert torch.equal(qs['quantizer_outputs'][0].cpu(), emb.cpu() + (rows - emb.cpu())), 'quantizer_outputs'
        wav = m.synthesis(list(qs['quantizer_outputs']), qs['quantizer_lengths'], ref=mel)
        close(wav, z['eval.synthesis'], what='synthesis')
    m.train()
    with vqs._raises(NotImplementedError, 'msmc_vqgan_emb.py:429'):
        m.analysis(emb, lengths)


def check_model_surface(dev, tmpdir):
    """constructor keywords, state_dict keys, the two centroid file forms, the frozen codebook across load_state_dict,
    construction-time refusals"""
    from msmctts_amd.networks import find_modules
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansQuantizer, KMeansVQGANEmb
    z, m = build_model('cpu', tmpdir)
    assert type(m) is KMeansVQGANEmb and type(m.quantizer) is KMeansQuantizer
    centers = torch.from_numpy(z['centers'])
    keys = set(m.state_dict().keys())
    assert {'quantizer.quantizer.0.embed', 'quantizer.quantizer.0.cluster_size', 'quantizer.quantizer.0.embed_avg',
            'in_linear.weight', 'in_linear.bias', 'mel_predictor.weight', 'mel_predictor.bias'} <= keys
    assert all(k.split('.')[0] in ('quantizer', 'in_linear', 'decoder', 'frame_decoder', 'global_encoder', 'mel_predictor') for k in keys)
    # a checkpoint's embed never counts: the centroids of the file are in the buffer again after load_state_dict
    assert torch.equal(m.quantizer.quantizer[0].embed, centers.t())
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd['quantizer.quantizer.0.embed'] = torch.zeros_like(sd['quantizer.quantizer.0.embed'])
    m.load_state_dict(sd)
    assert torch.equal(m.quantizer.quantizer[0].embed, centers.t())
    _, m2 = build_model('cpu', tmpdir, form='npy', load=False)
    assert torch.equal(m2.quantizer.quantizer[0].embed, centers.t())
    from _parity import json_field
    cfg = json_field(z['cfg'])
    path = os.path.join(str(tmpdir), 'kmeans.npy')
    with vqs._raises(NotImplementedError, 'ECAPA_TDNN'):
        find_modules({'autoencoder': dict(cfg, _name='KMeansVQGANEmb', quantizer_path=path, n_model_size=96)})
    with vqs._raises(NotImplementedError, 'ECAPA_TDNN'):
        find_modules({'autoencoder': dict(cfg, _name='KMeansVQGANEmb', quantizer_path=path, mel_dim=20)})
    with vqs._raises(ValueError, 'Wrong global encoder'):
        find_modules({'autoencoder': dict(cfg, _name='KMeansVQGANEmb', quantizer_path=path, global_encoder_config={'_name': 'Other'})})
    bad = os.path.join(str(tmpdir), 'bad.npy')
    np.save(bad, np.zeros((3, 4, 5), dtype=np.float32))
    with vqs._raises(ValueError, '[K, d]'):
        KMeansQuantizer(bad)


# ---- (h) trainer -------------------------------------------------------------------------------------------------------------------
def trainer_config(path):
    import _embcases as E
    from msmctts_amd.utils.config import Config
    z = _golden()
    from _parity import json_field
    base = E.config(False)
    # the fixture's model with the vocoder of the Emb trainer cases: 300 samples per frame, the batch's hop
    ae = dict(json_field(z['cfg']), _name='KMeansVQGANEmb', quantizer_path=path,
              decoder_config=dict(base.task.autoencoder.decoder_config))
    return Config({'id': 'small_kmeans', 'task': {'_name': 'NASynTTSEmb', 'autoencoder': ae, 'discriminator': base.task.discriminator},
                   'trainer': dict(E.TRAINER), 'optimizer': {'_default': dict(E.OPT)},
                   'dataset': dict(samplerate=24000, feature=['emb', 'mel', 'wav'], frameshift=[E.HOP, E.HOP, 1])})


def check_trainer_phase(dev, tmpdir, phase):
    """one EmbVQGANTrainer step of ``phase`` on the small KMeansVQGANEmb: finite losses and no VQ key, in_linear and (once the
    vocoder runs) decoder parameters move, the centroid buffer keeps its bits, ``last_windows`` is what the RNG draws"""
    import _embcases as E
    from _parity import t
    from msmctts_amd.tasks import build_task
    z = _golden()
    path = os.path.join(str(tmpdir), 'kmeans.pkl')
    with open(path, 'wb') as fout:
        pickle.dump(KMeansModel(z['centers']), fout)
    cfg = trainer_config(path)
    torch.manual_seed(31)
    task = build_task(cfg, mode='train')
    for mod in task.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    task = task.to(dev).train()
    tr = E._trainer(cfg, task, seed=200 + phase)
    iteration = E.PHASE_ITERATION[phase]
    assert tr._phase(iteration) == phase
    emb, lengths, mel = (t(z['batch.' + k]) for k in ('emb', 'emb_length', 'mel'))
    B, T, _ = emb.shape
    gen = torch.Generator().manual_seed(32)
    wav = torch.rand(B, T * E.HOP, 1, generator=gen) * 2 - 1
    wav = torch.where(torch.arange(T * E.HOP)[None, :, None] < (lengths * E.HOP)[:, None, None], wav, torch.zeros(()))
    batch = {k: v.to(dev) for k, v in dict(emb=emb, emb_length=lengths, mel=mel, wav=wav, wav_length=lengths * E.HOP).items()}
    batch['emb_length_host'] = lengths.tolist()
    before = {k: v.detach().clone() for k, v in task.state_dict().items()}
    task.zero_grad()
    log = tr.train_step(batch, iteration)
    assert last_kernel() == WIDE, last_kernel()
    expect = {'frame_loss'} | ({'stft_loss'} if phase > 0 else set())
    expect |= {'d_loss_real', 'd_loss_fake', 'd_loss', 'fm_loss', 'adv_loss', 'g_loss'} if phase == 2 else set()
    assert set(log['loss']) == expect, sorted(log['loss'])
    for k, v in log['loss'].items():
        assert np.isfinite(float(v)), (k, float(v))
    after = task.state_dict()
    moved = {k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k])}
    assert 'autoencoder.in_linear.weight' in moved, sorted(moved)[:8]
    assert any(k.startswith('autoencoder.decoder.') for k in moved) == (phase > 0)
    k = 'autoencoder.quantizer.quantizer.0.embed'
    assert same_bits(before[k].cpu(), after[k].cpu()) and same_bits(after[k].cpu(), torch.from_numpy(z['centers']).t().contiguous())
    if phase == 0:
        assert tr.last_windows is None
    else:
        want = E.reference_windows(random.Random(200 + phase), lengths.tolist(), tr.sample_batch_size, tr.frame_lengths)
        assert tr.last_windows == [(i, s) for i, s, _ in want], (tr.last_windows, want)


# ---- (i) feature presence --------------------------------------------------------------------------------------------------------
def check_feature_present():
    from msmctts_amd.hip import lib
    assert 'msmc_vq_search_wide' in lib.exported_symbols()
    assert isinstance(lib.get().msmc_vq_search_wide, ctypes._CFuncPtr)
    from msmctts_amd.networks.vqgantts.msmc_vqgan_emb import KMeansQuantizer, KMeansVQGANEmb  # noqa: F401
