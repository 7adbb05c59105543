"""Shared cases of the single-channel spectral domains of the resolution discriminators (``mrd_config.domain`` 'linear' / 'log':
csrc/spectral.hip mrd_image1_*, the C_in = 1 first convolution): tests/test_mrd_domains_emu.py runs the kernel-level ones on the
kernel interpreter, tests/test_gpu_mrd_domains.py all of them on the GPU.

Fixture: tests/golden/small_mrd_domains.npz (tests/golden/make_golden_mrd_domains.py -- the reference's own
MultiResolutionDiscriminator).  Bars: scores and feature maps 1e-3 abs (tests/_parity.py TOL); gradients the bar of
tests/_parity.py check_train_steps for the discriminator fixture (norm within 2e-3, elements within 1e-5 + 2e-3 |reference|).
"""
import numpy as np
import torch

from _parity import TOL, close
from _util import load_npz, t

DOMAINS = (('linear', 0), ('log', 1))
CASES = [(d, m) for d in ('linear', 'log') for m in (True, False)]
MPD = dict(periods=[2, 3], channels=4, max_channels=16)
_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(load_npz('small_mrd_domains.npz'))
    return _FIXTURE[0]


def digest(tensor, samples):
    """mirrors tests/golden/make_golden_mrd_domains.py::digest (data layout of the fixture, not code of the reference)"""
    f = tensor.detach().reshape(-1).double().cpu()
    idx = np.unique(np.linspace(0, f.numel() - 1, samples).round().astype(np.int64))
    return np.concatenate([[f.mean().item(), f.abs().mean().item(), f.std().item(), float(f.numel())], f[torch.from_numpy(idx)].numpy()])


def build_discriminator(dev, domain, mel_scale, dtype=torch.float32):
    """the product Discriminator over the fixture's resolution stacks (state_dict of the fixture; the period family, which the
    fixture does not cover, keeps its seeded initial weights)"""
    from msmctts_amd.networks.hifigan.discriminator import Discriminator
    z = fixture()
    torch.manual_seed(11)
    d = Discriminator(dict(hop_lengths=z['hops'].tolist(), hidden_channels=z['hidden'].tolist(), domain=domain, mel_scale=mel_scale,
                           sample_rate=24000), dict(MPD))
    d.mrd.load_state_dict({k[len('state.'):]: t(v) for k, v in z.items() if k.startswith('state.')})
    d.hip_dtype = dtype
    return d.to(dev).train()


def check_fixture_case(dev, domain, mel_scale, report=print):
    z = fixture()
    tag = '%s.%s' % (domain, 'mel' if mel_scale else 'plain')
    n, ns = len(z['hops']), int(z['digest_samples'])
    d = build_discriminator(dev, domain, mel_scale)
    x = t(z['wav']).to(dev).requires_grad_(True)
    scores, fmaps = d(x)
    scores, fmaps = scores[:n], fmaps[:n]                       # (resolution family first)
    sum(s.float().pow(2).sum() for s in scores).backward()
    worst = 0.0
    for i, s in enumerate(scores):
        want = z['%s.score.%d' % (tag, i)]
        worst = max(worst, float(np.abs(s.detach().cpu().numpy() - want).max()))
        assert len(fmaps[i]) == 6
        for j, f in enumerate(fmaps[i]):
            assert list(f.shape) == z['%s.fmap_shape.%d.%d' % (tag, i, j)].tolist()
            got, wantd = digest(f, ns), z['%s.fmap.%d.%d' % (tag, i, j)].astype(np.float64)
            worst = max(worst, float(np.abs(got - wantd).max()))
    report('mrd %-12s scores / fmaps: worst abs err %.3e (bar %.1e)' % (tag, worst, TOL))
    grads = {'grad_wav': x.grad}
    for name, p in d.mrd.named_parameters():
        if '.discriminator.0.1.' in name:
            grads['grad.' + name] = p.grad
    assert len(grads) == 1 + 3 * n
    for k, g in sorted(grads.items()):
        want = z['%s.%s' % (tag, k)]
        assert g is not None, k
        gn, wn = g.double().norm().item(), float(np.linalg.norm(want.astype(np.float64)))
        err = np.abs(g.detach().double().cpu().numpy() - want)
        report('mrd %-12s %-50s norm %.6e (ref %.6e)  worst elem err %.3e at |ref| %.3e'
               % (tag, k, gn, wn, err.max(), np.abs(want).reshape(-1)[err.argmax()]))
    for i, s in enumerate(scores):
        close(s, z['%s.score.%d' % (tag, i)], what='%s score %d' % (tag, i))
        for j, f in enumerate(fmaps[i]):
            close(digest(f, ns), z['%s.fmap.%d.%d' % (tag, i, j)].astype(np.float64), what='%s fmap %d %d' % (tag, i, j))
    for k, g in sorted(grads.items()):
        want = z['%s.%s' % (tag, k)]
        gn, wn = g.double().norm().item(), float(np.linalg.norm(want.astype(np.float64)))
        assert abs(gn - wn) <= 2e-3 * max(wn, 1e-3) + 1e-6, (tag, k, gn, wn)
        close(g, want, 1e-5, 2e-3, what='%s %s' % (tag, k))


def stfts_for(hops, mel_scale):
    from msmctts_amd.utils.audio import TorchSTFT
    return {dom: [TorchSTFT(fft_size=h * 4, hop_size=h, win_size=h * 4, normalized=True, domain=dom, mel_scale=mel_scale,
                            sample_rate=24000) for h in hops] for dom in ('double', 'linear', 'log')}


def check_image_exact(dev, x, hops, mel_scales=(True, False)):
    """``image_cl`` of 'linear' / 'log' is channel 0 / 1 of the 'double' image of the same waveform bit for bit (fp32 and bf16)"""
    for mel_scale in mel_scales:
        st = stfts_for(hops, mel_scale)
        for dtype in (torch.float32, torch.bfloat16):
            for k in range(len(hops)):
                both = st['double'][k].image_cl(x, dtype)
                for dom, c in DOMAINS:
                    one = st[dom][k].image_cl(x, dtype)
                    assert one.dtype == dtype and tuple(one.shape) == tuple(both.shape[:3]) + (1,) and one.is_contiguous()
                    assert torch.equal(one[..., 0], both[..., c]), (dom, mel_scale, dtype, hops[k])
                    # the reference's return layout: (B, F, T') for one channel
                    if dtype == torch.float32:
                        tr, _ = st[dom][k].transform(x)
                        assert torch.equal(tr, both[..., c])


def check_lockstep(dev, x, hops, rows=(1, 3)):
    """msmc_spectral_multi over the front-ends of ``hops`` is bit for bit the chains run one by one, forward and backward, for
    every domain (pattern of tests/_parity.py check_fronts_lockstep)"""
    from msmctts_amd.hip import spectral
    g = torch.Generator().manual_seed(9)
    for dom in ('double', 'linear', 'log'):
        st = stfts_for(hops, True)[dom]
        st[-1] = stfts_for(hops[-1:], False)[dom][0]            # (one chain without a filter bank)
        C = 2 if dom == 'double' else 1
        for dtype in (torch.float32, torch.bfloat16):
            specs = [(s_.fft_size, s_.hop_size) + tuple(s_.consts(x.device)) for s_ in st]
            together = spectral.mrd_fronts(x, specs, dtype, domain=dom)
            alone = [spectral.MrdFront(x, n_fft, hop, dft, fb, dtype, domain=dom) for n_fft, hop, dft, fb in specs]
            for a, b in zip(together, alone):
                assert tuple(a.img.shape) == (x.shape[0], a.F, a.T, C)
                for name in ('spec', 'mag', 'mel', 'img'):
                    assert torch.equal(getattr(a, name), getattr(b, name)), (dom, dtype, a.hop, name)
            r0, r1 = rows
            gs = [torch.randn(r1 - r0, f.F, f.T, C, generator=g).to(dev).to(dtype) for f in alone]
            got = spectral.backward_rows_lockstep(together, gs, r0, r1)
            for a, b, gi in zip(got, alone, gs):
                assert torch.equal(a, b.backward_rows(gi, r0, r1)), (dom, dtype, b.hop)


def clamp_straddling_mel(B=2, T=37, F=31, seed=3):
    """a magnitude tensor [B, 1, T, pad4(F)] whose log channel lies below 0, inside (0, 1) and above 1 for at least 5 % of the
    elements each (checked here, on the CPU): log10 m uniform over [-6, 3], the clamp edges are at -4 and 1"""
    g = torch.Generator().manual_seed(seed)
    FP = (F + 3) // 4 * 4
    mel = torch.zeros(B, 1, T, FP)
    mel[..., :F] = 10.0 ** (torch.rand(B, 1, T, F, generator=g) * 9.0 - 6.0)
    lg = (20.0 * torch.log10(mel[..., :F].double()) - 20.0 + 100.0) / 100.0
    for region in (lg < 0, (lg > 0) & (lg < 1), lg > 1):
        assert region.double().mean().item() >= 0.05
    return mel, F


def _formula(v, c):
    return v if c == 0 else torch.clamp((20.0 * torch.log10(v) - 20.0 + 100.0) / 100.0, 0.0, 1.0)


def check_image_backward(dev, report=print):
    """the single-channel kernels' backward against torch autograd on the formula in fp64, on an input that meets both clamp
    edges; the forward against channel c of the two-channel kernel, exactly.  Bound (that of tests/_bncases.py for its
    backward): 4 x the max abs error of torch's own fp32 autograd on the same formula against fp64, with a floor of 4 fp32 ulps
    of the largest gradient.  The bf16 case feeds a bf16 image gradient (exact in fp32) and writes the same fp32 gradient."""
    from msmctts_amd.hip import spectral
    mel, F = clamp_straddling_mel()
    g = torch.Generator().manual_seed(4)
    for dtype in (torch.float32, torch.bfloat16):
        both = spectral._MrdImage.apply(mel.to(dev), F, dtype)
        for dom, c in DOMAINS:
            m = mel.to(dev).clone().requires_grad_(True)
            img = spectral._MrdImage.apply(m, F, dtype, dom)
            assert tuple(img.shape) == tuple(both.shape[:3]) + (1,) and torch.equal(img[..., 0], both[..., c]), (dom, dtype)
            go = torch.randn(img.shape, generator=g).to(dtype)
            img.backward(go.to(dev))
            refs = []
            for ref_dtype in (torch.float64, torch.float32):
                mr = mel.to(ref_dtype).clone().requires_grad_(True)
                v = _formula(mr[:, 0, :, :F].transpose(1, 2), c)                       # [B, F, T]
                (v.unsqueeze(-1) * go.to(ref_dtype)).sum().backward()
                refs.append(mr.grad.double())
            want, torch32 = refs
            got = m.grad.cpu().double()
            if c == 1:              # the zero-gradient regions are met, and met exactly
                lg = (20.0 * torch.log10(mel[..., :F].double()) - 20.0 + 100.0) / 100.0
                dead = (lg < 0) | (lg > 1)
                assert dead.double().mean().item() >= 0.1 and (got[..., :F][dead] == 0).all()
            assert (got[..., F:] == 0).all()
            ulp = float(np.spacing(np.float32(want.abs().max().item())))
            bound = max(4 * (torch32 - want).abs().max().item(), 4 * ulp)
            err = (got - want).abs().max().item()
            report('image1 bwd %-6s %s err %.3e bound %.3e' % (dom, 'bf16' if dtype == torch.bfloat16 else 'fp32', err, bound))
            assert err <= bound, (dom, dtype, err, bound)


def check_front_reuse(dev, B=3, L=2410, domain='log'):
    """``disc(x[B:2B], fronts=fronts.rows(B, 2B))`` equals ``disc(x[B:2B])`` exactly"""
    from msmctts_amd.hip import convnet
    assert convnet.GROUPED
    z = fixture()
    d = build_discriminator(dev, domain, True)
    g = torch.Generator().manual_seed(31)
    x = torch.cat((torch.randn(B, L, generator=g), t(z['wav'])), 0).to(dev)
    with torch.no_grad():
        fronts = d.spectral_fronts(x)
        assert all(tuple(f.img.shape) == (2 * B, f.F, f.T, 1) for f in fronts.fronts)
        s1, f1 = d(x[B:2 * B], fronts=fronts.rows(B, 2 * B))
        s2, f2 = d(x[B:2 * B])
    for a, b in zip(s1, s2):
        assert torch.equal(a, b)
    for fa, fb in zip(f1, f2):
        for a, b in zip(fa, fb):
            assert torch.equal(a, b)
    # with gradient history: the images' gradient flows back through the saved front-end tensors
    y1 = x[B:2 * B].clone().requires_grad_(True)
    y2 = x[B:2 * B].clone().requires_grad_(True)
    n = len(fronts.fronts)
    sum(s.float().pow(2).sum() for s in d(y1, fronts=fronts.rows(B, 2 * B, wav=y1))[0][:n]).backward()
    sum(s.float().pow(2).sum() for s in d(y2)[0][:n]).backward()
    assert torch.equal(y1.grad, y2.grad)


def check_image_unaligned_and_refusals(dev):
    """the C ABI directly: an image (forward) or a magnitude / gradient pair (backward) that starts one element past an aligned
    address takes the element-by-element path and gives the same bits; bad arguments are refused"""
    from msmctts_amd.hip import lib
    L = lib.get()
    mel, F = clamp_straddling_mel()
    mel = mel.to(dev)
    B, _, T, FP = mel.shape
    st = lib.stream(mel)
    g = torch.Generator().manual_seed(8)
    for code, dtype in ((0, torch.float32), (1, torch.bfloat16)):
        for ch in (0, 1):
            img = torch.empty(B, F, T, 1, dtype=dtype, device=dev)
            assert L.msmc_mrd_image1_fwd_dt(lib.ptr(mel), lib.ptr(img), B, T, F, FP, ch, code, st) == 0
            buf = torch.zeros(img.numel() + 2, dtype=dtype, device=dev)
            off = buf[1:1 + img.numel()]
            assert L.msmc_mrd_image1_fwd_dt(lib.ptr(mel), lib.ptr(off), B, T, F, FP, ch, code, st) == 0
            assert torch.equal(off.view_as(img), img) and float(buf[0]) == 0 and float(buf[-1]) == 0      # (nothing past the ends)
            go = torch.randn(img.shape, generator=g).to(dtype).to(dev)
            gm = torch.empty_like(mel)
            assert L.msmc_mrd_image1_bwd_dt(lib.ptr(mel), lib.ptr(go), lib.ptr(gm), B, T, F, FP, ch, code, st) == 0
            mbuf, gbuf = torch.zeros(mel.numel() + 2, device=dev), torch.zeros(mel.numel() + 2, device=dev)
            mbuf[1:-1] = mel.reshape(-1)
            assert L.msmc_mrd_image1_bwd_dt(lib.ptr(mbuf[1:]), lib.ptr(go), lib.ptr(gbuf[1:]), B, T, F, FP, ch, code, st) == 0
            assert torch.equal(gbuf[1:-1].view_as(gm), gm) and float(gbuf[0]) == 0 and float(gbuf[-1]) == 0
    img = torch.empty(B, F, T, 1, device=dev)
    E_SHAPE = -2
    assert L.msmc_mrd_image1_fwd_dt(lib.ptr(mel), lib.ptr(img), B, T, F, FP, 2, 0, st) == E_SHAPE
    assert L.msmc_mrd_image1_fwd_dt(lib.ptr(mel), lib.ptr(img), B, T, F, FP, 0, 2, st) == E_SHAPE
    assert L.msmc_mrd_image1_fwd_dt(lib.ptr(mel), lib.ptr(img), B, T, F, F - 1, 0, 0, st) == E_SHAPE
    assert L.msmc_mrd_image1_bwd_dt(lib.ptr(mel), None, lib.ptr(mel), B, T, F, FP, 0, 0, st) == E_SHAPE
    op = lib.SpectralOp()
    op.kind, op.dtype, op.channel = 8, 0, 2
    op.a, op.out, op.B, op.T, op.F, op.FP = mel.data_ptr(), img.data_ptr(), B, T, F, FP
    assert L.msmc_spectral_multi((lib.SpectralOp * 1)(op), 1, st) == E_SHAPE


def build_small_task(dev, domain):
    """the small model of small_steps.npz (tests/_parity.py build_small) with only ``mrd_config.domain`` changed: the first
    convolution of every resolution stack keeps the input channel its domain reads (0: magnitude, 1: log-magnitude)"""
    import _parity
    from msmctts_amd.tasks import build_task
    cfg = _parity.small_config()
    cfg.task['discriminator']['mrd_config']['domain'] = domain
    task = build_task(cfg, mode='train')
    assert task.discriminator.mrd.domain == domain
    c = dict(DOMAINS)[domain]
    sd = {k: t(v) for k, v in load_npz('small_state.npz').items()}
    for k in list(sd):
        if k.startswith('discriminator.mrd.') and k.endswith('.discriminator.0.1.weight_v'):
            sd[k] = sd[k][:, c:c + 1].contiguous()
    task.load_state_dict(sd)
    for m in task.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return cfg, task.to(dev).train()


def gan_step_losses(dev, domain, graphed, amp_dtype, limit_s=240):
    """the loss dictionary of ONE GAN-phase train_step (iteration 6 > warmup_steps = 5) of that model, as
    tests/test_gpu_parity.py graphed_vs_eager runs it.  The step runs under a watchdog of its own: if it does not come back
    within ``limit_s`` seconds the process ends there (nothing further is started on a device that hangs)."""
    import faulthandler
    import random
    from msmctts_amd.synthetic import make_batch
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    batch = make_batch(3, 24, 80, 300, seed=5, device=dev)
    batch['mel_length_host'] = batch['mel_length'].tolist()
    cfg, task = build_small_task(dev, domain)
    tr = build_trainer(cfg, task, num_gpus=0, rank=0)
    tr.model = task
    tr.optimizer = build_optimizer(task, cfg.optimizer, capturable=True)
    tr.use_graphs = graphed
    if amp_dtype is not None:
        tr.amp_dtype = amp_dtype
    tr.rng = random.Random(3)
    faulthandler.dump_traceback_later(limit_s, exit=True)
    try:
        if not tr.replays(6):
            task.zero_grad()
        log = tr.train_step(batch, 6)
        if torch.device(dev).type == 'cuda':
            torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()
    if graphed:
        assert tr._graphs is not None
    return {k: float(v) for k, v in log['loss'].items()}
