"""GPU (-m gpu): the implicit-GEMM convolution kernels (csrc/conv.hip, csrc/conv_wgrad.hip) at the CSMSC layer shapes against
PyTorch-ROCm's own convolutions on the same device (fp32 reference of the same op), forward, data gradient
and weight gradient; fp32 kernels within 2e-4 of the output scale, bf16 kernels within 2e-2."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


from _convcases import (CONVS, SMALL, check_conv_case, check_conv_shared_state, check_mixed_family_groups, cl, conv_part_errors,
                        nchw, rel)


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 2e-4), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize('case', CONVS, ids=[c[0] for c in CONVS])
def test_conv_forward_dgrad_wgrad(case, dtype, tol):
    check_conv_case(case, dtype, tol, DEV)


@pytest.mark.parametrize('case', SMALL, ids=[c[0] for c in SMALL])
def test_conv_small_and_thin_shapes(case):
    """odd / thin channel counts, ragged tiles; offset (not 16-byte aligned) operands are refused"""
    check_conv_case(case, torch.bfloat16, 2e-2, DEV, batch_offset=1)
    check_conv_case(case, torch.float32, 2e-4, DEV)


def test_grouped_calls_with_members_of_several_kernel_families():
    """the members of tests/test_product_emu.py's test of the same name on the device: bit-equal to single launches, the same
    launch count and launch log"""
    check_mixed_family_groups(DEV)


def test_conv_state_shared_by_forward_and_weight_gradient():
    """tests/test_product_emu.py's test of the same name on the device: the same launch counts and kernel names"""
    check_conv_shared_state(DEV)


@pytest.mark.parametrize('gen', [1, 2, 3])
def test_wgrad_generations_agree(gen):
    """every generation of the bf16 weight-gradient kernels (1: first, 2: fp32 atomics, 3: split partials + fixed-order
    second stage), forced through the descriptor, against PyTorch on mid-size layers; generation 3 is bit-reproducible"""
    from msmctts_amd.hip import conv
    saved = (conv._WGRAD_CANDIDATES, dict(conv.TUNED))
    conv._WGRAD_CANDIDATES = ((gen, 0),)
    try:
        for case in (CONVS[2], CONVS[8], CONVS[9], CONVS[14]):
            conv.TUNED.clear()
            conv._PLANS.clear()
            fresh = (case[0] + ' gen%d' % gen,) + tuple(case[1:])
            check_conv_case(fresh, torch.bfloat16, 2e-2, DEV, parts=('wgrad',))
        if gen == 3:
            name, B, Cin, Cout, H, W, k, s, dil, pad, reflect, slope = CONVS[3]
            geom = conv.Geometry(H, W, k, s, dil, pad, reflect)
            x = torch.randn(B, H, W, Cin, device=DEV).bfloat16()
            g = torch.randn(B, geom.Hout, geom.Wout, Cout, device=DEV).bfloat16()
            outs = []
            for _ in range(3):
                dw, db = torch.zeros(k[0] * k[1], Cout, Cin, device=DEV), torch.zeros(Cout, device=DEV)
                conv.conv_wgrad(x, g, geom, k[0] * k[1], in_slope=slope, dw=dw, db=db)
                outs.append((dw, db))
            assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    finally:
        conv._WGRAD_CANDIDATES = saved[0]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])


WG4_LAYERS = [
    # (name, B, Cin, Cout, H, W, kernel, stride, dilation, padding, reflect, in_slope)
    ('ffn w1 256->1024 k3', 16, 256, 1024, 1, 400, (1, 3), (1, 1), (1, 1), (0, 1), False, 1.0),
    ('ffn w2 1024->256 k3 T100', 16, 1024, 256, 1, 100, (1, 3), (1, 1), (1, 1), (0, 1), False, 1.0),
    ('gen rb0 k11 d5 C256', 16, 256, 256, 1, 240, (1, 11), (1, 1), (1, 5), (0, 25), False, 0.1),
    ('gen rb1 k7 d3 C128', 16, 128, 128, 1, 1200, (1, 7), (1, 1), (1, 3), (0, 9), False, 0.1),
    ('gen rb2 k3 d1 C64', 16, 64, 64, 1, 6000, (1, 3), (1, 1), (1, 1), (0, 1), False, 0.1),
    ('mpd p7 conv4 512->512 s1', 16, 512, 512, 22, 7, (5, 1), (1, 1), (1, 1), (2, 0), False, 0.2),
]


@pytest.mark.parametrize('variant', [4, 5, 6])
def test_wgrad_fourth_generation_matches_pytorch(variant):
    """fourth generation of the bf16 weight gradient (wgrad4.inc: LDS-DMA ring of three / two / four pixel-tile stages)
    forced through the descriptor on the layer families it serves, against PyTorch; bit-reproducible like the third"""
    from msmctts_amd.hip import conv, lib
    saved = (conv._WGRAD_CANDIDATES, dict(conv.TUNED))
    conv._WGRAD_CANDIDATES = ((variant, 0),)
    try:
        for case in WG4_LAYERS:
            conv.TUNED.clear()
            conv._PLANS.clear()
            check_conv_case((case[0] + ' v%d' % variant,) + tuple(case[1:]), torch.bfloat16, 2e-2, DEV, parts=('wgrad',))
        name, B, Cin, Cout, H, W, k, s, dil, pad, reflect, slope = WG4_LAYERS[3]
        geom = conv.Geometry(H, W, k, s, dil, pad, reflect)
        x = torch.randn(B, H, W, Cin, device=DEV).bfloat16()
        g = torch.randn(B, geom.Hout, geom.Wout, Cout, device=DEV).bfloat16()
        outs = []
        for _ in range(3):
            dw, db = torch.zeros(k[0] * k[1], Cout, Cin, device=DEV), torch.zeros(Cout, device=DEV)
            conv.conv_wgrad(x, g, geom, k[0] * k[1], in_slope=slope, dw=dw, db=db)
            outs.append((dw, db))
        assert b'conv_wgrad4_kernel' in lib.get().msmc_conv_last_kernel()
        assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    finally:
        conv._WGRAD_CANDIDATES = saved[0]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])


def test_seventh_generation_gather_with_channel_counts_that_end_inside_a_chunk():
    """gather7.inc with Cin = 64 m + 8 t for every tail length t = 1 .. 7 (the pieces of the last 64-channel chunk past Cin come
    from the zero page on both operand sides), forward and data gradient, every variant that takes the layer, against PyTorch"""
    from msmctts_amd.hip import conv
    from _convcases import conv_case_data
    saved = (conv._GATHER_CANDIDATES, dict(conv.TUNED), conv.TUNE_BORROW)
    conv.TUNE_BORROW = False
    bad, ran = [], 0
    try:
        for ci, co, k, T in ((72, 128, 3, 300), (80, 136, 3, 100), (88, 64, 5, 500), (168, 128, 3, 200), (104, 256, 7, 150),
                             (112, 128, 3, 90), (248, 120, 3, 400), (600, 192, 3, 128)):
            case = ('g7 tail %d->%d k%d T%d' % (ci, co, k, T), 4, ci, co, 1, T, (1, k), (1, 1), (1, 1), (0, k // 2), False, 0.1 if k == 5 else 1.0)
            data = conv_case_data(case, torch.bfloat16, DEV)
            for v in (56, 59, 60, 61, 63):
                errs, n = _forced('gather', (v, 0), data, ('fwd', 'dgrad'), conv)
                ran += n
                bad.extend((case[0], v, part, e) for part, e in errs.items() if not e < 2e-2)
    finally:
        conv._GATHER_CANDIDATES, conv.TUNE_BORROW = saved[0], saved[2]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])
    assert not bad, bad[:20]
    assert ran >= 30, ran


def test_wgrad_fourth_generation_with_channel_counts_that_end_inside_a_tile():
    """wgrad4.inc (variants 4 / 5 / 6) with channel counts 64 m + 8 t on either side, t = 1 .. 7: the pieces past the last channel read
    the zero chunk, their rows / columns of dW and db are not stored; against PyTorch, model split and one split"""
    from msmctts_amd.hip import conv, lib
    from _convcases import conv_case_data
    L = lib.get()
    saved = (conv._WGRAD_CANDIDATES, dict(conv.TUNED), conv.TUNE_BORROW)
    conv.TUNE_BORROW = False
    bad, ran = [], 0
    try:
        for split in (0, 1):
            L.msmc_conv_set_wgrad_split(split)
            for ci, co, k, T in ((72, 128, 3, 300), (128, 80, 3, 100), (88, 104, 5, 500), (168, 120, 1, 200), (112, 248, 7, 150), (600, 72, 3, 128)):
                case = ('w4 tail %d->%d k%d T%d' % (ci, co, k, T), 4, ci, co, 1, T, (1, k), (1, 1), (1, 1), (0, k // 2), False, 0.1 if k == 5 else 1.0)
                data = conv_case_data(case, torch.bfloat16, DEV)
                for v in (4, 5, 6):
                    errs, n = _forced('wgrad', (v, 0), data, ('wgrad',), conv)
                    ran += n
                    bad.extend((case[0], v, split, part, e) for part, e in errs.items() if not e < 2e-2)
    finally:
        L.msmc_conv_set_wgrad_split(0)
        conv._WGRAD_CANDIDATES, conv.TUNE_BORROW = saved[0], saved[2]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])
    assert not bad, bad[:20]
    assert ran >= 30, ran


def test_wgrad_128_channel_tiles_every_step_count_and_ring_depth():
    """wgrad7.inc (descriptor variant 9) forced on layers that walk every code path of its tile loop on the hardware: 4 to 8
    sixteen-pixel steps per tile (T = 64 .. 128), ring depths 2 and 3, one to four taps per workgroup and two or three tap
    groups (k = 1, 2, 3, 5, 7, 11 with dilation), several tiles per workgroup (the ring wraps), channel counts that end
    inside a tile, input activation, bias -- against PyTorch fp32, model split and one split.  (The first form of this kernel
    spilled registers and was wrong on the GPU for 7 steps x 3 taps only, while the interpreter passed.)"""
    from msmctts_amd.hip import conv, lib
    from _convcases import conv_case_data
    L = lib.get()
    saved = (conv._WGRAD_CANDIDATES, dict(conv.TUNED), conv.TUNE_BORROW)
    conv.TUNE_BORROW = False
    bad, ran = [], 0
    try:
        for split in (0, 1):
            L.msmc_conv_set_wgrad_split(split)
            for T in (64, 70, 96, 100, 112, 128, 200, 400):
                for k, dil, ci, co, slope in ((3, 1, 128, 128, 1.0), (1, 1, 256, 136, 1.0), (2, 1, 128, 256, 0.1), (5, 2, 136, 128, 0.2),
                                              (7, 1, 128, 128, 0.0), (11, 5, 128, 128, 0.1)):
                    if split == 1 and T > 128 and k > 5:
                        continue                                   # (one workgroup column walking every tile: keep the sweep short)
                    span = dil * (k - 1)
                    case = ('w7 T%d k%d d%d %d->%d' % (T, k, dil, ci, co), 4, ci, co, 1, T, (1, k), (1, 1), (1, dil), (0, span // 2), False, slope)
                    data = conv_case_data(case, torch.bfloat16, DEV)
                    errs, n = _forced('wgrad', (9, 0), data, ('wgrad',), conv)
                    ran += n
                    bad.extend((case[0], split, part, e) for part, e in errs.items() if not e < 2e-2)
    finally:
        L.msmc_conv_set_wgrad_split(0)
        conv._WGRAD_CANDIDATES, conv.TUNE_BORROW = saved[0], saved[2]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])
    assert not bad, bad[:20]
    assert ran >= 60, ran


def test_wgrad_fourth_generation_grouped_matches_single_launches():
    """msmc_conv_wgrad_group_ws4(group4 = 1) on the three parallel ResBlock convolutions of a generator stage (k = 3, 7,
    11: one shared grid, the widest member sets the accumulator budget) against one launch per member"""
    import ctypes
    from msmctts_amd.hip import conv, lib
    L = lib.get()
    torch.manual_seed(0)
    B, C, Lx = 16, 128, 1200
    x = torch.randn(B, 1, Lx, C, device=DEV).bfloat16()
    descs, gs, refs, outs = [], [], [], []
    for k, dil in ((3, 1), (7, 3), (11, 1)):
        geom = conv.Geometry(1, Lx, (1, k), (1, 1), (1, dil), (0, dil * (k - 1) // 2), False)
        g = torch.randn(B, 1, Lx, C, device=DEV).bfloat16()
        d = conv._build_desc(x.dtype, B, 1, Lx, C, 1, Lx, C, geom.fwd_lattice, geom.fwd_taps, 0, 0.1, 1.0, 1.0, 1.0)
        d.x = d.w = d.out = x.data_ptr()
        d.variant, d.dw_copies = 4, 1
        need = L.msmc_conv_wgrad_workspace(ctypes.byref(d), g.data_ptr())
        ws = torch.zeros(max(1, need // 4), device=DEV)
        dw_ref, db_ref = torch.zeros(k, C, C, device=DEV), torch.zeros(C, device=DEV)
        assert L.msmc_conv_wgrad_ws(ctypes.byref(d), g.data_ptr(), dw_ref.data_ptr(), db_ref.data_ptr(), ws.data_ptr(),
                                    need, lib.stream(x)) == 0
        descs.append(d); gs.append(g); refs.append((dw_ref, db_ref))
        outs.append((torch.zeros(k, C, C, device=DEV), torch.zeros(C, device=DEV)))
    arr = (lib.ConvDesc * 3)(*descs)
    vp = ctypes.c_void_p * 3
    need = sum(L.msmc_conv_wgrad_workspace(ctypes.byref(d), g.data_ptr()) for d, g in zip(descs, gs))
    ws = torch.zeros(max(1, need // 4), device=DEV)
    rc = L.msmc_conv_wgrad_group_ws4(arr, vp(*[g.data_ptr() for g in gs]), vp(*[o[0].data_ptr() for o in outs]),
                                     vp(*[o[1].data_ptr() for o in outs]), 3, ws.data_ptr(), need, lib.stream(x), 1)
    assert rc == 0 and b'conv_wgrad4_group_kernel' in L.msmc_conv_last_kernel()
    torch.cuda.synchronize()
    for (dw_ref, db_ref), (dw, db) in zip(refs, outs):
        assert rel(dw, dw_ref) < 1e-4 and rel(db, db_ref) < 1e-4


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 2e-4), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize('Cin,Cout,k,u,L', [(512, 256, 12, 6, 40), (256, 128, 11, 5, 240), (128, 64, 11, 5, 1200),
                                            (64, 32, 4, 2, 6000)])
def test_conv_transpose(Cin, Cout, k, u, L, dtype, tol):
    from msmctts_amd.hip import conv
    B, p = 16, (k - u) // 2
    g = torch.Generator(device='cpu').manual_seed(Cin + k)
    x = torch.randn(B, Cin, L, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(Cin, Cout, k, generator=g) / (Cin * k / u) ** 0.5).to(DEV).requires_grad_(True)
    b = torch.randn(Cout, generator=g).to(DEV)
    ref = F.conv_transpose1d(F.leaky_relu(x, 0.1), w, b, u, p)
    go = torch.randn(ref.shape, generator=g).to(DEV)
    ref.backward(go)
    xc = x.detach().permute(0, 2, 1).unsqueeze(1).contiguous().to(dtype)
    gc = go.permute(0, 2, 1).unsqueeze(1).contiguous().to(dtype)
    wf = w.detach().permute(2, 1, 0).contiguous().to(dtype)
    wb = w.detach().permute(2, 0, 1).contiguous().to(dtype)
    out = conv.conv_transpose1d_forward(xc, wf, k, u, p, bias=b, in_slope=0.1)
    assert rel(out.squeeze(1).permute(0, 2, 1), ref) < tol
    gx = conv.conv_transpose1d_dgrad(gc, wb, k, u, p, L, mask_src=xc, mask_slope=0.1)
    assert rel(gx.squeeze(1).permute(0, 2, 1), x.grad) < tol
    dw = conv.conv_transpose1d_wgrad(xc, gc, k, u, p, in_slope=0.1)
    assert rel(dw, w.grad.permute(2, 0, 1)) < max(tol, 1e-3)


def test_generator_and_discriminator_full_size_vs_oracle_ops():
    """CSMSC-size HifiGAN generator + discriminator through the HIP stacks (fp32) against the same
    network evaluated with PyTorch-ROCm convolutions (oracle.model functions on the GPU)."""
    from msmctts_amd.configs import csmsc_config
    from msmctts_amd.networks import find_modules
    from oracle.model import discriminator_forward, hifigan_generator
    cfg = csmsc_config()['task']
    torch.manual_seed(0)
    nets = dict(find_modules({k: v for k, v in cfg.items() if k[:1] != '_'}))
    gen, disc = nets['autoencoder'].decoder.to(DEV), nets['discriminator'].to(DEV)
    x = torch.randn(4, 256, 40, device=DEV)
    P = {'autoencoder.decoder.' + k: v.detach() for k, v in gen.state_dict().items()}
    P.update({'discriminator.' + k: v.detach() for k, v in disc.state_dict().items()})
    wav = gen(x)
    ref = hifigan_generator(P, 'autoencoder.decoder', x, cfg['autoencoder']['decoder_config'])
    assert (wav - ref).abs().max().item() < 1e-3
    scores, fmaps = disc(wav.detach())
    rs, rf = discriminator_forward(P, cfg['discriminator'], wav.detach())
    for a, b in zip(scores, rs):
        assert (a.float() - b).abs().max().item() < 1e-3
    for fa, fb in zip(fmaps, rf):
        for a, b in zip(fa, fb):
            assert a.shape == b.shape and (a.float() - b).abs().max().item() < 1e-3


@pytest.mark.parametrize('hop', [15, 30, 50, 120, 240])
def test_mrd_spectral_front_end_full_size(hop):
    """HIP framed-DFT front-end (B=16, L=12000) against the torch.stft-based oracle on the same device:
    image within 1e-4, gradient wrt the waveform within 1e-3 of its scale."""
    from msmctts_amd.utils.audio import TorchSTFT
    from oracle import audio
    g = torch.Generator().manual_seed(hop)
    x = (torch.rand(16, 12000, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    st = TorchSTFT(fft_size=4 * hop, hop_size=hop, win_size=4 * hop, normalized=True, domain='double', mel_scale=True)
    img = st.image_cl(x)
    xo = x.detach().clone().requires_grad_(True)
    ref = audio.mrd_spectrogram(xo, hop)                       # (B, 2, F, T)
    assert (img.permute(0, 3, 1, 2) - ref).abs().max().item() < 1e-4
    go = torch.randn(ref.shape, generator=g).to(DEV)
    ref.backward(go)
    img.backward(go.permute(0, 2, 3, 1).contiguous())
    assert (x.grad - xo.grad).abs().max().item() < 1e-3 * max(1.0, xo.grad.abs().max().item())


def test_mel_loss_full_size():
    from msmctts_amd.trainers.criterions.stft_loss import MelLoss
    from oracle import audio
    g = torch.Generator().manual_seed(1)
    a = (torch.rand(16, 12000, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    b = (torch.rand(16, 12000, generator=g) * 2 - 1).to(DEV)
    ml = MelLoss(fft_size=2048, hop_size=300, win_size=1200, sample_rate=24000, num_mels=128)
    loss = ml(a, b)
    ao = a.detach().clone().requires_grad_(True)
    ref = audio.mel_loss(ao, b)
    assert abs(loss.item() - ref.item()) < 1e-4
    loss.backward()
    ref.backward()
    assert (a.grad - ao.grad).abs().max().item() < 1e-3 * max(1e-6, ao.grad.abs().max().item()) + 1e-9


def test_autotune_picks_a_variant_and_every_variant_is_correct():
    """first launch of a layer shape times the candidate kernels (descriptor.variant / split_shift) and keeps one;
    every candidate, forced, matches PyTorch"""
    from msmctts_amd.hip import conv
    case = CONVS[2]                                   # gen rb1 k7 d3 C128
    check_conv_case(case, torch.bfloat16, 2e-2, DEV)
    kinds = {k[0] for k in conv.TUNED}
    assert {'gather', 'wgrad'} <= kinds
    allowed = {'gather': {v for v, _ in conv._GATHER_CANDIDATES}, 'wgrad': {v for v, _ in conv._WGRAD_CANDIDATES}}
    assert all(v[0] in allowed[k[0]] and len(v[2]) >= 2 for k, v in conv.TUNED.items() if k[0] in ('gather', 'wgrad'))
    saved = (conv._GATHER_CANDIDATES, conv._WGRAD_CANDIDATES, dict(conv.TUNED))
    try:
        for gv in conv._GATHER_CANDIDATES:
            for wv in conv._WGRAD_CANDIDATES:
                conv.TUNED.clear()
                conv._GATHER_CANDIDATES, conv._WGRAD_CANDIDATES = (gv,), (wv,)
                name, B, Cin, Cout, H, W, k, s, dil, pad, reflect, slope = case
                fresh = (name + ' %s %s' % (gv, wv), B, Cin, Cout, H + 0, W, k, s, dil, pad, reflect, slope)
                conv_geom_cache_reset = getattr(conv, '_PLANS')
                conv_geom_cache_reset.clear()
                check_conv_case(fresh, torch.bfloat16, 2e-2, DEV)
    finally:
        conv._GATHER_CANDIDATES, conv._WGRAD_CANDIDATES = saved[0], saved[1]
        conv.TUNED.clear()
        conv.TUNED.update(saved[2])


def test_grouped_launches_equal_single_launches():
    """msmc_conv_gather_group / msmc_conv_wgrad_group against one launch per member (forward, strided data gradient with
    several phases, weight / bias gradients).  Members of a group run the leader's kernel instantiation, whose fp32
    accumulation order over (channel chunk, tap) can differ from a member's own tuned kernel: equal to bf16 rounding."""
    from msmctts_amd.hip import conv, lib
    torch.manual_seed(0)
    B, C, L = 4, 64, 700
    x = torch.randn(B, 1, L, C, device=DEV).bfloat16()
    items, refs = [], []
    for k, dil in ((3, 1), (7, 3), (11, 1)):
        geom = conv.Geometry(1, L, (1, k), (1, 1), (1, dil), (0, dil * (k - 1) // 2), False)
        w = (torch.randn(k, C, C, device=DEV) / (C * k) ** 0.5).bfloat16()
        b = torch.randn(C, device=DEV)
        res = torch.randn(B, 1, L, C, device=DEV).bfloat16()
        items.append(dict(x=x, w=w, geom=geom, bias=b, in_slope=0.1, res=res))
        refs.append(conv.conv_forward(x, w, geom, bias=b, in_slope=0.1, res=res))
    L0 = lib.get()
    for grouping in (1, 0):
        L0.msmc_conv_set_grouping(grouping)
        try:
            saved = dict(conv.TUNED)
            conv.TUNED.update({k: (1, 0, v[2]) for k, v in conv.TUNED.items() if k[0].endswith('-group')})
            outs = conv.conv_forward_group(items)
        finally:
            L0.msmc_conv_set_grouping(1)
        for o, r in zip(outs, refs):
            assert rel(o, r) < 1e-2
    gitems, grefs = [], []
    for k, s_ in ((5, 3), (5, 1)):
        H, W, Ci, Co = 300, 3, 16, 64
        geom = conv.Geometry(H, W, (k, 1), (s_, 1), (1, 1), (2, 0), False)
        g = torch.randn(B, geom.Hout, geom.Wout, Co, device=DEV).bfloat16()
        wb = (torch.randn(k, Ci, Co, device=DEV) / (Co * k) ** 0.5).bfloat16()
        xm = torch.randn(B, H, W, Ci, device=DEV).bfloat16()
        gitems.append(dict(g=g, wb=wb, geom=geom, mask_src=xm, mask_slope=0.2))
        grefs.append(conv.conv_dgrad(g, wb, geom, mask_src=xm, mask_slope=0.2))
    for o, r in zip(conv.conv_dgrad_group(gitems), grefs):
        assert rel(o, r) < 1e-2
    witems, wrefs = [], []
    for k, dil in ((3, 1), (7, 3), (11, 1)):
        geom = conv.Geometry(1, L, (1, k), (1, 1), (1, dil), (0, dil * (k - 1) // 2), False)
        g = torch.randn(B, 1, L, C, device=DEV).bfloat16()
        dw_ref, db_ref = torch.zeros(k, C, C, device=DEV), torch.zeros(C, device=DEV)
        conv.conv_wgrad(x, g, geom, k, in_slope=0.1, dw=dw_ref, db=db_ref)
        dw, db = torch.zeros(2, k, C, C, device=DEV), torch.zeros(2, C, device=DEV)
        witems.append(dict(x=x, g=g, geom=geom, n_slices=k, in_slope=0.1, dw=dw.view(-1), db=db.view(-1), copies=2))
        wrefs.append((dw_ref, db_ref, dw, db))
    conv.conv_wgrad_group(witems)
    for dw_ref, db_ref, dw, db in wrefs:
        assert rel(dw.sum(0), dw_ref) < 1e-4 and rel(db.sum(0), db_ref) < 1e-4


def _forced(kind, variant_shift, data, parts, conv):
    """run ``parts`` of a prepared case with ONE candidate forced through the tuner; returns (errors, ran) where ``ran``
    counts the descriptors that really executed the candidate (a candidate outside its scope returns MSMC_E_SHAPE at the
    validation launch and the library heuristic runs instead -- that proves nothing about the candidate)"""
    conv.TUNED.clear()
    conv._PLANS.clear()
    conv._CLASS_INDEX.clear()
    conv._CLASS_INDEXED[0] = -1
    if kind == 'gather':
        conv._GATHER_CANDIDATES = (variant_shift,)
    else:
        conv._WGRAD_CANDIDATES = (variant_shift,)
    errs = {}
    for part in parts:
        errs.update(conv_part_errors(data, part))
    ran = sum(1 for k, v in conv.TUNED.items() if k[0] == kind and (v[0], v[1]) == tuple(variant_shift) and v[2])
    return errs, ran


@pytest.mark.parametrize('family', ['gen', 'mpd', 'mrd', 'fft'])
def test_every_gather_candidate_forced_on_every_csmsc_layer(family):
    """No forward / data-gradient kernel reaches hip/tuned_gfx950.json without a direct hardware test: every tuner
    candidate (msmc_conv_desc.variant, hip/conv.py _GATHER_CANDIDATES: generations 1-2, direct, wave-split, third
    generation 16-23, LDS-DMA halo 24-31, persistent thin-layer 32) is FORCED on every convolution shape of the CSMSC
    generator / period / resolution discriminators it accepts, forward and data gradient, against PyTorch fp32 (2e-2,
    bf16).  Shapes outside a candidate's scope are skipped (MSMC_E_SHAPE); each candidate must have run somewhere in
    the model (asserted over the three families in test_every_candidate_ran_somewhere)."""
    from msmctts_amd.hip import conv
    from _convcases import conv_case_data, conv_part_errors, csmsc_layers
    saved = (conv._GATHER_CANDIDATES, dict(conv.TUNED), conv.TUNE_BORROW)
    conv.TUNE_BORROW = False            # time (= force) the one candidate on every shape, never borrow a neighbour's choice
    bad = []
    try:
        for case in csmsc_layers()[family]:
            data = conv_case_data(case, torch.bfloat16, DEV)
            for cand in saved[0]:
                errs, ran = _forced('gather', cand, data, ('fwd', 'dgrad'), conv)
                _RAN[('gather', cand)] = _RAN.get(('gather', cand), 0) + ran
                bad.extend((case[0], cand, part, e) for part, e in errs.items() if not e < 2e-2)
    finally:
        conv._GATHER_CANDIDATES, conv.TUNE_BORROW = saved[0], saved[2]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])
    assert not bad, bad[:20]


@pytest.mark.parametrize('family', ['gen', 'mpd', 'mrd', 'fft'])
def test_every_wgrad_candidate_forced_on_every_csmsc_layer(family):
    """the same for the weight (+ bias) gradient candidates (_WGRAD_CANDIDATES: generations 1-4 with their pixel-split
    shifts and the general-lattice LDS-DMA generation, variant 7) -- in particular variant 7 on every stride-3
    period-discriminator layer and every reflect-padded 3x3 resolution-discriminator layer with channel counts it takes"""
    from msmctts_amd.hip import conv
    from _convcases import conv_case_data, conv_part_errors, csmsc_layers
    saved = (conv._WGRAD_CANDIDATES, dict(conv.TUNED), conv.TUNE_BORROW)
    conv.TUNE_BORROW = False
    bad = []
    try:
        for case in csmsc_layers()[family]:
            data = conv_case_data(case, torch.bfloat16, DEV)
            for cand in saved[0]:
                errs, ran = _forced('wgrad', cand, data, ('wgrad',), conv)
                _RAN[('wgrad', cand)] = _RAN.get(('wgrad', cand), 0) + ran
                if cand[0] == 7 and ran:
                    _RAN.setdefault('wgrad5 layers', []).append(case[0])
                bad.extend((case[0], cand, part, e) for part, e in errs.items() if not e < 2e-2)
    finally:
        conv._WGRAD_CANDIDATES, conv.TUNE_BORROW = saved[0], saved[2]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])
    assert not bad, bad[:20]


_RAN = {}


def test_every_candidate_ran_somewhere():
    """(after the two sweeps above, same process) every tuner candidate executed on at least one CSMSC layer; the
    general-lattice weight gradient on all twenty strided / reflected discriminator layers with C % 64 == 0"""
    from msmctts_amd.hip import conv
    if not any(k[0] == 'gather' for k in _RAN if isinstance(k, tuple)):
        pytest.skip('the sweeps did not run in this session')
    missing = [k for k in [('gather', c) for c in conv._GATHER_CANDIDATES] + [('wgrad', c) for c in conv._WGRAD_CANDIDATES]
               if not _RAN.get(k)]
    assert not missing, missing
    if (7, 0) in conv._WGRAD_CANDIDATES:
        layers = set(_RAN.get('wgrad5 layers', []))
        want = {c[0] for fam in ('mpd', 'mrd') for c in csmsc_layers_cached()[fam]
                if c[2] % 64 == 0 and c[3] % 64 == 0 and (c[7] != (1, 1) or c[10])}
        assert want <= layers, sorted(want - layers)


def csmsc_layers_cached():
    from _convcases import csmsc_layers
    return csmsc_layers()


@pytest.mark.parametrize('g1v', [34, 35])
def test_one_tap_gemm_fp32_forced_on_the_spectral_shapes(g1v):
    """variants 34 / 35 (128 x 128 / 64 x 128 tiles) on fp32 (gemm1.inc, exact fp32 matrix-core multiplies): forced on the framed-DFT / mel-basis GEMM shapes
    of the spectral front-ends (STFT loss resolutions, resolution-discriminator spectrograms, mel projection), forward
    and data gradient, against PyTorch fp32 at 1e-5 of the output scale"""
    from msmctts_amd.hip import conv, lib
    from _convcases import conv_case_data
    cases = [('dft 1200->2052 T40', 16, 1200, 2052, 1, 40, (1, 1), (1, 1), (1, 1), (0, 0), False, 1.0),
             ('dft 960->964 T51', 32, 960, 964, 1, 51, (1, 1), (1, 1), (1, 1), (0, 0), False, 1.0),
             ('dft 480->484 T101', 16, 480, 484, 1, 101, (1, 1), (1, 1), (1, 1), (0, 0), False, 1.0),
             ('dft 200->204 T241', 16, 200, 204, 1, 241, (1, 1), (1, 1), (1, 1), (0, 0), False, 1.0),
             ('mel 1028->128 T40', 16, 1028, 128, 1, 40, (1, 1), (1, 1), (1, 1), (0, 0), False, 1.0)]
    saved = (conv._GATHER_CANDIDATES, dict(conv.TUNED), conv.TUNE_BORROW)
    conv.TUNE_BORROW = False
    bad = []
    try:
        for case in cases:
            data = conv_case_data(case, torch.float32, DEV)
            for part in ('fwd', 'dgrad'):
                errs, ran = _forced('gather', (g1v, 0), data, (part,), conv)
                assert ran == 1 and b'conv_gemm1_kernel<float' in lib.get().msmc_conv_last_kernel(), (case[0], part, ran)
                bad.extend((case[0], p_, e) for p_, e in errs.items() if not e < 1e-5)
    finally:
        conv._GATHER_CANDIDATES, conv.TUNE_BORROW = saved[0], saved[2]
        conv.TUNED.clear()
        conv.TUNED.update(saved[1])
    assert not bad, bad




def test_layer_applied_twice_keeps_its_two_weight_gradient_reductions_apart():
    """A layer applied TWICE in one backward pass (rb(rb(x)); D(real) and D(fake) as separate calls) has two recorded second
    stages with the same accumulator: msmc_conv_wgrad_reduce_pending must not put them into one launch (plain `dw += sum`
    read-modify-writes; round-3 advice).  A bf16 ResBlock at a size where the split-partials generations run, every layer
    twice: the weight gradients match the fp32 chain on the same (bf16-rounded) weights and are bit-identical run to run."""
    from msmctts_amd.hip import conv as K
    from msmctts_amd.networks.hifigan.common import ResBlock1
    torch.manual_seed(12)
    rb = ResBlock1(64, 3, (1, 3, 5)).to(DEV)
    rb.hip_dtype = torch.bfloat16
    x = torch.randn(8, 64, 3000, device=DEV)
    go = torch.randn(8, 64, 3000, device=DEV)
    runs = []
    # the no-atomics generation (split partials + second stage) on every layer: the tuner may only pick variant 3 here (the
    # atomic generations are not reproducible run to run by construction, and they have no second stage to merge)
    keep = (dict(K.TUNED), K._WGRAD_CANDIDATES, K.TUNE_BORROW)
    K.TUNED.clear()
    K._WGRAD_CANDIDATES, K.TUNE_BORROW = ((3, 0),), False
    try:
        for _ in range(9):
            rb.zero_grad()
            xi = x.clone().requires_grad_(True)
            y = rb(rb(xi))
            (y.float() * go).sum().backward()
            torch.cuda.synchronize()
            runs.append({n: p.grad.detach().clone() for n, p in rb.named_parameters()})
        assert rb._bank.deferred.chunks, 'no split weight gradient ran: the test does not exercise the deferred second stage'
        # (hip/convnet.py ConvBank._drop_idle_copies: these layers only ever ran the no-atomics generation, so their privatised
        #  accumulator copies were dropped after a few passes -- the gradients before and after must be the same bits)
        assert all(l.dw_copies == 1 for l in rb._bank.layers), [l.dw_copies for l in rb._bank.layers]
    finally:
        K.TUNED.clear()
        K.TUNED.update(keep[0])
        K._WGRAD_CANDIDATES, K.TUNE_BORROW = keep[1], keep[2]
    for n in runs[0]:
        assert all(torch.equal(runs[0][n], r[n]) for r in runs[1:]), 'gradient of %s differs run to run' % n
    # fp32 chain on the same weights
    rb.zero_grad()
    xr = x.clone().requires_grad_(True)
    h = xr
    for _ in range(2):
        for c1, c2 in zip(rb.convs1, rb.convs2):
            t_ = F.conv1d(F.leaky_relu(h, 0.1), c1.weight(), c1.bias, 1, c1.padding, c1.dilation)
            h = F.conv1d(F.leaky_relu(t_, 0.1), c2.weight(), c2.bias, 1, c2.padding, c2.dilation) + h
    (h * go).sum().backward()
    for n, p in rb.named_parameters():
        want, got = p.grad.float(), runs[0][n].float()
        err = ((got - want).norm() / want.norm()).item()
        assert err <= 8e-2, 'gradient of %s: relative L2 error %.3e against the fp32 chain' % (n, err)     # (bf16 through 24 convolutions; a lost accumulation is an error of order 0.5)
