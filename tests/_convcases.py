"""Convolution layer cases shared by the GPU tests (full CSMSC sizes) and the kernel-interpreter tests
(same layer geometry, fewer pixels): every check compares the HIP kernels with PyTorch's own convolution."""
import torch
import torch.nn.functional as F


def cl(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


def rel(a, b):
    return (a.float() - b.float()).abs().max().item() / max(1e-6, b.float().abs().max().item())


# (name, B, Cin, Cout, H, W, kernel, stride, dilation, padding, reflect, in_slope)
CONVS = [
    ('gen conv_pre k7', 16, 256, 512, 1, 40, (1, 7), (1, 1), (1, 1), (0, 3), False, 1.0),
    ('gen rb0 k11 d5 C256', 16, 256, 256, 1, 240, (1, 11), (1, 1), (1, 5), (0, 25), False, 0.1),
    ('gen rb1 k7 d3 C128', 16, 128, 128, 1, 1200, (1, 7), (1, 1), (1, 3), (0, 9), False, 0.1),
    ('gen rb2 k3 d1 C64', 16, 64, 64, 1, 6000, (1, 3), (1, 1), (1, 1), (0, 1), False, 0.1),
    ('gen rb3 k11 d1 C32', 8, 32, 32, 1, 12000, (1, 11), (1, 1), (1, 1), (0, 5), False, 0.1),
    ('gen conv_post k7 C32->1', 16, 32, 1, 1, 12000, (1, 7), (1, 1), (1, 1), (0, 3), False, 0.01),
    ('mpd p2 conv0 1->16', 16, 1, 16, 6000, 2, (5, 1), (3, 1), (1, 1), (2, 0), False, 1.0),
    ('mpd p3 conv1 16->64', 16, 16, 64, 1334, 3, (5, 1), (3, 1), (1, 1), (2, 0), False, 0.2),
    ('mpd p11 conv2 64->256', 16, 64, 256, 122, 11, (5, 1), (3, 1), (1, 1), (2, 0), False, 0.2),
    ('mpd p5 conv3 256->512', 16, 256, 512, 89, 5, (5, 1), (3, 1), (1, 1), (2, 0), False, 0.2),
    ('mpd p7 conv4 512->512 s1', 16, 512, 512, 22, 7, (5, 1), (1, 1), (1, 1), (2, 0), False, 0.2),
    ('mpd p2 post 512->1', 16, 512, 1, 75, 2, (3, 1), (1, 1), (1, 1), (1, 0), False, 0.2),
    ('mrd h15 conv0 2->4 s1', 16, 2, 4, 31, 801, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0),
    ('mrd h15 conv1 4->8 s2', 16, 4, 8, 31, 801, (3, 3), (2, 2), (1, 1), (1, 1), True, 1.0),
    ('mrd h240 conv3 64->128 s2', 16, 64, 128, 241, 26, (3, 3), (2, 2), (1, 1), (1, 1), True, 1.0),
    ('mrd h240 conv4 128->256 s1', 16, 128, 256, 121, 13, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0),
    ('mrd h240 conv6 512->1', 16, 512, 1, 61, 7, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0),
]

# the same geometries with few pixels / channels (the interpreter runs one work-item at a time), plus the
# thin and odd channel counts of the first discriminator layers
SMALL = [
    ('gen k11 d5 C64', 2, 64, 64, 1, 70, (1, 11), (1, 1), (1, 5), (0, 25), False, 0.1),
    ('gen k7 d3 C32', 2, 32, 32, 1, 150, (1, 7), (1, 1), (1, 3), (0, 9), False, 0.1),
    ('gen k3 C96->40', 1, 96, 40, 1, 40, (1, 3), (1, 1), (1, 1), (0, 1), False, 0.1),
    ('gen post C32->1', 2, 32, 1, 1, 140, (1, 7), (1, 1), (1, 1), (0, 3), False, 0.01),
    ('mpd 1->16', 2, 1, 16, 61, 2, (5, 1), (3, 1), (1, 1), (2, 0), False, 1.0),
    ('mpd 16->64 p3', 2, 16, 64, 40, 3, (5, 1), (3, 1), (1, 1), (2, 0), False, 0.2),
    ('mpd 64->1 p5', 1, 64, 1, 9, 5, (3, 1), (1, 1), (1, 1), (1, 0), False, 0.2),
    ('mrd 2->4 s1', 2, 2, 4, 9, 37, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0),
    ('mrd 4->8 s2', 2, 4, 8, 9, 37, (3, 3), (2, 2), (1, 1), (1, 1), True, 1.0),
    ('mrd 8->16 s1', 1, 8, 16, 11, 21, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0),
    ('mrd 64->72 s2', 1, 64, 72, 13, 18, (3, 3), (2, 2), (1, 1), (1, 1), True, 1.0),
    # inputs smaller than the receptive field / the reflection border
    ('tiny L3 k11 d5', 1, 32, 32, 1, 3, (1, 11), (1, 1), (1, 5), (0, 25), False, 0.1),
    ('tiny 2x2 reflect 4->8', 1, 4, 8, 2, 2, (3, 3), (1, 1), (1, 1), (1, 1), True, 1.0),
    ('tiny 3x2 reflect 64->64 s2', 2, 64, 64, 3, 2, (3, 3), (2, 2), (1, 1), (1, 1), True, 1.0),
]


def csmsc_layers(B=16):
    """Every convolution layer shape of the CSMSC model's HifiGAN generator, period and resolution discriminators
    (40-frame window = 12000 samples), as CONVS-style cases keyed by family."""
    out = {'gen': [], 'mpd': [], 'mrd': [], 'fft': []}
    # kernel-size-1 layers of the FFT blocks / quantiser glue (T = 400 and T / 4): Q|K|V and output projections, 1x1 stacks
    for T in (400, 100):
        for ci, co in ((256, 384), (128, 256), (256, 256), (512, 256), (80, 256), (256, 80)):
            out['fft'].append(('fft 1x1 T%d %d->%d' % (T, ci, co), B, ci, co, 1, T, (1, 1), (1, 1), (1, 1), (0, 0), False, 1.0))
    out['fft'].append(('fft ffn k3 256->1024', B, 256, 1024, 1, 400, (1, 3), (1, 1), (1, 1), (0, 1), False, 1.0))
    out['fft'].append(('fft ffn k3 1024->256 relu', B, 1024, 256, 1, 400, (1, 3), (1, 1), (1, 1), (0, 1), False, 0.0))
    # the 600 / 1536-wide feed-forward layers of the predictor's FFT blocks (configs.am_config): channel counts that end inside a tile of 64
    out['fft'].append(('am ffn k3 600->1536', B, 600, 1536, 1, 100, (1, 3), (1, 1), (1, 1), (0, 1), False, 1.0))
    out['fft'].append(('am ffn k3 1536->600 relu', B, 1536, 600, 1, 100, (1, 3), (1, 1), (1, 1), (0, 1), False, 0.0))
    out['gen'].append(('gen conv_pre k7 256->512', B, 256, 512, 1, 40, (1, 7), (1, 1), (1, 1), (0, 3), False, 1.0))
    for C, L in ((256, 240), (128, 1200), (64, 6000), (32, 12000)):
        for k in (3, 7, 11):
            for d in (1, 3, 5):
                out['gen'].append(('gen rb C%d L%d k%d d%d' % (C, L, k, d), B, C, C, 1, L, (1, k), (1, 1), (1, d),
                                   (0, d * (k - 1) // 2), False, 0.1))
    out['gen'].append(('gen conv_post k7 32->1', B, 32, 1, 1, 12000, (1, 7), (1, 1), (1, 1), (0, 3), False, 0.01))
    for p in (2, 3, 5, 7, 11):
        H = -(-12000 // p)
        chans = (1, 16, 64, 256, 512)
        for i in range(4):
            out['mpd'].append(('mpd p%d conv%d %d->%d s3' % (p, i, chans[i], chans[i + 1]), B, chans[i], chans[i + 1], H, p,
                               (5, 1), (3, 1), (1, 1), (2, 0), False, 1.0 if i == 0 else 0.2))
            H = (H + 4 - 5) // 3 + 1
        out['mpd'].append(('mpd p%d conv4 512->512 s1' % p, B, 512, 512, H, p, (5, 1), (1, 1), (1, 1), (2, 0), False, 0.2))
        out['mpd'].append(('mpd p%d post 512->1' % p, B, 512, 1, H, p, (3, 1), (1, 1), (1, 1), (1, 0), False, 0.2))
    for hop, hidden in ((15, 128), (30, 128), (50, 256), (120, 256), (240, 512)):
        F_, T_ = 2 * hop + 1, 12000 // hop + 1
        chans = (2, hidden // 32, hidden // 16, hidden // 8, hidden // 4, hidden // 2, hidden, 1)
        for i, st in enumerate((1, 2, 1, 2, 1, 2, 1)):
            out['mrd'].append(('mrd h%d conv%d %d->%d s%d' % (hop, i, chans[i], chans[i + 1], st), B, chans[i], chans[i + 1],
                               F_, T_, (3, 3), (st, st), (1, 1), (1, 1), True, 1.0 if i == 0 else 0.2))
            F_, T_ = (F_ + 2 - 3) // st + 1, (T_ + 2 - 3) // st + 1
    return out


def conv_case_data(case, dtype, dev):
    """operands in the kernels' layouts and PyTorch's results (forward, data gradient, weight / bias gradient) of one
    layer: computed once per (case, dtype), checked against as many kernel variants as the caller forces"""
    name, B, Cin, Cout, H, W, k, s, dil, pad, reflect, slope = case
    g = torch.Generator(device='cpu').manual_seed(sum(ord(c) for c in name))
    x = torch.randn(B, Cin, H, W, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(Cout, Cin, *k, generator=g) / (Cin * k[0] * k[1]) ** 0.5).to(dev).requires_grad_(True)
    b = torch.randn(Cout, generator=g).to(dev).requires_grad_(True)
    xa = F.leaky_relu(x, slope) if slope != 1.0 else x
    if reflect:
        ref = F.conv2d(F.pad(xa, (pad[1], pad[1], pad[0], pad[0]), mode='reflect'), w, b, s, 0, dil)
    else:
        ref = F.conv2d(xa, w, b, s, pad, dil)
    go = torch.randn(ref.shape, generator=g).to(dev)
    ref.backward(go)
    T = k[0] * k[1]
    d = dict(case=case, dtype=dtype, T=T, ref=ref.detach(), gx_ref=x.grad, b=b.detach(),
             dw_ref=w.grad.permute(2, 3, 0, 1).reshape(T, Cout, Cin),
             wf=w.detach().permute(2, 3, 0, 1).reshape(T, Cout, Cin).contiguous().to(dtype),
             wb=w.detach().permute(2, 3, 1, 0).reshape(T, Cin, Cout).contiguous().to(dtype),
             xc=cl(x.detach()).to(dtype), gc=cl(go).to(dtype))
    d['db_ref'] = d['gc'].float().reshape(-1, Cout).sum(0)
    d['db_scale'] = d['gc'].float().reshape(-1, Cout).abs().sum(0).max().item()
    return d


def conv_part_errors(d, part):
    """relative error(s) of one part ('fwd' / 'dgrad' / 'wgrad') of a prepared case under the CURRENT kernel choices
    (a fresh Geometry per call: descriptors, and with them forced variants, are cached per geometry object)"""
    from msmctts_amd.hip import conv
    name, B, Cin, Cout, H, W, k, s, dil, pad, reflect, slope = d['case']
    geom = conv.Geometry(H, W, k, s, dil, pad, reflect)
    if part == 'fwd':
        out = conv.conv_forward(d['xc'], d['wf'], geom, bias=d['b'], in_slope=slope)
        return {'fwd': rel(nchw(out), d['ref'])}
    if part == 'dgrad':
        if reflect:
            gx = conv.reflect_fold(conv.conv_dgrad(d['gc'], d['wb'], geom), H, W, pad[0],
                                   mask_src=d['xc'] if slope != 1.0 else None, slope=slope)
        else:
            gx = conv.conv_dgrad(d['gc'], d['wb'], geom, mask_src=d['xc'] if slope != 1.0 else None, mask_slope=slope)
        return {'dgrad': rel(nchw(gx), d['gx_ref'])}
    db = torch.zeros(Cout, device=d['xc'].device)
    dw = conv.conv_wgrad(d['xc'], d['gc'], geom, d['T'], in_slope=slope, db=db)
    return {'wgrad': rel(dw, d['dw_ref']), 'bias grad': (db - d['db_ref']).abs().max().item() / (d['db_scale'] + 1e-6) * 1e3}


def check_conv_case(case, dtype, tol, dev, parts=('fwd', 'dgrad', 'wgrad'), batch_offset=0):
    """forward / data gradient / weight + bias gradient of one layer against PyTorch on ``dev``."""
    from msmctts_amd.hip import conv
    name, B, Cin, Cout, H, W, k, s, dil, pad, reflect, slope = case
    g = torch.Generator(device='cpu').manual_seed(sum(ord(c) for c in name))
    x = torch.randn(B, Cin, H, W, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(Cout, Cin, *k, generator=g) / (Cin * k[0] * k[1]) ** 0.5).to(dev).requires_grad_(True)
    b = torch.randn(Cout, generator=g).to(dev).requires_grad_(True)
    xa = F.leaky_relu(x, slope) if slope != 1.0 else x
    if reflect:
        ref = F.conv2d(F.pad(xa, (pad[1], pad[1], pad[0], pad[0]), mode='reflect'), w, b, s, 0, dil)
    else:
        ref = F.conv2d(xa, w, b, s, pad, dil)
    go = torch.randn(ref.shape, generator=g).to(dev)
    ref.backward(go)
    geom = conv.Geometry(H, W, k, s, dil, pad, reflect)
    T = k[0] * k[1]
    wf = w.detach().permute(2, 3, 0, 1).reshape(T, Cout, Cin).contiguous().to(dtype)
    wb = w.detach().permute(2, 3, 1, 0).reshape(T, Cin, Cout).contiguous().to(dtype)
    xc, gc = cl(x.detach()).to(dtype), cl(go).to(dtype)
    if batch_offset:
        # operands that start in the middle of a larger allocation at an element-aligned address are refused
        # loudly (the kernels use 16-byte vector accesses), not mis-read
        import pytest
        buf = torch.empty(xc.numel() + batch_offset, dtype=xc.dtype, device=xc.device)
        xo = buf[batch_offset:].view(xc.shape)
        xo.copy_(xc)
        with pytest.raises(ValueError, match='16-byte aligned'):
            conv.conv_forward(xo, wf, geom, bias=b.detach(), in_slope=slope)
        with pytest.raises(ValueError, match='16-byte aligned'):
            conv.conv_wgrad(xo, gc, geom, T, in_slope=slope)
    if 'fwd' in parts:
        out = conv.conv_forward(xc, wf, geom, bias=b.detach(), in_slope=slope)
        assert rel(nchw(out), ref) < tol, 'forward'
    if 'dgrad' in parts:
        if reflect:
            gx = conv.reflect_fold(conv.conv_dgrad(gc, wb, geom), H, W, pad[0],
                                   mask_src=xc if slope != 1.0 else None, slope=slope)
        else:
            gx = conv.conv_dgrad(gc, wb, geom, mask_src=xc if slope != 1.0 else None, mask_slope=slope)
        assert rel(nchw(gx), x.grad) < tol, 'dgrad'
    if 'wgrad' in parts:
        db = torch.zeros(Cout, device=dev)
        dw = conv.conv_wgrad(xc, gc, geom, T, in_slope=slope, db=db)
        want = w.grad.permute(2, 3, 0, 1).reshape(T, Cout, Cin)
        wtol = max(tol, 1e-3 if dtype == torch.float32 else tol)
        assert rel(dw, want) < wtol, ('wgrad', rel(dw, want))
        # the fused bias gradient sums exactly the (rounded) operand the kernel was given
        bref = gc.float().reshape(-1, Cout).sum(0)
        bscale = gc.float().reshape(-1, Cout).abs().sum(0).max().item()
        assert (db - bref).abs().max().item() < 1e-5 * bscale + 1e-6, ('fused bias grad', db, bref)
        # privatised accumulators: R copies back to back, workgroup i adds into copy i % R; their sum is dW
        R = 4
        dwR = torch.zeros(R, T, Cout, Cin, device=dev)
        dbR = torch.zeros(R, Cout, device=dev)
        conv.conv_wgrad(xc, gc, geom, T, in_slope=slope, dw=dwR.view(-1), db=dbR.view(-1), copies=R)
        assert rel(dwR.sum(0), want) < wtol, ('wgrad copies', rel(dwR.sum(0), want))
        assert (dbR.sum(0) - bref).abs().max().item() < 1e-5 * bscale + 1e-6, 'bias grad copies'
        cs = conv.colsum(gc.reshape(-1, Cout))
        assert (cs - bref).abs().max().item() < 1e-5 * bscale + 1e-6, ('bias grad', cs, bref)


# ---- grouped entry points with members of several kernel families in one call ---------------------------------------
# Launch count and launch log (kernel names in launch order) of the two calls below.  Both were recorded by running
# check_mixed_family_groups against the library built from the commit BEFORE the grouped launchers were unified into one
# routine per direction (that commit's kernel interpreter); they hold unchanged on the interpreter and on the device.
MIXED_FORWARD_LAUNCHES = 7
MIXED_FORWARD_KERNELS = ['conv_gather3_group_kernel<2, 1, 1, 3, false>', 'conv_gather3_kernel<4, 1, 1, 6, false>',
                         'conv_gather5_group_kernel<1, 1, 4, 1, 3>', 'conv_gather5_kernel<1, 1, 4, 1, 3>',
                         'conv_gather7_group_kernel<2, 2, 2, 1, 3>', 'conv_gather6_group_kernel<2>',
                         'conv_gather_ks_group_kernel<unsigned short, 2, 2>']
MIXED_WGRAD_LAUNCHES = 6
MIXED_WGRAD_KERNELS = ['conv_wgrad5_group_kernel<5>', 'conv_wgrad_reduce_kernel', 'conv_wgrad4_group_kernel<4, 1>',
                       'conv_wgrad_reduce_kernel', 'conv_wgrad2_group_kernel<5>', 'conv_wgrad_reduce_kernel']


def _launch_log(L, fn, device):
    """(launch-count delta, kernel names in launch order) of fn()"""
    import ctypes
    L.msmc_prof_enable(1)
    n0 = L.msmc_conv_launch_count()
    try:
        fn()
        count = L.msmc_conv_launch_count() - n0
        if torch.device(device).type == 'cuda':
            torch.cuda.synchronize()
        buf, ms, names = ctypes.create_string_buffer(128), ctypes.c_float(), []
        for i in range(L.msmc_prof_count()):
            assert L.msmc_prof_read(i, buf, 128, ctypes.byref(ms)) == 0
            names.append(buf.value.decode())
    finally:
        L.msmc_prof_enable(0)
    return count, names


def check_mixed_family_groups(device, report=None):
    """One msmc_conv_gather_group call and one msmc_conv_wgrad_group_ws4(group4 = 1) call whose members belong to several
    kernel families, interleaved: every member's result is the single launch of the same descriptor bit for bit, and the
    launches are the ones listed above, in that order.  ``report``: called with the four observed figures before they are
    compared (recording)."""
    import ctypes
    from msmctts_amd.hip import conv, lib
    L = lib.get()
    torch.manual_seed(0)

    def bf(*shape):
        return torch.randn(*shape, device=device).bfloat16()

    # ---- forward: seven gen-5 members of one configuration (more than one launch carries: six on one grid, the seventh
    # alone), two gen-7, gen-3 members of two configurations (two + one), two thin-channel and two wave-split members
    x5, w5, b5 = bf(2, 1, 150, 128), (bf(3, 264, 128) / 20), torch.randn(264, device=device)
    x3, w3 = bf(2, 1, 150, 64), (bf(3, 64, 64) / 14)
    x6, w6, b6 = bf(2, 11, 30, 16), (bf(9, 40, 16) / 12), torch.randn(40, device=device)
    x9 = bf(2, 1, 70, 512)
    w9 = {64: bf(3, 64, 512) / 39, 72: bf(3, 72, 512) / 39}

    def g5():
        return dict(x=x5, w=w5, geom=conv.Geometry(1, 150, (1, 3), (1, 1), (1, 2), (0, 2), False), bias=b5, in_slope=0.1)

    def g3():
        return dict(x=x3, w=w3, geom=conv.Geometry(1, 150, (1, 3), (1, 1), (1, 1), (0, 1), False), in_slope=0.1)

    def g6():
        return dict(x=x6, w=w6, geom=conv.Geometry(11, 30, (3, 3), (1, 1), (1, 1), (1, 1), False), bias=b6, out_slope=0.2)

    def g9(co):
        return dict(x=x9, w=w9[co], geom=conv.Geometry(1, 70, (1, 3), (1, 1), (1, 1), (0, 1), False), in_slope=0.1)

    members = [(40, g5()), (16, g3()), (56, g5()), (40, g5()), (9, g9(64)), (50, g6()), (40, g5()), (17, g3()), (40, g5()),
               (56, g5()), (16, g3()), (40, g5()), (9, g9(72)), (40, g5()), (50, g6()), (40, g5())]
    st = lib.stream(x5)
    descs, outs, refs = [], [], []
    for variant, item in members:
        d, out = conv._forward_desc(**item)
        d.variant = variant
        assert L.msmc_conv_gather(ctypes.byref(d), st) == 0, variant
        descs.append(d); outs.append(out); refs.append(out.clone())
        out.zero_()
    arr = (lib.ConvDesc * len(descs))(*descs)
    fwd = _launch_log(L, lambda: lib.check(L.msmc_conv_gather_group(arr, len(descs), st), 'msmc_conv_gather_group'), device)
    for (variant, _), out, ref in zip(members, outs, refs):
        assert ref.float().abs().max() > 0 and torch.equal(out, ref), variant

    # ---- weight gradient: two variant-7 members, two variant-4 and one variant-5 member (one fourth-generation grid), a
    # variant-3 member and a member outside the fourth generation's scope (Cout % 64: third generation)
    L.msmc_conv_set_wgrad_split(2)                              # (a shared grid plans another split: fix it for bit equality)
    try:
        xa = bf(2, 1, 90, 64)
        wmembers = []                                           # (H, W, kernel, stride, dilation, padding, reflect, Cout, variant)
        wmembers.append((1, 90, (1, 3), (1, 1), (1, 1), (0, 1), False, 64, 4))
        wmembers.append((40, 3, (5, 1), (3, 1), (1, 1), (2, 0), False, 64, 7))
        wmembers.append((9, 20, (3, 3), (1, 2), (1, 1), (1, 1), True, 64, 3))
        wmembers.append((1, 90, (1, 11), (1, 1), (1, 1), (0, 5), False, 64, 5))
        wmembers.append((13, 18, (3, 3), (2, 2), (1, 1), (1, 1), True, 128, 7))
        wmembers.append((1, 90, (1, 3), (1, 1), (1, 1), (0, 1), False, 40, 3))
        wmembers.append((1, 90, (1, 7), (1, 1), (1, 3), (0, 9), False, 128, 4))
        descs, keep, refs, outs = [], [], [], []
        for (H, W, k, s, dil, pad, reflect, cout, variant) in wmembers:
            geom = conv.Geometry(H, W, k, s, dil, pad, reflect)
            x = xa if (H, W) == (1, 90) else bf(2, H, W, 64)
            g = bf(2, geom.Hout, geom.Wout, cout)
            d = conv._build_desc(x.dtype, 2, H, W, 64, geom.Hout, geom.Wout, cout, geom.fwd_lattice, geom.fwd_taps,
                                 1 if reflect else 0, 0.1, 1.0, 1.0, 1.0)
            d.x = d.w = d.out = x.data_ptr()
            d.variant, d.dw_copies = variant, 1
            T = k[0] * k[1]
            need = L.msmc_conv_wgrad_workspace(ctypes.byref(d), g.data_ptr())
            ws = torch.zeros(max(1, need // 4), device=device)
            dw_ref, db_ref = torch.zeros(T, cout, 64, device=device), torch.zeros(cout, device=device)
            assert L.msmc_conv_wgrad_ws(ctypes.byref(d), g.data_ptr(), dw_ref.data_ptr(), db_ref.data_ptr(), ws.data_ptr(),
                                        need, st) == 0, variant
            descs.append(d); keep.append((x, g)); refs.append((dw_ref, db_ref))
            outs.append((torch.zeros(T, cout, 64, device=device), torch.zeros(cout, device=device)))
        n = len(descs)
        arr = (lib.ConvDesc * n)(*descs)
        vp = ctypes.c_void_p * n
        need = sum(L.msmc_conv_wgrad_workspace(ctypes.byref(d), xg[1].data_ptr()) for d, xg in zip(descs, keep))
        ws = torch.zeros(max(1, need // 4), device=device)
        wg = _launch_log(L, lambda: lib.check(L.msmc_conv_wgrad_group_ws4(
            arr, vp(*[xg[1].data_ptr() for xg in keep]), vp(*[o[0].data_ptr() for o in outs]),
            vp(*[o[1].data_ptr() for o in outs]), n, ws.data_ptr(), need, st, 1), 'msmc_conv_wgrad_group_ws4'), device)
        for m, (dw_ref, db_ref), (dw, db) in zip(wmembers, refs, outs):
            assert dw_ref.abs().max() > 0 and torch.equal(dw, dw_ref) and torch.equal(db, db_ref), m
    finally:
        L.msmc_conv_set_wgrad_split(0)
    if report:
        report(fwd[0], fwd[1], wg[0], wg[1])
    assert fwd[0] == MIXED_FORWARD_LAUNCHES, fwd
    assert fwd[1] == MIXED_FORWARD_KERNELS, fwd
    assert wg[0] == MIXED_WGRAD_LAUNCHES, wg
    assert wg[1] == MIXED_WGRAD_KERNELS, wg


# ---- process state shared by the forward (csrc/conv.hip) and the weight-gradient (csrc/conv_wgrad.hip) unit ------------
# What check_conv_shared_state observes, per dtype: launch-count deltas and msmc_conv_last_kernel() names.  Recorded by
# running this same check against the kernel interpreter built from the commit BEFORE conv.hip was split into three
# translation units (one unit, every switch a single static); the split must leave them as they are.
SHARED_STATE = {
    'bf16': {'forward': [1, 'conv_gather2_kernel<unsigned short, 1, 2, 4>'],
             'wgrad': [1, 'conv_wgrad2_kernel<3>'],
             'forward_group, grouping 1': 1, 'forward_group, grouping 0': 2,
             'wgrad_group, grouping 1': 1, 'wgrad_group, grouping 0': 2,
             # (64 bf16 channels are two channel chunks: too shallow for the pipelined forward, and the second-generation
             #  bf16 weight gradient does not read the switch)
             'forward gen 1': [1, 'conv_gather_kernel<unsigned short, 1>'],
             'forward gen 1, pipeline 0': [1, 'conv_gather_kernel<unsigned short, 1>'],
             'wgrad, pipeline 0': [1, 'conv_wgrad2_kernel<3>']},
    'fp32': {'forward': [1, 'conv_gather2_kernel<float, 1, 2, 4>'],
             'wgrad': [1, 'conv_wgrad_kernel<float, 4, 1>'],
             'forward_group, grouping 1': 1, 'forward_group, grouping 0': 2,
             'wgrad_group, grouping 1': 2, 'wgrad_group, grouping 0': 2,    # (no fp32 group kernel: one launch per member)
             'forward gen 1': [1, 'conv_gather_pipe_kernel<float, 1, 1>'],
             'forward gen 1, pipeline 0': [1, 'conv_gather_kernel<float, 1>'],
             'wgrad, pipeline 0': [1, 'conv_wgrad_kernel<float, 4, 0>']},
}
SHARED_FRESH_THREAD = (0, '')           # launch count and last-kernel name a thread sees before its first call


def check_conv_shared_state(device, report=None):
    """The launch counter, the last-kernel slot and the grouping / pipeline switches are ONE object each for the forward and
    the weight-gradient kernels: both directions move the same counter and name slot, msmc_conv_set_grouping(0) and
    msmc_conv_set_pipeline(0) reach both, and counter and slot stay per thread.  Layer: B = 1, 1 x 40 lattice, 64 -> 64
    channels, 1 x 3 kernel, alone and as a group of two.  ``report``: called with the observed figures before they are
    compared (recording)."""
    import ctypes
    import threading
    from msmctts_amd.hip import conv, lib
    L = lib.get()
    torch.manual_seed(0)
    count, last = L.msmc_conv_launch_count, lambda: L.msmc_conv_last_kernel().decode()
    geom = conv.Geometry(1, 40, (1, 3), (1, 1), (1, 1), (0, 1), False)
    vp = ctypes.c_void_p * 2

    def observe(dtype):
        x = torch.randn(1, 1, 40, 64, device=device).to(dtype)
        w = (torch.randn(3, 64, 64, device=device) / 14).to(dtype)
        g = torch.randn(1, 1, 40, 64, device=device).to(dtype)
        st = lib.stream(x)
        fd, out = conv._forward_desc(x=x, w=w, geom=geom, in_slope=0.1)
        wd = conv._build_desc(x.dtype, 1, 1, 40, 64, 1, 40, 64, geom.fwd_lattice, geom.fwd_taps, 0, 0.1, 1.0, 1.0, 1.0)
        wd.x = wd.w = wd.out = x.data_ptr()
        wd.dw_copies = 1
        need = L.msmc_conv_wgrad_workspace(ctypes.byref(wd), g.data_ptr())
        ws = torch.zeros(max(1, 2 * need // 4), device=device)
        dw, db = torch.zeros(2, 3, 64, 64, device=device), torch.zeros(2, 64, device=device)
        farr, warr = (lib.ConvDesc * 2)(fd, fd), (lib.ConvDesc * 2)(wd, wd)

        def forward():
            lib.check(L.msmc_conv_gather(ctypes.byref(fd), st), 'msmc_conv_gather')

        def wgrad():
            lib.check(L.msmc_conv_wgrad_ws(ctypes.byref(wd), g.data_ptr(), dw[0].data_ptr(), db[0].data_ptr(),
                                           ws.data_ptr(), need, st), 'msmc_conv_wgrad_ws')

        def forward_group():
            lib.check(L.msmc_conv_gather_group(farr, 2, st), 'msmc_conv_gather_group')

        def wgrad_group():
            lib.check(L.msmc_conv_wgrad_group_ws(warr, vp(g.data_ptr(), g.data_ptr()), vp(dw[0].data_ptr(), dw[1].data_ptr()),
                                                 vp(db[0].data_ptr(), db[1].data_ptr()), 2, ws.data_ptr(), 2 * need, st),
                      'msmc_conv_wgrad_group_ws')

        def run(fn):                    # [launch-count delta, last-kernel name] of one call
            n0 = count()
            fn()
            return [count() - n0, last()]

        seen = {'forward': run(forward), 'wgrad': run(wgrad)}
        for on in (1, 0):
            L.msmc_conv_set_grouping(on)
            try:
                seen['forward_group, grouping %d' % on] = run(forward_group)[0]
                seen['wgrad_group, grouping %d' % on] = run(wgrad_group)[0]
            finally:
                L.msmc_conv_set_grouping(1)
        fd.variant = 1                  # first-generation forward kernels: the ones the pipeline switch chooses between
        seen['forward gen 1'] = run(forward)
        L.msmc_conv_set_pipeline(0)
        try:
            seen['forward gen 1, pipeline 0'] = run(forward)
            seen['wgrad, pipeline 0'] = run(wgrad)
        finally:
            L.msmc_conv_set_pipeline(1)
        if torch.device(device).type == 'cuda':
            torch.cuda.synchronize()
        return seen

    seen = {'bf16': observe(torch.bfloat16), 'fp32': observe(torch.float32)}
    fresh = []
    t = threading.Thread(target=lambda: fresh.append((count(), last())))
    t.start()
    t.join()
    if report:
        report(seen, fresh[0])
    assert count() > 0 and last() != ''                     # (so the fresh thread's figures are its own)
    assert seen == SHARED_STATE, seen
    assert fresh[0] == SHARED_FRESH_THREAD, fresh
