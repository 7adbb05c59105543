"""Shared cases of the host layer between the modules of msmctts_amd/hip and the C ABI: ``lib.call``, ``lib.workspace``, the fp32
frames a search keeps for the EMA update behind it (``vq._F32_OF``) and the frame source of hip/kmeans.py (``_Frames``).  The CPU
file (tests/test_hip_lib_helpers.py) runs them on the kernel interpreter, the GPU file (tests/test_gpu_hip_lib_helpers.py) runs
the ones that take a device on the card."""
import re

import numpy as np
import pytest
import torch

from msmctts_amd.hip import kmeans, lib, vq


# ---- lib.call -----------------------------------------------------------------------------------------------------------------
def _prepare_args(dev, H=1, d=16, K=16):
    embed = torch.randn(H, d, K, generator=torch.Generator().manual_seed(3)).to(dev)
    embed_t = torch.zeros((H, K, d), dtype=torch.float32, device=dev)
    enorm = torch.zeros((H, K), dtype=torch.float32, device=dev)
    return embed, embed_t, enorm, (lib.ptr(embed), lib.ptr(embed_t), lib.ptr(enorm), H, d, K, lib.stream(embed))


def check_call_passes_a_zero_return(dev):
    embed, embed_t, enorm, args = _prepare_args(dev)
    assert lib.call('msmc_vq_prepare', *args) is None
    assert torch.equal(embed_t, embed.transpose(1, 2))                      # (it ran: the codebook, transposed)
    assert torch.allclose(enorm, embed.pow(2).sum(1), rtol=1e-5, atol=1e-5)


def check_call_raises_on_a_code(dev):
    _, _, _, args = _prepare_args(dev)
    L = lib.get()
    original = L.msmc_vq_prepare
    setattr(L, 'msmc_vq_prepare', lambda *a: -2)
    try:
        with pytest.raises(RuntimeError) as err:
            lib.call('msmc_vq_prepare', *args)
        assert str(err.value) == 'msmc_vq_prepare failed with code -2'
        with pytest.raises(RuntimeError) as err:
            lib.call('msmc_vq_prepare', *args, what='msmc_vq_prepare(a label)')
        assert str(err.value) == 'msmc_vq_prepare(a label) failed with code -2'
    finally:
        setattr(L, 'msmc_vq_prepare', original)


def check_call_unknown_name():
    with pytest.raises(AttributeError):
        lib.call('msmc_no_such_entry_point')


def check_call_runs_what_is_installed_on_the_handle(dev):
    """the contract of the benchmark's timers: ``setattr(lib.get(), name, wrapper)`` after import is what runs"""
    _, embed_t, _, args = _prepare_args(dev)
    L = lib.get()
    original = L.msmc_vq_prepare
    seen = []

    def wrapper(*a):
        seen.append(len(a))
        return original(*a)

    lib.call('msmc_vq_prepare', *args)
    assert seen == []
    setattr(L, 'msmc_vq_prepare', wrapper)
    try:
        embed_t.zero_()
        lib.call('msmc_vq_prepare', *args)
        assert seen == [7] and embed_t.abs().sum() > 0                       # (the wrapper ran, and through it the kernel)
    finally:
        setattr(L, 'msmc_vq_prepare', original)
    lib.call('msmc_vq_prepare', *args)
    assert seen == [7] and lib.get().msmc_vq_prepare is original


# ---- lib.workspace ------------------------------------------------------------------------------------------------------------
def check_workspace(dev):
    dev = torch.device(dev)
    have = torch.empty(5, dtype=torch.float32, device=dev)
    for nbytes in (0, 1, 17, 20):                                           # (20: exactly its size)
        assert lib.workspace(nbytes, dev, have) is have
    assert lib.workspace(20, dev, have, floor=64) is have                   # (the floor sizes a new tensor only)
    for other in (torch.empty(24, dtype=torch.uint8, device=dev), torch.empty(3, dtype=torch.float64, device=dev)):
        assert lib.workspace(24, dev, other) is other                       # (bytes count, not elements)
        assert lib.workspace(25, dev, other) is not other
    for nbytes, floor, numel in ((21, 0, 6), (24, 0, 6), (10, 0, 3), (10, 4, 4), (0, 1, 1), (17, 4, 5), (0, 0, 0)):
        for old in (None, have if nbytes > 20 else None):
            ws = lib.workspace(nbytes, dev, old, floor=floor)
            assert ws is not have and ws.dtype == torch.float32 and ws.device.type == dev.type and tuple(ws.shape) == (numel,)
            assert ws.numel() == max(floor, -(-nbytes // 4))


# ---- the fp32 frames a search keeps for the EMA update ------------------------------------------------------------------------
def check_search_keeps_only_a_cast(dev, H=2, d=16, K=16, B=2, T=16):
    gen = torch.Generator().manual_seed(11)
    embed = torch.randn(H, d, K, generator=gen).to(dev)
    x = torch.randn(B, T, H * d, generator=gen).to(dev)
    length = torch.tensor([T, T - 5], dtype=torch.int64, device=dev)
    et, en = vq.vq_prepare(embed, frames=B * T)

    vq.vq_search(x, et, en)
    assert vq._F32_OF['last'] is None                                       # (fp32 frames are their own copy: nothing kept)

    xb = x.bfloat16()
    _, _, ind = vq.vq_search(xb, et, en)
    kept = vq._F32_OF['last']
    assert kept is not None and kept[0] == xb.data_ptr() and kept[1] == torch.bfloat16
    assert kept[3].dtype == torch.float32 and torch.equal(kept[3], xb.float())

    def buffers():
        return embed.clone(), torch.ones(H, K, device=dev), embed.clone()

    from_pin, direct = buffers(), buffers()
    vq.vq_ema_update(xb, ind, length, *from_pin, 0.99, 1e-5)
    assert vq._F32_OF['last'] is None                                       # (one reader per search)
    vq.vq_ema_update(xb.float(), ind, length, *direct, 0.99, 1e-5)
    for a, b, name in zip(from_pin, direct, ('embed', 'cluster_size', 'embed_avg')):
        assert torch.equal(a, b), name
    assert not torch.equal(from_pin[0], embed)                              # (the update did something)

    vq.vq_search(xb, et, en)
    vq.vq_search(x, et, en)
    assert vq._F32_OF['last'] is None                                       # (an fp32 search leaves no earlier cast behind either)


# ---- kmeans._Frames -------------------------------------------------------------------------------------------------------------
def check_frame_source_kinds(N=37, d=16):
    wide = torch.randn(N, 2 * d, generator=torch.Generator().manual_seed(5))
    base = wide[:, ::2].contiguous()
    index = torch.tensor([3, 0, 36])
    kinds = {'tensor': base, 'numpy': base.numpy(), 'tensor view': wide[:, ::2], 'numpy view': wide.numpy()[:, ::2]}
    assert not kinds['tensor view'].is_contiguous() and not kinds['numpy view'].flags['C_CONTIGUOUS']
    for name, frames in kinds.items():
        f = kmeans._Frames(frames, 'cpu')
        assert (f.N, f.d, f.device, f.on_device) == (N, d, torch.device('cpu'), False), name
        for got, want in ((f.rows(5, 20), base[5:20]), (f.take(index), base[index]), (f.rows(0, N), base)):
            assert got.dtype == torch.float32 and got.is_contiguous() and got.device == f.device, name
            assert torch.equal(got, want), name
    assert torch.equal(kmeans._Frames(base.double().numpy(), 'cpu').rows(5, 20), base[5:20])    # (other dtypes arrive as fp32)


def check_frame_source_refuses_other_ranks():
    for bad in (torch.zeros(5), torch.zeros(2, 3, 4), np.zeros(5, dtype=np.float32), np.zeros((2, 3, 4), dtype=np.float32)):
        text = re.escape('frames: expected [N, d], got %s' % (tuple(bad.shape),))
        with pytest.raises(ValueError, match=text):
            kmeans._Frames(bad, 'cpu')
        with pytest.raises(ValueError, match=text):
            kmeans.fit_kmeans(bad, 2, device='cpu')
        with pytest.raises(ValueError, match=text):
            kmeans.kmeans_plusplus(bad, 2, device='cpu')
