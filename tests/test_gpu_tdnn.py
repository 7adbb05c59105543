"""GPU: the speaker reference encoder on the MI355X -- the kernel cases of tests/_tdnncases.py (the same on the interpreter:
tests/test_tdnn_emu.py), the module and model cases of tests/_ecapacases.py against the reference's own outputs (interpreter:
tests/test_ecapa.py), and one bf16 forward + backward of the encoder captured into a hipGraph."""
import numpy as np
import pytest
import torch

import _ecapacases
import _tdnncases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('N,C', _tdnncases.RBN_SHAPES)
def test_relu_batch_norm_forward_backward_and_buffers(N, C, dtype, training):
    _tdnncases.check_relu_bn(DEV, N, C, dtype, training)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_relu_batch_norm_on_a_channel_slice(dtype, training):
    """C = 32 channels of a 256-wide row, as a Res2 branch sees them"""
    N, C, wide, offset = _tdnncases.RBN_SLICE
    _tdnncases.check_relu_bn(DEV, N, C, dtype, training, wide=wide, offset=offset)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,T,C', _tdnncases.SE_SHAPES)
def test_se_residual_forward_and_all_gradients(B, T, C, dtype):
    _tdnncases.check_se(DEV, B, T, C, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,T,C', list(_tdnncases.ASP_CASES))
def test_attentive_stats_pool_forward_and_gradients(B, T, C, dtype):
    _tdnncases.check_asp(DEV, B, T, C, dtype)


def test_refusals_return_the_shape_error():
    _tdnncases.check_relu_bn_refusals(DEV)
    _tdnncases.check_se_refusals(DEV)
    _tdnncases.check_asp_refusals(DEV)


def test_ecapa_encoder_matches_the_reference_on_the_kernels():
    _ecapacases.check_encoder(DEV)


def test_ecapa_kernel_and_stock_paths_agree_on_the_same_weights():
    _ecapacases.check_paths_agree(DEV)


def test_ecapa_construction_refusals():
    from msmctts_amd.networks.vqgantts.tdnn import ECAPA_TDNN
    with pytest.raises(NotImplementedError, match='channels'):
        ECAPA_TDNN(in_channels=24, embd_dim=32, channels=32)


def test_ecapa_autoencoder_with_the_global_encoder_matches_the_reference():
    _ecapacases.check_autoencoder(DEV)


def test_ecapa_bf16_forward_backward_replays_from_a_graph():
    """eager bf16 forward + backward, then the same captured into a hipGraph and replayed twice: replay == eager within one bf16
    rounding (2^-8 |q|, plus 1e-6), the two replays bit-identical"""
    m, z = _ecapacases.build_encoder(DEV)
    m.hip_dtype = torch.bfloat16
    m.train()
    x = torch.from_numpy(z['enc.x']).to(DEV).requires_grad_(True)
    cot = torch.from_numpy(z['enc.cotangent']).to(DEV)
    names = [k for k, _ in m.named_parameters()]

    def step():
        for p in m.parameters():
            p.grad = None
        x.grad = None
        y = m(x)
        (y * cot).sum().backward()
        return y

    def snapshot(y):
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            y = step()
        eager = snapshot(y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(snapshot(y))
    for name, a, b in zip(['y', 'grad x'] + names, replays[0], replays[1]):
        assert torch.equal(a, b), name
    for name, e, r in zip(['y', 'grad x'] + names, eager, replays[0]):
        err = (e.double() - r.double()).abs()
        tol = 2.0 ** -8 * e.double().abs() + 1e-6
        print('graph %-40s max err %.3e' % (name, float(err.max())))
        assert bool((err <= tol).all()), name
    # two eager steps and two replays ran (the capture itself executes nothing): the counter lives on the device and is replayed
    assert int(m.bn2.num_batches_tracked) == int(z['enc.state.bn2.num_batches_tracked']) + 4
