"""CPU: the speaker reference encoder's kernels (csrc/tdnn.hip msmc_relu_bn_* / msmc_se_* / msmc_asp_*) on the kernel interpreter,
through the Python ops of hip/tdnn.py, against the fp64 formulas (cases, reference and bounds: tests/_tdnncases.py; the same on
the GPU: tests/test_gpu_tdnn.py).  Every case runs its op twice and asserts bit-identical results."""
import os
import subprocess

import pytest
import torch

import _tdnncases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')
DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emulator():
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    lib.use_library_for_tests(EMU)
    assert lib.backend() == 'emu'
    yield
    lib._lib, lib._host_pointers_ok = saved


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
