"""CPU: the BatchNorm kernels of the normalised quantiser (csrc/norm.hip msmc_bn_*) on the kernel interpreter, through the Python
op of hip/norm.py, against the fp64 formulas (cases, reference and bounds: tests/_bncases.py; the same on the GPU:
tests/test_gpu_bn.py)."""
import os
import subprocess

import pytest
import torch

import _bncases

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
@pytest.mark.parametrize('out_fp32', [False, True], ids=['same', 'f32out'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('N,C', _bncases.SHAPES)
def test_batch_norm_forward_backward_and_buffers(N, C, dtype, out_fp32, training):
    _bncases.check_case(DEV, N, C, dtype, out_fp32, training)


def test_batch_norm_survives_cancellation():
    """x = 100 + 0.1 randn: a variance formed as E[x^2] - E[x]^2 in fp32 misses this bound by orders of magnitude"""
    _bncases.check_case(DEV, 150, 256, torch.float32, False, True, cancel=True)


def test_batch_norm_is_bit_reproducible():
    _bncases.check_determinism(DEV)


def test_batch_norm_refusals():
    _bncases.check_refusals(DEV)
