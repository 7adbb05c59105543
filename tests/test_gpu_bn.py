"""GPU: the BatchNorm kernels of the normalised quantiser (csrc/norm.hip msmc_bn_*) on the MI355X, through the Python
op of hip/norm.py, against the fp64 formulas (cases, reference and bounds: tests/_bncases.py; the same on the interpreter:
tests/test_bn_emu.py)."""
import pytest
import torch

import _bncases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


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
