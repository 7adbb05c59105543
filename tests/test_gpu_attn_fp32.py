"""GPU: the fp32 attention core (csrc/attn.hip attn_*_f32_kernel) on the MI355X -- the cases of tests/_attn32cases.py (the same on
the interpreter: tests/test_attn_fp32_emu.py)."""
import pytest

import _attn32cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('n', range(len(cases.VALUE_CASES)), ids=[c[0] for c in cases.VALUE_CASES])
def test_values_and_gradients_within_4x_of_the_fp32_chain(n):
    cases.check_values(DEV, n)


@pytest.mark.parametrize('n', range(len(cases.DROPOUT_CASES)), ids=[c[0] for c in cases.DROPOUT_CASES])
def test_dropout_mask_is_the_bf16_kernels_mask_and_the_backward_regenerates_it(n):
    cases.check_dropout(DEV, n)


def test_padding_batching_and_repetition_change_no_bit():
    cases.check_exact_properties(DEV)


def test_rejected_arguments_return_the_shape_error_and_raise():
    cases.check_rejected_arguments(DEV)


def test_output_gradient_is_cast_to_fp32():
    cases.check_gradient_casts(DEV)


@pytest.mark.parametrize('kernels', [True, False], ids=['kernels', 'stock'])
@pytest.mark.parametrize('prologue', [False, True], ids=['pos', 'prologue'])
@pytest.mark.parametrize('T', [45, 161])
def test_fp32_block_stack_matches_the_oracle(T, prologue, kernels):
    cases.check_block_stack(DEV, T, prologue, kernels)


def test_fp32_is_a_supported_dtype_and_the_symbols_are_exported():
    cases.check_feature_present()
