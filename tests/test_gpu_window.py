"""GPU: the window-gather kernel pair (csrc/window.hip) on the MI355X -- the cases of tests/_windowcases.py (the same on the
interpreter: tests/test_window_emu.py)."""
import pytest

import _windowcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


PARAMS = [(n, p) for n in range(len(cases.CASES)) for p in range(len(cases.DTYPES))]      # (the scalar cases too)
PARAM_IDS = ['%s %s' % (cases.IDS[n], cases.DTYPE_IDS[p]) for n, p in PARAMS]


@pytest.mark.parametrize('n,pair', PARAMS, ids=PARAM_IDS)
def test_windows_and_gradient_equal_the_stack_cast_chain_bit_for_bit(n, pair):
    cases.check_forward_backward(DEV, n, pair)


@pytest.mark.parametrize('n,pair', PARAMS, ids=PARAM_IDS)
def test_backward_writes_every_element_of_a_nan_filled_gradient(n, pair):
    cases.check_backward_writes_every_element(DEV, n, pair)


def test_any_table_contents_stay_inside_the_buffers():
    cases.check_hostile_tables(DEV)


def test_rejected_arguments_return_the_shape_error_and_raise():
    cases.check_rejected_arguments(DEV)


def test_the_symbols_are_exported():
    cases.check_feature_present()
