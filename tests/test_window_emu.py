"""CPU: the window-gather kernel pair (csrc/window.hip) on the kernel interpreter, through the C entries and hip/window.py,
bit for bit against the stack / cast chain and its autograd (cases and reference: tests/_windowcases.py; the same on the GPU:
tests/test_gpu_window.py)."""
import os
import subprocess

import pytest

import _windowcases as cases

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
