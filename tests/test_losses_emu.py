"""CPU: the loss-term kernels of csrc/losses.hip (multi-tensor L1 / MSE sums, masked means, weighted sums of scalars) on the kernel
interpreter, through the C entries and through hip/losses.py mse_const_halves / weighted_sum, against float64 references (cases,
references and bars: tests/_losscases.py; the same on the GPU: tests/test_gpu_losses.py)."""
import os
import subprocess

import pytest

import _losscases as cases

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


BOTH = (0, 1)
NAMES = ['fp32', 'bf16']
MODES = ['l1', 'mse']


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('mode', BOTH, ids=MODES)
@pytest.mark.parametrize('name', cases.TABLE_KEYS)
def test_forward_exact_sums(name, mode, which):
    cases.check_forward(DEV, which, mode, name, True)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('mode', BOTH, ids=MODES)
@pytest.mark.parametrize('name', ('ve+1', '256ve+1', 'big', 'mixed'))
def test_forward_random_values(name, mode, which):
    cases.check_forward(DEV, which, mode, name, False)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('mode', BOTH, ids=MODES)
@pytest.mark.parametrize('name', cases.TABLE_KEYS)
def test_atomic_forward(name, mode, which):
    cases.check_forward(DEV, which, mode, name, True, atomic=True)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('mode', BOTH, ids=MODES)
@pytest.mark.parametrize('off', ((1, 0), (0, 1)), ids=['a', 'b'])
def test_forward_operand_one_element_into_its_buffer(off, mode, which):
    if mode == 1 and off == (0, 1):
        off = (1, 0)                                # the MSE sum has no b: a alone, on the other table
        cases.check_forward(DEV, which, mode, 've+1', True, off=off)
        return
    for name in ('256ve+1', 've+1'):
        cases.check_forward(DEV, which, mode, name, True, off=off)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('mode', BOTH, ids=MODES)
@pytest.mark.parametrize('name', cases.TABLE_KEYS)
def test_backward(name, mode, which):
    cases.check_backward(DEV, which, mode, name)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('mode', BOTH, ids=MODES)
@pytest.mark.parametrize('off', ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ids=['a', 'b', 'ga'])
def test_backward_operand_one_element_into_its_buffer(off, mode, which):
    for name in ('256ve+1', 've+1'):
        cases.check_backward(DEV, which, mode, name, off=off)


def test_backward_largest_size_the_interpreter_runs():
    cases.check_backward(DEV, 0, 0, 'cap', ns=(cases.CAP_EMU,))
    cases.check_backward(DEV, 0, 1, 'cap', ns=(cases.CAP_EMU,))


def test_multi_tensor_refusals():
    cases.check_multi_refusals(DEV)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('use', ('both', 'first', 'second'))
def test_mse_const_halves(use, B, which):
    cases.check_halves(DEV, which, B, use)


@pytest.mark.parametrize('exact', (True, False), ids=['exact', 'random'])
@pytest.mark.parametrize('len64', (0, 1), ids=['i32', 'i64'])
@pytest.mark.parametrize('shape', sorted(cases.MM_SHAPES), ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('wa,wb', cases.MM_PAIRS)
def test_masked_mean_of_squared_differences(wa, wb, shape, len64, exact):
    cases.check_masked_mean(DEV, shape, wa, wb, 1, len64, exact)


@pytest.mark.parametrize('exact', (True, False), ids=['exact', 'random'])
@pytest.mark.parametrize('len64', (0, 1), ids=['i32', 'i64'])
@pytest.mark.parametrize('shape', sorted(cases.MM_SHAPES), ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('which', BOTH, ids=NAMES)
def test_masked_mean_of_one_tensor(which, shape, len64, exact):
    cases.check_masked_mean(DEV, shape, which, which, 0, len64, exact)


def test_masked_mean_refusals():
    cases.check_masked_mean_refusals(DEV)


@pytest.mark.parametrize('n', (1, 2, 64))
def test_scalar_weighted_sum(n):
    cases.check_wsum(DEV, n)


def test_scalar_weighted_sum_refusals():
    cases.check_wsum_refusals(DEV)


def test_weighted_sum_function():
    cases.check_weighted_sum_function(DEV)
