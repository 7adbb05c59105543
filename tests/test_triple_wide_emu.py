"""CPU: the wide triple loss (csrc/triple_wide.inc) on the kernel interpreter, through the C entry, hip/losses.py and Quantize
(cases and references: tests/_triplewidecases.py; the same on the GPU: tests/test_gpu_triple_wide.py)."""
import os
import subprocess

import pytest

import _triplewidecases as cases

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


@pytest.mark.parametrize('s,n', cases.PARAMS, ids=cases.IDS)
def test_exact_on_an_integer_lattice(s, n):
    cases.check_lattice(DEV, s, n)


@pytest.mark.parametrize('s,n', cases.PARAMS, ids=cases.IDS)
def test_matches_float64_within_the_derived_budget(s, n):
    cases.check_real_values(DEV, s, n)


@pytest.mark.parametrize('s', cases.INVARIANT_SHAPES, ids=cases.INVARIANT_IDS)
def test_rows_do_not_depend_on_the_other_frames_or_the_tiling(s):
    cases.check_invariance(DEV, s)


@pytest.mark.parametrize('s,n', cases.SHARED_PARAMS, ids=cases.SHARED_IDS)
def test_agrees_with_the_resident_and_streamed_kernels(s, n):
    cases.check_agrees_with_the_other_kernels(DEV, s, n)


@pytest.mark.parametrize('m', range(len(cases.MODULES)), ids=cases.MODULE_IDS)
def test_quantize_takes_the_wide_kernel(m):
    cases.check_module(DEV, m)


def test_wrapper_routes_between_the_three_entries():
    cases.check_wrapper_routes(DEV)


def test_refused_arguments_and_the_empty_input():
    cases.check_refusals(DEV)


def test_the_symbols_are_exported_and_bound():
    cases.check_feature_present()
