"""CPU: the acoustic features on the kernel interpreter -- csrc/features.hip, msmctts_amd/hip/features.py and
tools/extract_features.py (cases, references and the derivation of the bounds: tests/_featurecases.py; the same on the GPU:
tests/test_gpu_features.py).  The real geometry (2048 / 800 / 200, M = 80, the fixture's three waveforms: 43 frames) runs here
too: it takes about as long as the other cases together, under ten seconds."""
import os
import subprocess

import pytest

import _featurecases as cases

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


def test_restatement_equals_the_reference_fixture():
    cases.check_restatement()


def test_kernel_at_the_real_geometry():
    cases.check_real_geometry(DEV)


@pytest.mark.parametrize('name', list(cases.LENGTHS))
def test_small_geometry_lengths(name):
    cases.check_length(DEV, name)


def test_ragged_batch_equals_solo_runs():
    cases.check_ragged(DEV)


def test_two_runs_give_the_same_bits():
    cases.check_repeat(DEV)


def test_silence():
    cases.check_silence(DEV)


@pytest.mark.parametrize('name', list(cases.VARIANTS))
def test_variants(name):
    cases.check_variant(DEV, name)


def test_int16_input():
    cases.check_int16(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


def test_host_tensors_need_the_interpreter():
    cases.check_host_tensors_need_the_interpreter()


def test_the_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_tool_reads_a_config(tmp_path):
    cases.check_tool_config(tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
