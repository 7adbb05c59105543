"""CPU: the spectrogram and the Griffin-Lim inverses on the kernel interpreter -- csrc/griffin_lim.hip,
msmctts_amd/hip/griffin_lim.py, tools/invert_features.py and tools/extract_features.py --spectrogram (cases, references and the
derivation of the bounds: tests/_griffinlimcases.py; the same on the GPU: tests/test_gpu_griffin_lim.py)."""
import os
import subprocess

import pytest

import _griffinlimcases as cases

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


def test_the_feature_is_present():
    cases.check_feature_present()


def test_restatement_equals_the_reference_fixture():
    cases.check_restatement()


def test_stft_complex_mode():
    cases.check_stft_complex(DEV)


def test_spectrogram_equals_the_reference_fixture():
    cases.check_db(DEV)


@pytest.mark.parametrize('frames', cases.ISTFT_FRAMES)
def test_istft_lengths(frames):
    cases.check_istft_length(DEV, frames)


@pytest.mark.parametrize('name', list(cases.GEOMETRIES))
def test_istft_geometries(name):
    cases.check_istft_geometry(DEV, name)


def test_istft_ragged_batch_equals_solo_runs():
    cases.check_istft_ragged(DEV)


def test_round_trip():
    cases.check_round_trip(DEV)


def test_projection_and_momentum():
    cases.check_project(DEV)


def test_first_inverse_of_a_run():
    cases.check_first_inverse(DEV)


def test_runs_converge_as_the_reference():
    cases.check_runs_converge(DEV)


def test_sixty_iterations():
    cases.check_sixty_iterations(DEV)


def test_real_geometry():
    cases.check_real_geometry(DEV)


def test_ragged_run_equals_solo_runs():
    cases.check_ragged_run(DEV)


def test_deemphasis():
    cases.check_deemphasis(DEV)


def test_two_runs_give_the_same_bits():
    cases.check_repeat(DEV)


def test_silence():
    cases.check_silence(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


def test_host_tensors_need_the_interpreter():
    cases.check_host_tensors_need_the_interpreter()


def test_the_tools(tmp_path):
    cases.check_tools(DEV, tmp_path)


def test_from_config(tmp_path):
    cases.check_config(tmp_path)
