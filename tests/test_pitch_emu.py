"""CPU: the F0 tracker on the kernel interpreter -- csrc/pitch.hip, msmctts_amd/hip/pitch.py and the ``--pitch`` path of
tools/extract_features.py (cases, the float64 restatement and the derivation of the bounds: tests/_pitchcases.py; the same on the
GPU: tests/test_gpu_pitch.py).  The real geometry (800 / 200, lags 32 .. 266, one second: 81 frames) runs here too, in a few
seconds."""
import os
import subprocess

import pytest

import _pitchcases as cases

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


def test_restatement_tracks_the_f0_of_its_inputs():
    cases.check_restatement_tracks_f0()


def test_at_most_two_percent_of_frames_are_left_out():
    cases.check_left_out_cap()


def test_kernel_at_the_real_geometry():
    cases.check_real_geometry(DEV)


@pytest.mark.parametrize('name', list(cases.LENGTHS))
def test_small_geometry_lengths(name):
    cases.check_length(DEV, name)


def test_noise_in_the_middle_is_unvoiced():
    cases.check_gap(DEV)


def test_periodic_frame_is_exactly_zero_at_its_period():
    cases.check_periodic_is_exact(DEV)


def test_ragged_batch_equals_solo_runs():
    cases.check_ragged(DEV)


def test_two_runs_give_the_same_bits():
    cases.check_repeat(DEV)


def test_silence_is_unvoiced():
    cases.check_silence(DEV)


def test_int16_input():
    cases.check_int16(DEV)


def test_hz_track():
    cases.check_hz(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


def test_host_tensors_need_the_interpreter():
    cases.check_host_tensors_need_the_interpreter()


def test_the_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_extractor_reads_a_config():
    cases.check_config()


def test_the_feature_is_present():
    cases.check_feature_present()
