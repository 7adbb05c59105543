"""GPU: the F0 tracker on the MI355X -- csrc/pitch.hip, msmctts_amd/hip/pitch.py and the ``--pitch`` path of
tools/extract_features.py: the cases of tests/_pitchcases.py (on the interpreter: tests/test_pitch_emu.py)."""
import pytest

import _pitchcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


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


def test_the_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
