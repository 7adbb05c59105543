"""GPU: the acoustic features on the MI355X -- csrc/features.hip, msmctts_amd/hip/features.py and tools/extract_features.py:
the cases of tests/_featurecases.py (on the interpreter: tests/test_features_emu.py)."""
import pytest

import _featurecases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


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


def test_the_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
