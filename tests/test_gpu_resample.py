"""GPU: the waveform preparation on the MI355X -- csrc/resample.hip, msmctts_amd/hip/resample.py, tools/prepare_wavs.py and the
``--resample`` path of tools/extract_features.py: the cases of tests/_resamplecases.py (on the interpreter:
tests/test_resample_emu.py)."""
import pytest

import _resamplecases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('name', list(cases.RATIOS))
def test_ratios(name):
    cases.check_ratio(DEV, name)


def test_bank_beyond_lds():
    cases.check_bank_beyond_lds(DEV)


def test_default_preset():
    cases.check_default_preset(DEV)


@pytest.mark.parametrize('name', list(cases.length_cases()))
def test_lengths(name):
    cases.check_length(DEV, name)


def test_empty_utterance_in_a_batch():
    cases.check_empty_in_batch(DEV)


@pytest.mark.parametrize('channels', [1, 2, 3])
def test_channels(channels):
    cases.check_channels(DEV, channels)


def test_int16_equals_fp32():
    cases.check_int16(DEV)


def test_same_rate_is_a_pure_downmix():
    cases.check_same_rate_is_downmix(DEV)


def test_ragged_batch_with_poisoned_padding_equals_solo_runs():
    cases.check_ragged(DEV)


def test_two_runs_give_the_same_bits():
    cases.check_repeat(DEV)


def test_wider_row_gives_the_same_bits():
    cases.check_wider_row(DEV)


def test_normalisation():
    cases.check_normalisation(DEV)


def test_prepared_waveforms_feed_the_extractors():
    cases.check_chain(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


def test_prepare_wavs_tool(tmp_path):
    cases.check_prepare_tool(DEV, tmp_path)


def test_extract_features_resample(tmp_path):
    cases.check_extract_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
