"""CPU: the waveform preparation on the kernel interpreter -- csrc/resample.hip, msmctts_amd/hip/resample.py,
``read_wav_channels``, tools/prepare_wavs.py and the ``--resample`` path of tools/extract_features.py (cases, the float64
restatement and the derivation of the bound: tests/_resamplecases.py; the same on the GPU: tests/test_gpu_resample.py)."""
import os
import subprocess

import pytest

import _resamplecases as cases

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


def test_restatement_is_resample_poly():
    cases.check_restatement_is_resample_poly()


def test_restatement_passes_1_khz_and_stops_15_khz():
    cases.check_sines()


def test_out_length_and_bank_layout():
    cases.check_out_length()


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


def test_host_tensors_need_the_interpreter():
    cases.check_host_tensors_need_the_interpreter()


def test_read_wav_channels(tmp_path):
    cases.check_read_wav_channels(tmp_path)


def test_prepare_wavs_tool(tmp_path):
    cases.check_prepare_tool(DEV, tmp_path)


def test_extract_features_resample(tmp_path):
    cases.check_extract_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
