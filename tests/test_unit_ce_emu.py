"""CPU: the unit predictor's loss and label decoding on the kernel interpreter -- csrc/unit_ce.hip, hip/unit_ce.py, the 'softmax'
method of the multi-stage quantiser, ``KMeansVQGANEmb.compute_embedding_loss`` / ``decode_units`` and ``UnitPredictorTrainer``
(cases, references and the derivation of the bounds: tests/_unitcecases.py; the same, with the large shapes, on the GPU:
tests/test_gpu_unit_ce.py)."""
import os
import subprocess

import pytest

import _unitcecases as cases

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


@pytest.mark.parametrize('name', cases.SMALL)
def test_kernels_match_the_restatement(name):
    cases.check_case(DEV, name)


def test_workgroups_stride_over_the_rows():
    cases.check_strided_grid(DEV)


def test_extreme_and_constant_rows():
    cases.check_extreme_rows(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_masked_cross_entropy_through_autograd(bf16):
    cases.check_autograd(DEV, bf16)


def test_softmax_method_of_the_multi_stage_quantiser():
    cases.check_softmax_method(DEV)


def test_kmeans_embedding_losses(tmp_path):
    cases.check_kmeans_losses(DEV, tmp_path)


def test_decode_units_round_trip(tmp_path):
    cases.check_decode_units(DEV, tmp_path)


def test_text_unit_batch():
    cases.check_text_unit_batch()


def test_trainer_steps_on_units_and_on_their_frames(tmp_path):
    cases.check_trainer_step(DEV, tmp_path)


def test_trainer_refusals(tmp_path):
    cases.check_trainer_refusals(DEV, tmp_path)


def test_head_width():
    cases.check_head_width(DEV)


def test_the_feature_is_present():
    cases.check_feature_present()
