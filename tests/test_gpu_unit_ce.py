"""GPU: the unit predictor's loss and label decoding on the MI355X -- csrc/unit_ce.hip, hip/unit_ce.py, the 'softmax' method of
the multi-stage quantiser, ``KMeansVQGANEmb.compute_embedding_loss`` / ``decode_units`` and ``UnitPredictorTrainer``: every case
of tests/_unitcecases.py (the smaller ones also on the interpreter: tests/test_unit_ce_emu.py)."""
import pytest

import _unitcecases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('name', list(cases.CASES))
def test_kernels_match_the_restatement(name):
    cases.check_case(DEV, name)


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


def test_trainer_steps_on_units_and_on_their_frames(tmp_path):
    cases.check_trainer_step(DEV, tmp_path)


def test_trainer_refusals(tmp_path):
    cases.check_trainer_refusals(DEV, tmp_path)


def test_head_width():
    cases.check_head_width(DEV)


def test_the_feature_is_present():
    cases.check_feature_present()
