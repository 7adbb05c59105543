"""GPU: the unit-input path on the MI355X -- runs back to labels (csrc/units.hip), the decoder input from labels and its gradient
(csrc/unit_embed.hip), hip/units.py, ``KMeansVQGANEmb.forward_units`` / ``synthesis_units``, the unit batch of
``EmbVQGANTrainer`` in its three phases and tools/synthesize_units.py: the cases of tests/_unitembedcases.py (the smaller ones also
on the interpreter: tests/test_unit_embed_emu.py)."""
import pytest

import _unitembedcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('R', cases.EXPAND_R)
def test_expand_matches_the_restatement(R):
    cases.check_expand(DEV, R)


def test_expand_undoes_collapse():
    cases.check_expand_round_trip(DEV)


def test_expand_refuses_empty_shapes():
    cases.check_expand_refusals(DEV)


@pytest.mark.parametrize('s', range(len(cases.FWD_SHAPES)), ids=cases.FWD_IDS)
def test_embed_forward_is_the_gather_bit_for_bit(s):
    cases.check_embed_forward(DEV, s)


def test_embed_forward_with_more_blocks_than_the_grid():
    cases.check_embed_forward_strided_grid(DEV, 3, 2800, 2048, 100)           # 2100 blocks, 2048 workgroups: 69 MB written


def test_embed_forward_refusals_launch_nothing():
    cases.check_embed_forward_refusals(DEV)


def test_embed_backward_is_the_documented_sum():
    cases.check_embed_backward(DEV)


def test_embed_backward_wide_rows_and_more_labels_than_frames():
    cases.check_embed_backward_wide(DEV)


def test_embed_backward_refusals_and_short_workspace():
    cases.check_embed_backward_refusals(DEV)


def test_unit_embed_through_autograd():
    cases.check_autograd(DEV)


@pytest.mark.parametrize('global_encoder', [False, True], ids=['plain', 'global encoder'])
def test_forward_units_agrees_with_forward_on_centroid_frames(tmp_path, global_encoder):
    cases.check_model(DEV, tmp_path, global_encoder)


def test_synthesis_units_on_runs_is_synthesis_units_on_labels(tmp_path):
    cases.check_synthesis_units(DEV, tmp_path)


@pytest.mark.parametrize('phase', [0, 1, 2])
def test_trainer_steps_on_a_unit_batch(tmp_path, phase):
    cases.check_trainer_phase(DEV, tmp_path, phase)


def test_trainer_refuses_a_model_without_forward_units():
    cases.check_trainer_needs_forward_units(DEV)


def test_synthesize_units_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
