"""GPU: ``EmbVQGANTrainer`` on the MI355X against the restated reference step -- the cases of tests/_embcases.py (the same on
the interpreter: tests/test_emb_trainer_emu.py)."""
import pytest

import _embcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('global_encoder', [False, True], ids=['plain', 'ecapa'])
@pytest.mark.parametrize('phase', [0, 1, 2], ids=['frames', 'spectral', 'gan'])
def test_step_matches_the_restated_reference_step(phase, global_encoder):
    cases.check_phase(DEV, phase, global_encoder)


def test_trainer_task_dataset_and_synthetic_batch_resolve_and_refusals_raise():
    cases.check_construction(DEV)


def test_model_window_forms_equal_the_slice_stack_chain():
    cases.check_model_window_forms(DEV)
