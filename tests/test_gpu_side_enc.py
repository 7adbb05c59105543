"""GPU: the pitch / energy side encoder, ``EmbVC`` and their trainer steps on the MI355X -- csrc/side_enc.hip,
hip/side_enc.py, ``MAMSEncoder.fused_side``, networks/vqgantts/msmc_vqgan_emb.py ``EmbVC`` (cases, references and the derivation
of the bounds: tests/_sideenccases.py; the same on the interpreter: tests/test_side_enc_emu.py)."""
import pytest

import _sideenccases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('name', cases.FRONT_CASES)
def test_front_kernels_match_the_restatement(name):
    T, C = (int(v[1:]) for v in name.split('-'))
    cases.check_front(DEV, T, C)


def test_front_backward_refuses_a_short_workspace():
    cases.check_front_workspace_refused(DEV)


@pytest.mark.parametrize('scale', cases.POOL_SCALES)
def test_pool_add_kernels_match_the_restatement(scale):
    cases.check_pool(DEV, scale)


def test_two_chained_pooled_stages():
    cases.check_pool_chain(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_fused_encoder_against_the_stock_chain(bf16):
    cases.check_autograd(DEV, bf16)


def test_the_fused_path_runs():
    cases.check_fused_path_ran(DEV)


def test_embvc_against_the_reference():
    cases.check_vc_golden(DEV)


def test_embvc_unsupported_methods_raise():
    cases.check_vc_unsupported(DEV)


def test_infer_step_gives_a_waveform():
    cases.check_vc_infer(DEV)


@pytest.mark.parametrize('model', ['EmbVC', 'MSMCVQGANEmb'])
def test_trainer_steps_with_tracks(model):
    cases.check_trainer(DEV, model)


def test_batch_tracks():
    cases.check_batch_tracks()


def test_the_feature_is_present():
    cases.check_feature_present()
