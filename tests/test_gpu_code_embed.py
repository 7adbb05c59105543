"""GPU: the stored-code path of the main model on the MI355X -- csrc/code_embed.hip, hip/code_embed.py,
``MultiStageQuantizer.embed_codes``, ``MSMCVQGANEmb.analysis_codes`` / ``synthesis_codes``, ``EmbPredictorTrainer``,
``NASynTTSEmb.predict`` and tools/extract_codes.py: every case of tests/_codeembedcases.py (all but the strided-grid size also on
the interpreter: tests/test_code_embed_emu.py)."""
import pytest

import _codeembedcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('i64', [False, True], ids=['int32', 'int64'])
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', cases.SMALL)
def test_kernel_matches_the_restatement(name, bf16, i64):
    cases.check_case(DEV, name, bf16, i64)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_workgroups_stride_over_the_blocks(bf16):
    cases.check_case(DEV, 'strided grid', bf16, False)


def test_misaligned_codebook_takes_the_element_path():
    cases.check_misaligned(DEV)


def test_refusals_launch_nothing():
    cases.check_refusals(DEV)


def test_host_layer():
    cases.check_host_layer(DEV)


@pytest.mark.parametrize('n_heads,norm', [(2, False), (1, False), (2, True)], ids=['heads2', 'heads1', 'norm'])
def test_analysis_codes_against_analysis(n_heads, norm):
    cases.check_model(DEV, n_heads, norm)


def test_synthesis_codes():
    cases.check_synthesis_codes(DEV)


def test_trainer_step_on_codes_equals_the_parent_chain():
    cases.check_trainer_step(DEV)


def test_trainer_step_on_frames():
    cases.check_trainer_frames(DEV)


def test_trainer_refusals():
    cases.check_trainer_refusals(DEV)


def test_trainer_names_resolve():
    cases.check_trainer_names(DEV)


def test_task_predict_passes_ref():
    cases.check_task_predict(DEV)


def test_extract_codes(tmp_path):
    cases.check_extract_codes(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
