"""CPU: the unit-input path on the kernel interpreter -- runs back to labels (csrc/units.hip), the decoder input from labels and
its gradient (csrc/unit_embed.hip), hip/units.py, ``KMeansVQGANEmb.forward_units`` / ``synthesis_units``, the unit batch of
``EmbVQGANTrainer`` and tools/synthesize_units.py (cases and references: tests/_unitembedcases.py; the same, with the wide
shapes, on the GPU: tests/test_gpu_unit_embed.py)."""
import os
import subprocess

import pytest

import _unitembedcases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')
DEV = 'cpu'
SMALL_FWD = [s for s, (B, T, C, K) in enumerate(cases.FWD_SHAPES) if B * T * C <= 3 * 257 * 64]


@pytest.fixture(scope='module', autouse=True)
def emulator():
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    lib.use_library_for_tests(EMU)
    assert lib.backend() == 'emu'
    yield
    lib._lib, lib._host_pointers_ok = saved


@pytest.mark.parametrize('R', cases.EXPAND_R)
def test_expand_matches_the_restatement(R):
    cases.check_expand(DEV, R)


def test_expand_undoes_collapse():
    cases.check_expand_round_trip(DEV)


def test_expand_refuses_empty_shapes():
    cases.check_expand_refusals(DEV)


@pytest.mark.parametrize('s', SMALL_FWD, ids=[cases.FWD_IDS[s] for s in SMALL_FWD])
def test_embed_forward_is_the_gather_bit_for_bit(s):
    cases.check_embed_forward(DEV, s)


def test_embed_forward_with_more_blocks_than_the_grid():
    cases.check_embed_forward_strided_grid(DEV, 3, 257, 256, 2000)            # 25 blocks, 24 workgroups on the interpreter


def test_embed_forward_refusals_launch_nothing():
    cases.check_embed_forward_refusals(DEV)


def test_embed_backward_is_the_documented_sum():
    cases.check_embed_backward(DEV)


def test_embed_backward_refusals_and_short_workspace():
    cases.check_embed_backward_refusals(DEV)


def test_unit_embed_through_autograd():
    cases.check_autograd(DEV)


@pytest.mark.parametrize('global_encoder', [False, True], ids=['plain', 'global encoder'])
def test_forward_units_agrees_with_forward_on_centroid_frames(tmp_path, global_encoder):
    cases.check_model(DEV, tmp_path, global_encoder)


def test_synthesis_units_on_runs_is_synthesis_units_on_labels(tmp_path):
    cases.check_synthesis_units(DEV, tmp_path)


def test_trainer_steps_on_a_unit_batch(tmp_path):
    cases.check_trainer_phase(DEV, tmp_path, 0)


def test_trainer_refuses_a_model_without_forward_units():
    cases.check_trainer_needs_forward_units(DEV)


def test_unit_batch_and_collation():
    cases.check_unit_batch_and_collation()


def test_synthesize_units_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
