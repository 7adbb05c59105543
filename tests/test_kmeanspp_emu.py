"""CPU: the k-means++ seeding (csrc/kmeans_pp.hip, msmctts_amd/hip/kmeans.py) on the kernel interpreter -- the seeding against its
numpy restatement bit for bit, the edge cases of the draw, refusals, ``fit_kmeans(init='k-means++')`` and the command-line tool
(cases and references: tests/_kmeansppcases.py; the same on the GPU: tests/test_gpu_kmeanspp.py).  The (1024, 3000, 100, 6) case
takes minutes on the interpreter: (1024, 600, 8, 3) stands in for it here, the fits run the two smaller blob cases, and the
repeated calls of the determinism check run three small shapes (the GPU file runs every shape)."""
import os
import subprocess

import pytest

import _kmeansppcases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')
DEV = 'cpu'
FITS = (0, 1)
FIT_IDS = cases.fitcases.FIT_IDS[:2]
SHAPE_IDS = [cases.IDS[s] for s in cases.EMU_CASES]


@pytest.fixture(scope='module', autouse=True)
def emulator():
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    lib.use_library_for_tests(EMU)
    assert lib.backend() == 'emu'
    yield
    lib._lib, lib._host_pointers_ok = saved


def test_the_feature_is_present():
    cases.check_feature_present()


@pytest.mark.parametrize('s', cases.EMU_CASES, ids=SHAPE_IDS)
def test_seeding_matches_the_restated_order_bit_for_bit(s):
    cases.check_shape(DEV, s)


def test_edge_uniforms_pick_frames_of_non_zero_weight():
    cases.check_edge_uniforms(DEV)


def test_fewer_distinct_frames_than_centres():
    cases.check_duplicates(DEV)


@pytest.mark.parametrize('s', (0, 1, 3), ids=[cases.IDS[s] for s in (0, 1, 3)])
def test_seeding_is_deterministic_and_stays_inside_its_buffers(s):
    cases.check_determinism(DEV, s)


def test_default_local_trials():
    cases.check_default_local_trials()


def test_refused_arguments_leave_the_buffers_alone():
    cases.check_refusals(DEV)


@pytest.mark.parametrize('i', FITS, ids=FIT_IDS)
def test_fit_from_the_seeding_is_the_fit_from_its_rows(i):
    cases.check_fit(DEV, i)


@pytest.mark.parametrize('i', FITS, ids=FIT_IDS)
def test_host_frames_are_seeded_from_a_sample(i):
    cases.check_fit_seeds_from_a_sample(DEV, i)


@pytest.mark.parametrize('i', FITS, ids=FIT_IDS)
def test_fit_without_seeding_is_unchanged(i):
    cases.check_fit_without_seeding_is_unchanged(DEV, i)


def test_command_line_tool_seeds_a_file_the_quantiser_loads(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_float64_restatement_against_scikit_learn():
    pytest.importorskip('sklearn.cluster')
    cases.check_reference_against_sklearn()
