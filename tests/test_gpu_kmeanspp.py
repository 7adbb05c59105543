"""GPU: the k-means++ seeding (csrc/kmeans_pp.hip, msmctts_amd/hip/kmeans.py) on the MI355X -- the cases of
tests/_kmeansppcases.py (the same on the interpreter: tests/test_kmeanspp_emu.py)."""
import pytest

import _kmeansppcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FITS = range(len(cases.fitcases.FIT_SHAPES))
FIT_IDS = cases.fitcases.FIT_IDS
SHAPE_IDS = [cases.IDS[s] for s in cases.GPU_CASES]


def test_the_feature_is_present():
    cases.check_feature_present()


@pytest.mark.parametrize('s', cases.GPU_CASES, ids=SHAPE_IDS)
def test_seeding_matches_the_restated_order_bit_for_bit(s):
    cases.check_shape(DEV, s)


def test_edge_uniforms_pick_frames_of_non_zero_weight():
    cases.check_edge_uniforms(DEV)


def test_fewer_distinct_frames_than_centres():
    cases.check_duplicates(DEV)


@pytest.mark.parametrize('s', cases.GPU_CASES, ids=SHAPE_IDS)
def test_seeding_is_deterministic_and_stays_inside_its_buffers(s):
    cases.check_determinism(DEV, s)


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
