"""GPU: the k-means fit (csrc/kmeans.hip, msmctts_amd/hip/kmeans.py) on the MI355X -- the cases of tests/_kmeansfitcases.py (the
same on the interpreter: tests/test_kmeans_fit_emu.py)."""
import pytest

import _kmeansfitcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FITS = range(len(cases.FIT_SHAPES))


def test_the_feature_is_present():
    cases.check_feature_present()


@pytest.mark.parametrize('s', range(len(cases.STATS_SHAPES)), ids=cases.STATS_IDS)
def test_statistics_match_the_restated_order_and_float64(s):
    cases.check_stats_shape(DEV, s)


def test_labels_outside_the_codebook_are_skipped():
    cases.check_skipped_labels(DEV)


def test_no_frames():
    cases.check_no_frames(DEV)


def test_rows_beyond_the_sizes_stay_untouched():
    cases.check_oversized_buffers(DEV)


def test_blocks_accumulate_in_order():
    cases.check_accumulate(DEV)


def test_refused_arguments_leave_the_buffers_alone():
    cases.check_refusals(DEV)


def test_workspace_grows_with_frames_and_runs_only():
    cases.check_workspace_size()


@pytest.mark.parametrize('d,K', [(4, 3), (272, 24), (1024, 100), (2048, 5)])
def test_update_divides_and_measures_the_movement(d, K):
    cases.check_update(DEV, d, K)


@pytest.mark.parametrize('i', FITS, ids=cases.FIT_IDS)
def test_one_lloyd_step(i):
    cases.check_one_step(DEV, i)


@pytest.mark.parametrize('i', FITS, ids=cases.FIT_IDS)
def test_fit_is_deterministic(i):
    cases.check_fit_is_deterministic(DEV, i)


@pytest.mark.parametrize('i', FITS, ids=cases.FIT_IDS)
def test_fit_in_blocks_of_97_frames(i):
    cases.check_fit_in_blocks(DEV, i)


@pytest.mark.parametrize('i', FITS, ids=cases.FIT_IDS)
def test_fit_properties(i):
    cases.check_fit_properties(DEV, i)


def test_command_line_tool_writes_a_file_the_model_loads(tmp_path):
    cases.check_tool(DEV, tmp_path)


@pytest.mark.parametrize('i', FITS, ids=cases.FIT_IDS)
def test_saved_file_is_what_the_quantiser_loads(i, tmp_path):
    cases.check_saved_file_is_the_quantisers(DEV, i, tmp_path)


@pytest.mark.parametrize('i', FITS, ids=cases.FIT_IDS)
def test_final_inertia_against_float64_lloyd(i):
    cases.check_final_inertia(DEV, i)
