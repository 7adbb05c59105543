"""GPU: unit extraction on the MI355X -- the labels-only wide assignment (csrc/vq_assign.inc), run collapse and code usage
(csrc/units.hip), hip/units.py, ``KMeansQuantizer.units`` and tools/extract_units.py: the cases of tests/_unitscases.py (the
smaller ones also on the interpreter: tests/test_units_emu.py)."""
import pytest

import _unitscases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('N', cases.FRAMES)
@pytest.mark.parametrize('s', range(len(cases.SHAPES)), ids=cases.IDS)
def test_labels_are_the_wide_searchs_and_dist_the_documented_sum(s, N):
    cases.check_labels_and_dist(DEV, s, N)


def test_a_frame_on_its_centroid_weighs_exactly_zero():
    cases.check_exact_zeros(DEV)


def test_identical_centroids_lowest_index_wins():
    cases.check_ties(DEV)


def test_without_a_distance_buffer_only_the_labels_are_written():
    cases.check_null_distance(DEV)


def test_refused_arguments_launch_nothing():
    cases.check_refusals(DEV)


@pytest.mark.parametrize('T', cases.COLLAPSE_T)
def test_collapse_matches_the_restatement(T):
    cases.check_collapse(DEV, T)


def test_collapse_and_usage_refuse_empty_shapes():
    cases.check_collapse_refusals(DEV)


@pytest.mark.parametrize('K', [1, 100, 5000])
def test_usage_is_the_bincount_of_the_valid_frames(K):
    cases.check_usage(DEV, K)


def test_usage_summary_is_the_reference_scripts_formula():
    cases.check_usage_summary()


def test_assign_units_takes_arrays_host_and_device_tensors_in_any_block():
    cases.check_assign_units_inputs(DEV)


def test_assign_units_takes_centres_in_every_form(tmp_path):
    cases.check_assign_units_centres(DEV, tmp_path)


def test_quantizer_units_are_the_indices_of_forward(tmp_path):
    cases.check_quantizer_units(DEV, tmp_path)


def test_extract_units_tool(tmp_path):
    cases.check_tool(DEV, tmp_path)


def test_the_feature_is_present():
    cases.check_feature_present()
