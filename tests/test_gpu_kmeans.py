"""GPU: the wide nearest-centroid search (csrc/vq_wide.inc), KMeansVQGANEmb and its EmbVQGANTrainer steps on the MI355X -- the
cases of tests/_kmeanscases.py (the smaller ones also on the interpreter: tests/test_kmeans_emu.py)."""
import pytest

import _kmeanscases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('s', range(len(cases.WIDE_SHAPES)), ids=['d%d K%d' % sh for sh in cases.WIDE_SHAPES])
def test_wide_shapes_match_float64(s):
    cases.check_wide_shape(DEV, s)


@pytest.mark.parametrize('n', cases.SMALL_N)
def test_frame_counts_that_fill_no_tile(n):
    cases.check_wide_shape(DEV, cases.SMALL_N_SHAPE, n)


def test_first_minimum_across_tiles_and_waves():
    cases.check_first_minimum(DEV)


@pytest.mark.parametrize('K', [17, 100])
def test_phantom_columns_of_the_partial_last_tile_cannot_win(K):
    cases.check_partial_last_tile(DEV, K)


@pytest.mark.parametrize('d', [272, 1040])
def test_every_d_slice_counts(d):
    cases.check_d_slices(DEV, d)


def test_refused_arguments_and_untouched_rows():
    cases.check_refusals_and_guards(DEV)


def test_routing_keeps_every_served_shape_on_its_kernel():
    cases.check_routing(DEV)


@pytest.mark.parametrize('dim,K', [(64, 24), (272, 100), (1024, 100)])
def test_module_gradient_matches_the_restated_forward(dim, K):
    cases.check_module_gradient(DEV, dim, K)


def test_model_surface(tmp_path):
    cases.check_model_surface(DEV, tmp_path)


def test_model_matches_the_reference_fixture(tmp_path):
    cases.check_model_parity(DEV, tmp_path)


@pytest.mark.parametrize('phase', [0, 1, 2])
def test_trainer_steps_without_a_vq_term(tmp_path, phase):
    cases.check_trainer_phase(DEV, tmp_path, phase)


def test_the_feature_is_present():
    cases.check_feature_present()
