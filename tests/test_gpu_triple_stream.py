"""GPU: the streamed triple loss (csrc/triple_stream.inc) on the MI355X -- the cases of tests/_triplestreamcases.py (the same on
the interpreter: tests/test_triple_stream_emu.py), plus the hipGraph-replayed predictor step."""
import pytest

import _triplestreamcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('s,n', cases.SAME_PARAMS, ids=cases.SAME_IDS)
def test_forced_chunks_give_the_bits_of_the_resident_kernel(s, n):
    cases.check_same_bits_as_resident(DEV, s, n)


@pytest.mark.parametrize('s,n', cases.LARGE_PARAMS, ids=cases.LARGE_IDS)
def test_large_shapes_do_not_depend_on_the_chunk(s, n):
    cases.check_chunk_invariance(DEV, s, n)


@pytest.mark.parametrize('s,n', cases.LARGE_PARAMS, ids=cases.LARGE_IDS)
def test_large_shapes_are_exact_on_an_integer_lattice(s, n):
    cases.check_lattice(DEV, s, n)


@pytest.mark.parametrize('s,n', cases.LARGE_PARAMS, ids=cases.LARGE_IDS)
def test_large_shapes_match_float64_within_the_derived_budget(s, n):
    cases.check_real_values(DEV, s, n)


@pytest.mark.parametrize('m', range(len(cases.MODULES)), ids=cases.MODULE_IDS)
def test_quantiser_modules_take_the_streamed_kernel(m):
    cases.check_module(DEV, m)


def test_predictor_step_against_a_large_codebook_matches_the_oracle():
    cases.check_predictor_step(DEV)


def test_predictor_step_replayed_from_graphs_gives_the_eager_losses():
    cases.check_graphed_predictor_step_matches_eager(DEV)


def test_refused_arguments_and_the_empty_input():
    cases.check_refusals(DEV)


def test_wrapper_routes_between_the_two_entries():
    cases.check_wrapper_routes(DEV)


def test_the_symbols_are_exported_and_bound():
    cases.check_feature_present()
