"""GPU: the streamed exact codeword search (csrc/vq_stream.inc) on the MI355X -- the cases of tests/_vqstreamcases.py (the same on
the interpreter: tests/test_vq_stream_emu.py), plus the hipGraph-replayed train step."""
import pytest

import _vqstreamcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('s,n', cases.SAME_PARAMS, ids=cases.SAME_IDS)
def test_forced_chunks_give_the_bits_of_the_resident_kernel(s, n):
    cases.check_same_bits_as_resident(DEV, s, n)


def test_lds_tile_family_gives_the_bits_of_the_lds_tile_kernel():
    cases.check_lds_tile_family_same_bits(DEV)


@pytest.mark.parametrize('H,d,K', [(1, 64, 64), (2, 128, 128)], ids=['H1 d64 K64', 'H2 d128 K128'])
def test_first_minimum_holds_across_chunk_boundaries(H, d, K):
    cases.check_first_minimum_across_chunks(DEV, H, d, K)


@pytest.mark.parametrize('s,n', cases.LARGE_PARAMS, ids=cases.LARGE_IDS)
def test_codebooks_larger_than_lds_match_float64(s, n):
    cases.check_large_shape(DEV, s, n)


@pytest.mark.parametrize('m', range(len(cases.MODULES)), ids=cases.MODULE_IDS)
def test_quantiser_modules_with_a_large_codebook_match_the_restated_reference(m):
    cases.check_module(DEV, m)


def test_one_warmup_and_one_gan_step_with_a_large_codebook():
    cases.check_train_steps(DEV)


def test_gan_step_replayed_from_graphs_matches_eager():
    cases.check_graphed_step_matches_eager(DEV)


def test_refused_arguments_and_the_empty_input():
    cases.check_refusals(DEV)


def test_wrapper_threads_the_chunk():
    cases.check_wrapper_threads_the_chunk(DEV)


def test_the_symbol_is_exported():
    cases.check_feature_present()
