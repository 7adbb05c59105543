"""GPU: the spectral front-end kernels (csrc/spectral.hip) on the MI355X -- the cases of tests/_spectralcases.py (the same on the
interpreter: tests/test_spectral_emu.py) and the two shapes past the 2048-workgroup cap of the launch grid."""
import pytest

import _spectralcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


FRAMES = range(len(cases.FRAME_CASES))
MAGS = [(c, m) for c in cases.MAG_CASES + cases.MAG_CASES_GPU for m in (1, 0)]
MAG_IDS = ['R%d F%d CP%d FP%d mode %d' % (c + (m,)) for c, m in MAGS]
IMAGES = [(n, d) for n in range(len(cases.IMAGE_CASES)) for d in range(len(cases.IMAGE_DTYPES))]
IMAGE_IDS = ['B%d T%d F%d FP%d %s' % (cases.IMAGE_CASES[n] + (cases.IMAGE_DTYPES[d][2],)) for n, d in IMAGES]


@pytest.mark.parametrize('n', FRAMES, ids=cases.FRAME_IDS)
def test_frames_equal_reflect_pad_and_unfold_bit_for_bit(n):
    cases.check_frames_forward(DEV, n)


@pytest.mark.parametrize('n', FRAMES, ids=cases.FRAME_IDS)
def test_overlap_add_equals_the_float64_gradient_of_pad_and_unfold(n):
    cases.check_frames_backward(DEV, n)


@pytest.mark.parametrize('case,mode', MAGS, ids=MAG_IDS)
def test_magnitude_and_its_gradient_within_the_derived_bounds(case, mode):
    cases.check_magnitude(DEV, case, mode)


@pytest.mark.parametrize('n,which', IMAGES, ids=IMAGE_IDS)
def test_two_channel_image_and_its_gradient_within_the_derived_bounds(n, which):
    cases.check_image(DEV, n, which)


@pytest.mark.parametrize('n', cases.LOG_SIZES + cases.LOG_SIZES_GPU)
def test_log_clamp_and_its_gradient_within_the_derived_bounds(n):
    cases.check_log_clamp(DEV, n)


def test_one_launch_of_several_stages_equals_the_single_entries_bit_for_bit():
    cases.check_multi(DEV)


@pytest.mark.parametrize('n', range(len(cases.CHAIN_CASES)), ids=cases.CHAIN_IDS)
def test_chains_within_four_times_the_error_of_the_fp32_torch_chain(n):
    cases.check_chain(DEV, n)


def test_frames_past_the_single_reflection_are_refused():
    cases.check_frames_past_the_reflection_are_refused(DEV)


def test_every_shape_of_the_host_layer_is_accepted():
    cases.check_host_shapes_are_accepted(DEV)


def test_rejected_arguments_return_the_shape_error():
    cases.check_rejected_arguments(DEV)
