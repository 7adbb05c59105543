"""CPU: the wide nearest-centroid search (csrc/vq_wide.inc) on the kernel interpreter -- through the C entry, hip/vq.py, the
quantiser modules, KMeansVQGANEmb and EmbVQGANTrainer (cases and references: tests/_kmeanscases.py; the same, with the wider
shapes, on the GPU: tests/test_gpu_kmeans.py)."""
import os
import subprocess

import pytest

import _kmeanscases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')
DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emulator():
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    lib.use_library_for_tests(EMU)
    assert lib.backend() == 'emu'
    yield
    lib._lib, lib._host_pointers_ok = saved


# the wide shapes at N = 256 take the launcher's own choice on the interpreter; every instantiation runs at the small N below
@pytest.mark.parametrize('s', cases.EMU_SHAPES, ids=['d%d K%d' % cases.WIDE_SHAPES[s] for s in cases.EMU_SHAPES])
def test_wide_shapes_match_float64(s):
    cases.check_wide_shape(DEV, s, splits=(0,) if cases.WIDE_SHAPES[s][0] >= 1024 else cases.SPLITS)


@pytest.mark.parametrize('n', cases.SMALL_N)
def test_frame_counts_that_fill_no_tile(n):
    cases.check_wide_shape(DEV, cases.SMALL_N_SHAPE, n)


def test_first_minimum_across_tiles_and_waves():
    cases.check_first_minimum(DEV)


@pytest.mark.parametrize('K', [17, 100])
def test_phantom_columns_of_the_partial_last_tile_cannot_win(K):
    cases.check_partial_last_tile(DEV, K)


def test_every_d_slice_counts():
    cases.check_d_slices(DEV, 272)


def test_refused_arguments_and_untouched_rows():
    cases.check_refusals_and_guards(DEV)


def test_routing_keeps_every_served_shape_on_its_kernel():
    cases.check_routing(DEV)


@pytest.mark.parametrize('dim,K', [(64, 24), (272, 100)])
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
