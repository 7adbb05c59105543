"""CPU: the EMA update of one wide head (csrc/ema_wide.hip, msmctts_amd/hip/vq.py, Quantize.ema_wide) on the kernel interpreter --
the cases of tests/_emawidecases.py (the same on the GPU: tests/test_gpu_ema_wide.py).  The two largest shapes run one update
here, three on the GPU."""
import os
import subprocess

import pytest

import _emawidecases as cases

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


def test_the_feature_is_present():
    cases.check_feature_present()


@pytest.mark.parametrize('s', range(len(cases.SHAPES)), ids=cases.IDS)
def test_updates_match_the_restated_order_and_float64(s):
    cases.check_shape(DEV, s, updates=1 if s in cases.LARGE else cases.UPDATES)


@pytest.mark.parametrize('s', [1, 2, 3], ids=[cases.IDS[s] for s in (1, 2, 3)])
def test_padded_frames_are_never_read(s):
    cases.check_padding_is_never_read(DEV, s)


@pytest.mark.parametrize('s', range(len(cases.SHAPES)), ids=cases.IDS)
def test_stats_then_apply_is_update_and_calls_repeat(s):
    cases.check_halves_and_repeat(DEV, s)


@pytest.mark.parametrize('s', cases.BOTH, ids=[cases.IDS[s] for s in cases.BOTH])
def test_against_the_resident_kernels(s):
    cases.check_against_resident(DEV, s)


def test_refused_arguments_leave_the_buffers_alone():
    cases.check_refusals(DEV)


@pytest.mark.parametrize('dim,K', [(528, 24), (1024, 100)])
def test_quantize_trains_with_the_flag(dim, K):
    cases.check_module(DEV, dim, K)


def test_the_flag_is_opt_in():
    cases.check_flag_is_opt_in(DEV)


@pytest.mark.parametrize('dim,K', [(528, 24)])
def test_codebook_sync_gives_the_fused_bits(dim, K):
    cases.check_sync_path(DEV, dim, K)


def test_trainer_keyword_sets_the_flag():
    cases.check_trainer_keyword()
