"""GPU: the EMA update of one wide head (csrc/ema_wide.hip, msmctts_amd/hip/vq.py, Quantize.ema_wide) on the MI355X -- the cases of
tests/_emawidecases.py (the same on the interpreter: tests/test_ema_wide_emu.py)."""
import pytest

import _emawidecases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_the_feature_is_present():
    cases.check_feature_present()


@pytest.mark.parametrize('s', range(len(cases.SHAPES)), ids=cases.IDS)
def test_updates_match_the_restated_order_and_float64(s):
    cases.check_shape(DEV, s)


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


@pytest.mark.parametrize('dim,K', [(528, 24)])
def test_codebook_sync_gives_the_fused_bits(dim, K):
    cases.check_sync_path(DEV, dim, K)
