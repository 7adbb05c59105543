"""CPU: the LayerNorm, gate and glue kernels (csrc/norm.hip) on the kernel interpreter, through the C entries and once through
hip/norm.py, against float64 references built from stock torch operators (cases, references and bars: tests/_normcases.py; the
same on the GPU: tests/test_gpu_norm.py)."""
import os
import subprocess

import pytest

import _normcases as cases

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


BOTH = (0, 1)
NAMES = ['fp32', 'bf16']
SHAPE_ID = lambda s: 'x'.join(str(v) for v in s)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('shape', cases.LN_FWD_SHAPES, ids=SHAPE_ID)
def test_add_layer_norm_forward_against_float64(shape, which):
    cases.check_ln_fwd(DEV, shape[0], shape[1], which)


@pytest.mark.parametrize('eps', (1e-5, 1e-12, 1e-2))
@pytest.mark.parametrize('C', (256, 67))
def test_add_layer_norm_forward_planted_rows(C, eps):
    cases.check_ln_planted(DEV, C, eps)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('shape', cases.LN_BWD_SHAPES, ids=SHAPE_ID)
def test_add_layer_norm_backward_against_float64_autograd(shape, which):
    cases.check_ln_bwd(DEV, shape[0], shape[1], which)


def test_parameter_gradients_of_many_layer_norms_in_one_call():
    cases.check_param_multi(DEV)


def test_backward_entries_refuse_a_short_workspace_and_p_drop_outside_0_1():
    cases.check_ln_bwd_refusals(DEV)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
def test_misaligned_rows_take_the_element_path(which):
    cases.check_misaligned(DEV, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('C', (256, 67))
def test_layer_norm_dropout_uses_the_shared_mask(C, which):
    cases.check_dropout_ln(DEV, C, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
def test_gate_and_dropout_backward_use_the_shared_mask(which):
    cases.check_dropout_gate_and_bwd(DEV, which)


def test_mask_seeding_and_keep_rate():
    cases.check_seeding_and_rate(DEV)


@pytest.mark.parametrize('n', range(len(cases.FC_SHAPES)), ids=[SHAPE_ID(s) for s in cases.FC_SHAPES])
def test_fused_projection_and_layer_norm_against_float64(n):
    cases.check_fc(DEV, n)


def test_fused_projection_and_layer_norm_dropout_uses_the_shared_mask():
    cases.check_fc_dropout(DEV)


def test_fused_projection_and_layer_norm_refusals():
    cases.check_fc_refusals(DEV)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('shape', cases.GATE_SHAPES, ids=SHAPE_ID)
def test_gate_and_its_gradient_against_float64(shape, which):
    cases.check_gate(DEV, shape[0], shape[1], which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
def test_gate_stays_finite_where_expf_overflows(which):
    cases.check_gate_overflow(DEV, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('n', cases.TANH_SIZES)
def test_tanh_family_against_float64(n, which):
    cases.check_tanh(DEV, n, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('n', cases.GLUE_SIZES)
def test_sum_n_and_dropout_add_are_the_rounded_fp32_sum(n, which):
    cases.check_sum_n(DEV, n, which)


def test_glue_refusals():
    cases.check_glue_refusals(DEV)


@pytest.mark.parametrize('shape', cases.ROW_MASK_SHAPES, ids=SHAPE_ID)
def test_row_mask_equals_arange_below_length(shape):
    cases.check_row_mask(DEV, shape[0], shape[1])


def test_grid_stride_kernels_past_the_interpreters_grid_cap():
    cases.check_past_cap(DEV, cases.past_cap_emu())


@pytest.mark.parametrize('n', range(len(cases.PROLOGUE_SHAPES)), ids=[SHAPE_ID(s) for s in cases.PROLOGUE_SHAPES])
def test_fft_prologue_against_float64(n):
    cases.check_prologue(DEV, n)


def test_host_layer_defers_and_accumulates_parameter_gradients():
    cases.check_host_route(DEV)
