"""GPU: the weight-norm, column-sum, reflect-fold and leaky-ReLU kernels (csrc/wnorm.hip) on the MI355X -- the cases of
tests/_wnormcases.py (the same on the interpreter: tests/test_wnorm_emu.py) and the fold sizes past the grid caps of the MI355X
(16 * 256 * 256 items of the grouped form, 4096 * 256 elements of the single one)."""
import pytest

import _wnormcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


BOTH = (0, 1)
NAMES = ['fp32', 'bf16']


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('entry', cases.PREP_ENTRIES)
def test_weight_norm_prepare_against_float64(entry, which):
    cases.check_prepare(DEV, which, entry)


def test_weight_norm_prepare_refusals():
    cases.check_prepare_refusals(DEV)


@pytest.mark.parametrize('accumulate', (0, 1))
@pytest.mark.parametrize('table,max_row', (('small', 4000), ('small', 0), ('large', 7175), ('large', 0)))
def test_weight_norm_backward_against_float64_autograd(table, max_row, accumulate):
    cases.check_backward(DEV, table, accumulate, max_row)


def test_weight_norm_backward_refusals():
    cases.check_backward_refusals(DEV)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('C', cases.COLSUM_C)
def test_column_sums_against_float64(C, which):
    cases.check_colsum(DEV, C, which)


@pytest.mark.parametrize('rows', (cases.COLSUM_CAP_ROWS, cases.colsum_fewer()))
@pytest.mark.parametrize('C,which', cases.COLSUM_BIG)
def test_column_sums_past_the_block_cap(C, which, rows):
    assert rows is not None and rows > 256 * 128
    cases.check_colsum(DEV, C, which, (rows,))


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('C', (3, 4, 64, 257))
def test_atomic_column_sums_against_float64(C, which):
    cases.check_colsum_atomic(DEV, C, which)


def test_column_sum_refusals():
    cases.check_colsum_refusals(DEV)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('C', sorted(cases.FOLD_P))
def test_reflect_fold_against_float64_autograd(C, which):
    cases.check_fold_channels(DEV, C, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('key', sorted(cases.FOLD_SPECIAL))
def test_reflect_fold_groups_choose_the_vector_every_member_allows(key, which):
    cases.check_fold_special(DEV, key, which)


def test_reflect_fold_refusals():
    cases.check_fold_refusals(DEV)


def test_reflect_fold_past_the_grid_cap():
    cases.check_fold_past_cap(DEV, cases.FOLD_CAP_GPU)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
@pytest.mark.parametrize('n', cases.LRELU_SIZES)
def test_leaky_relu_backward_is_exact(n, which):
    cases.check_lrelu(DEV, n, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
def test_leaky_relu_backward_groups(which):
    cases.check_lrelu_groups(DEV, which)


@pytest.mark.parametrize('which', BOTH, ids=NAMES)
def test_leaky_relu_backward_group_of_misaligned_views(which):
    cases.check_lrelu_misaligned(DEV, which)


def test_leaky_relu_backward_refusals():
    cases.check_lrelu_refusals(DEV)


def test_host_layer_column_sums_folds_and_groups():
    cases.check_host_colsum_and_folds(DEV)


def test_host_layer_weight_normalised_layer_through_the_bank():
    cases.check_host_weight_norm_layer(DEV)
