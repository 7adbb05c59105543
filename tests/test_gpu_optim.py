"""GPU: the clip + AdamW kernels (csrc/optim.hip) on the MI355X -- the cases of tests/_optimcases.py (the same on the
interpreter: tests/test_optim_emu.py)."""
import pytest

import _optimcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('which', ('all', 'one', 'two', 'empty'))
def test_every_size_and_empty_tensors(which):
    cases.check_sizes(DEV, which)


def test_table_of_302_tensors_and_305_blocks():
    cases.check_long_table(DEV)


@pytest.mark.parametrize('offs', cases.ALIGN, ids=['p%dg%dm%dv%d' % o for o in cases.ALIGN])
def test_operand_alignment(offs):
    cases.check_alignment(DEV, offs)


@pytest.mark.parametrize('name', sorted(cases.STATES))
def test_states_steps_betas_and_decay(name):
    cases.check_state(DEV, name)


@pytest.mark.parametrize('write_grads', (0, 1))
@pytest.mark.parametrize('name', cases.CLIPS)
def test_clip(name, write_grads):
    cases.check_clip(DEV, name, write_grads)


def test_refusals_write_nothing():
    cases.check_refusals(DEV)


def test_host_layer_three_steps_with_offset_gradient_views():
    cases.check_host_layer(DEV)
