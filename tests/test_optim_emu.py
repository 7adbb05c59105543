"""CPU: the clip + AdamW kernels (csrc/optim.hip) on the kernel interpreter, through msmc_opt_clip_adamw with hand-built tensor
tables and once through trainers/optimizers/hip_adamw.py, against a float64 reference that is itself pinned to torch.optim.AdamW
(cases, references and bars: tests/_optimcases.py; the same on the GPU: tests/test_gpu_optim.py)."""
import os
import subprocess

import pytest

import _optimcases as cases

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


def test_float64_reference_is_torch_adamw_after_clip_grad_norm():
    cases.check_reference_pins_torch()


def test_measured_error_of_fp32_power():
    ep = cases.eps_pow()
    print('optim eps_pow = %.3f u (4 x the measured %.3f u)' % (ep / cases.U, ep / cases.U / 4))
    assert 0 < ep <= 16 * cases.U


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
