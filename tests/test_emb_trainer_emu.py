"""CPU: ``EmbVQGANTrainer`` over the kernel interpreter against the restated reference step (cases, reference and bar:
tests/_embcases.py; the same on the GPU: tests/test_gpu_emb_trainer.py)."""
import os
import subprocess

import pytest
import torch

import _embcases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu', 'libmsmc_emu.so')
DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emulator():
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'tests', 'emu')])
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok, torch.get_num_threads())
    lib.use_library_for_tests(EMU)
    assert lib.backend() == 'emu'
    torch.set_num_threads(4)
    yield
    lib._lib, lib._host_pointers_ok = saved[:2]
    torch.set_num_threads(saved[2])


# every fibre of the vocoder and the discriminators is interpreted: a GAN-phase case takes about a minute here, so the interpreter
# runs it without the reference encoder only; with the encoder it runs on the GPU (tests/test_gpu_emb_trainer.py has the full matrix)
PHASES = [(0, False), (0, True), (1, False), (1, True), (2, False)]


@pytest.mark.parametrize('phase,global_encoder', PHASES,
                         ids=['%s-%s' % (('frames', 'spectral', 'gan')[p], 'ecapa' if g else 'plain') for p, g in PHASES])
def test_step_matches_the_restated_reference_step(phase, global_encoder):
    cases.check_phase(DEV, phase, global_encoder)


def test_trainer_task_dataset_and_synthetic_batch_resolve_and_refusals_raise():
    cases.check_construction(DEV)


def test_model_window_forms_equal_the_slice_stack_chain():
    cases.check_model_window_forms(DEV)


def test_emb_dataset_collation():
    cases.check_dataset_collation()
