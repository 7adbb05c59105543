"""CPU: the speaker reference encoder (networks/vqgantts/tdnn.py ECAPA_TDNN) and MSMCVQGANEmb with it, on the kernel interpreter,
against the reference's own outputs (cases: tests/_ecapacases.py; the same on the GPU: tests/test_gpu_tdnn.py)."""
import os
import subprocess

import pytest

import _ecapacases

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


def test_encoder_matches_the_reference_on_the_kernels():
    _ecapacases.check_encoder(DEV)


def test_stock_operator_form_matches_the_reference_too():
    _ecapacases.check_encoder(DEV, use_hip=False)


def test_kernel_and_stock_paths_agree_on_the_same_weights():
    _ecapacases.check_paths_agree(DEV)


def test_construction_refusals_and_no_silent_fallback():
    _ecapacases.check_construction_and_path_policy(DEV)


def test_autoencoder_with_the_global_encoder_matches_the_reference():
    _ecapacases.check_autoencoder(DEV)
