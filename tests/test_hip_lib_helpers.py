"""CPU: the host layer between the modules of msmctts_amd/hip and the C ABI on the kernel interpreter -- ``lib.call``,
``lib.workspace``, the cast a search keeps for the EMA update behind it, and the frame source of the k-means fit (cases:
tests/_hiplibcases.py; the ones that take a device run on the card in tests/test_gpu_hip_lib_helpers.py)."""
import os
import subprocess

import pytest

import _hiplibcases as cases

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


def test_call_passes_a_zero_return():
    cases.check_call_passes_a_zero_return(DEV)


def test_call_raises_with_the_name_or_the_label():
    cases.check_call_raises_on_a_code(DEV)


def test_call_of_an_unknown_name():
    cases.check_call_unknown_name()


def test_call_runs_what_is_installed_on_the_handle():
    cases.check_call_runs_what_is_installed_on_the_handle(DEV)


def test_workspace_reuses_or_allocates():
    cases.check_workspace(DEV)


def test_search_keeps_only_a_cast_for_the_ema_update():
    cases.check_search_keeps_only_a_cast(DEV)


def test_frame_source_reads_every_kind_alike():
    cases.check_frame_source_kinds()


def test_frame_source_refuses_other_ranks():
    cases.check_frame_source_refuses_other_ranks()
