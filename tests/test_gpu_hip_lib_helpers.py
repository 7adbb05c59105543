"""GPU: the host layer between the modules of msmctts_amd/hip and the C ABI on the MI355X -- the cases of tests/_hiplibcases.py
that take a device (all of them on the interpreter: tests/test_hip_lib_helpers.py)."""
import pytest

import _hiplibcases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_call_runs_what_is_installed_on_the_handle():
    cases.check_call_runs_what_is_installed_on_the_handle(DEV)


def test_workspace_reuses_or_allocates():
    cases.check_workspace(DEV)


def test_search_keeps_only_a_cast_for_the_ema_update():
    cases.check_search_keeps_only_a_cast(DEV)
