"""The kernel chooser of hip/conv.py (``_tune``: which (variant, split_shift) a descriptor gets, and whether it was borrowed),
``_group_choice``, the round trip of the shipped decisions and the operand check -- on the CPU, with no library call: the
launches are stubs with a scripted return code per (variant, split_shift), the timings are scripted, the capture test is
patched and the interpreter is unbound (``lib._host_pointers_ok`` False) so that the chooser takes its GPU paths.  Every row
of the table in ``_tune``'s docstring is checked on the chosen fields, the launches, ``TUNED``, the budget and ``_borrowed``,
for a forward ('gather') and a weight-gradient ('wgrad') descriptor."""
import ctypes
import json
import os

import pytest
import torch

from msmctts_amd.hip import conv, lib

TAPS = ((0, 0, 0), (0, 1, 1), (0, 2, 2))
BUDGET = 5


class Untouchable(object):
    """stands for the bound library where no entry point may be reached"""
    def __getattr__(self, name):
        raise AssertionError('library entry %s reached' % name)


class Accepted(object):
    """a host tensor the operand check takes for one on the GPU"""
    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)


@pytest.fixture(autouse=True)
def tuner(monkeypatch):
    """an empty decision table, a small budget, timing allowed, no capture, the interpreter unbound, no library"""
    keep, budget = dict(conv.TUNED), conv.TUNE_BUDGET[0]
    conv.TUNED.clear()
    conv._CLASS_INDEXED[0] = -1
    conv.TUNE_BUDGET[0] = BUDGET
    monkeypatch.setattr(conv, 'AUTOTUNE', True)
    monkeypatch.setattr(conv, 'TUNE_BORROW', True)
    monkeypatch.setattr(conv, 'DEFER_TO', None)
    monkeypatch.setattr(conv, '_capturing', lambda: False)
    monkeypatch.setattr(lib, '_host_pointers_ok', False)
    monkeypatch.setattr(lib, '_lib', Untouchable())
    yield
    conv.TUNED.clear()
    conv.TUNED.update(keep)
    conv.TUNE_BUDGET[0] = budget
    conv._CLASS_INDEXED[0] = -1


def make_desc(T=400, dtype=torch.bfloat16, built=(7, 0)):
    d = conv._build_desc(dtype, 4, 1, T, 64, 1, T, 96, (1, T, 0, 1, 0, 1, 1, 1, 0, -1), TAPS, 0, 1.0, 1.0, 1.0, 1.0)
    d.variant, d.split_shift, d.dw_copies = built[0], built[1], 2
    return d


def sig_of(kind, desc):
    return (kind,) + conv._signature(desc)


class Launch(object):
    """stub launch of ``desc``: records the (variant, split_shift) it was issued with, returns the scripted code (0 unless
    listed in ``refuse``)"""
    def __init__(self, desc, refuse=()):
        self.desc, self.refuse, self.log = desc, set(refuse), []

    def __call__(self):
        c = (self.desc.variant, self.desc.split_shift)
        self.log.append(c)
        return 5 if c in self.refuse else 0


def scripted_times(monkeypatch, desc, ms):
    """``_time_ms`` issues its three launches and reports the scripted time of the candidate the descriptor holds"""
    def fake(fn):
        for _ in range(3):
            fn()
        return ms[(desc.variant, desc.split_shift)]
    monkeypatch.setattr(conv, '_time_ms', fake)


def state(desc):
    return (desc.variant, desc.split_shift), desc._tuned, desc._borrowed


KINDS = [('gather', False), ('wgrad', True)]


@pytest.mark.parametrize('kind,on_trust', KINDS)
def test_interpreter_bound_keeps_the_descriptor_as_built(kind, on_trust, monkeypatch):
    monkeypatch.setattr(lib, '_host_pointers_ok', True)
    desc = make_desc()
    conv.TUNED[sig_of(kind, desc)] = (19, 0, {})                  # (not even looked up)
    before = dict(conv.TUNED)
    launch = Launch(desc)
    conv._tune(kind, desc, launch, ((1, 0), (2, 0)), on_trust)
    assert state(desc) == ((7, 0), True, False) and launch.log == []
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET


@pytest.mark.parametrize('kind,on_trust', KINDS)
def test_exact_key_is_applied_without_a_launch(kind, on_trust):
    desc = make_desc()
    conv.TUNED[sig_of(kind, desc)] = (4, -1, {(4, -1): 0.1})
    before = dict(conv.TUNED)
    launch = Launch(desc)
    conv._tune(kind, desc, launch, ((1, 0), (2, 0)), on_trust)
    assert state(desc) == ((4, -1), True, False) and launch.log == []
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET


def test_forward_borrows_the_nearest_shape_with_one_validating_launch():
    desc = make_desc(T=380)
    conv.TUNED[sig_of('gather', make_desc(T=400))] = (19, 0, {})
    conv.TUNED[sig_of('gather', make_desc(T=100))] = (9, 0, {})
    before = dict(conv.TUNED)
    launch = Launch(desc)
    conv._tune('gather', desc, launch, ((1, 0), (2, 0)))
    assert state(desc) == ((19, 0), True, False) and launch.log == [(19, 0)]
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET


def test_forward_restores_a_refused_borrow_and_goes_on_to_the_next_rows(monkeypatch):
    conv.TUNED[sig_of('gather', make_desc(T=400))] = (19, 0, {})
    before = dict(conv.TUNED)
    # ... to the library heuristic while the stream is capturing
    monkeypatch.setattr(conv, '_capturing', lambda: True)
    desc = make_desc(T=380)
    launch = Launch(desc, refuse=[(19, 0)])
    conv._tune('gather', desc, launch, ((1, 0), (2, 0)))
    assert state(desc) == ((7, 0), True, False) and launch.log == [(19, 0)]
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET
    # ... to the timing row otherwise
    monkeypatch.setattr(conv, '_capturing', lambda: False)
    desc = make_desc(T=380)
    launch = Launch(desc, refuse=[(19, 0)])
    scripted_times(monkeypatch, desc, {(1, 0): 0.5, (2, 0): 0.25})
    conv._tune('gather', desc, launch, ((1, 0), (2, 0)))
    assert state(desc) == ((2, 0), True, False)
    assert launch.log == [(19, 0)] + [(1, 0)] * 4 + [(2, 0)] * 4
    assert conv.TUNED[sig_of('gather', desc)] == (2, 0, {(1, 0): 0.5, (2, 0): 0.25}) and len(conv.TUNED) == len(before) + 1
    assert conv.TUNE_BUDGET[0] == BUDGET - 1


def test_weight_gradient_takes_the_nearest_shape_on_trust():
    desc = make_desc(T=380)
    conv.TUNED[sig_of('wgrad', make_desc(T=400))] = (4, -1, {})
    conv.TUNED[sig_of('gather', make_desc(T=380))] = (19, 0, {})      # (another kind: not a neighbour)
    before = dict(conv.TUNED)
    launch = Launch(desc)
    conv._tune('wgrad', desc, launch, ((2, 0),), on_trust=True)
    assert state(desc) == ((4, -1), True, True) and launch.log == []
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET


@pytest.mark.parametrize('kind,on_trust', KINDS)
@pytest.mark.parametrize('why', ['autotune off', 'budget spent', 'capturing'])
def test_nothing_found_and_no_timing_leaves_the_library_heuristic(kind, on_trust, why, monkeypatch):
    if why == 'autotune off':
        monkeypatch.setattr(conv, 'AUTOTUNE', False)
    elif why == 'budget spent':
        conv.TUNE_BUDGET[0] = 0
    else:
        monkeypatch.setattr(conv, '_capturing', lambda: True)
    budget = conv.TUNE_BUDGET[0]
    desc = make_desc()
    launch = Launch(desc)
    conv._tune(kind, desc, launch, ((1, 0), (2, 0)), on_trust)
    assert state(desc) == ((7, 0), True, False) and launch.log == []
    assert conv.TUNED == {} and conv.TUNE_BUDGET[0] == budget


@pytest.mark.parametrize('kind,on_trust', KINDS)
def test_timing_keeps_the_fastest_candidate_that_ran(kind, on_trust, monkeypatch):
    desc = make_desc()
    launch = Launch(desc, refuse=[(2, 0)])
    scripted_times(monkeypatch, desc, {(1, 0): 0.5, (3, -1): 0.2, (4, 0): 0.3})
    conv._tune(kind, desc, launch, ((1, 0), (2, 0), (3, -1), (4, 0)), on_trust)
    assert state(desc) == ((3, -1), True, False)
    # one validating launch per candidate in list order, three timed ones behind it unless it was refused
    assert launch.log == [(1, 0)] * 4 + [(2, 0)] + [(3, -1)] * 4 + [(4, 0)] * 4
    assert conv.TUNED == {sig_of(kind, desc): (3, -1, {(1, 0): 0.5, (3, -1): 0.2, (4, 0): 0.3})}
    assert conv.TUNE_BUDGET[0] == BUDGET - 1


@pytest.mark.parametrize('kind,on_trust', KINDS)
def test_timing_with_no_candidate_that_runs_records_the_library_heuristic(kind, on_trust, monkeypatch):
    desc = make_desc()
    launch = Launch(desc, refuse=[(1, 0), (2, 0)])
    scripted_times(monkeypatch, desc, {})
    conv._tune(kind, desc, launch, ((1, 0), (2, 0)), on_trust)
    assert state(desc) == ((0, 0), True, False) and launch.log == [(1, 0), (2, 0)]
    assert conv.TUNED == {sig_of(kind, desc): (0, 0, {})} and conv.TUNE_BUDGET[0] == BUDGET - 1


def test_fp32_weight_gradient_ignores_a_neighbour_of_the_bf16_only_generations(monkeypatch):
    """variant >= 3 next to an fp32 descriptor: never taken on trust.  Without timing the fields stay as built; with timing
    allowed the neighbour gets one validating launch (the footnote of the table): refused -- what the library does with
    generation 3 in fp32 -- the candidates are timed; accepted, it is kept without a TUNED entry"""
    neighbour = sig_of('wgrad', make_desc(T=400, dtype=torch.float32))
    conv.TUNED[neighbour] = (3, -1, {})
    before = dict(conv.TUNED)
    monkeypatch.setattr(conv, '_capturing', lambda: True)
    desc = make_desc(T=380, dtype=torch.float32)
    launch = Launch(desc)
    conv._tune('wgrad', desc, launch, ((2, 0), (2, 1)), on_trust=True)
    assert state(desc) == ((7, 0), True, False) and launch.log == []
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET

    monkeypatch.setattr(conv, '_capturing', lambda: False)
    desc = make_desc(T=380, dtype=torch.float32)
    launch = Launch(desc, refuse=[(3, -1)])
    scripted_times(monkeypatch, desc, {(2, 0): 0.4, (2, 1): 0.3})
    conv._tune('wgrad', desc, launch, ((2, 0), (2, 1)), on_trust=True)
    assert state(desc) == ((2, 1), True, False) and launch.log == [(3, -1)] + [(2, 0)] * 4 + [(2, 1)] * 4
    assert conv.TUNED[sig_of('wgrad', desc)] == (2, 1, {(2, 0): 0.4, (2, 1): 0.3}) and conv.TUNE_BUDGET[0] == BUDGET - 1

    conv.TUNED.clear()
    conv.TUNED[neighbour] = (4, 0, {})
    desc = make_desc(T=380, dtype=torch.float32)
    launch = Launch(desc)
    conv._tune('wgrad', desc, launch, ((2, 0), (2, 1)), on_trust=True)
    assert state(desc) == ((4, 0), True, False) and launch.log == [(4, 0)]
    assert conv.TUNED == {neighbour: (4, 0, {})} and conv.TUNE_BUDGET[0] == BUDGET - 1      # (the budget: spent above)
    # the same neighbour next to a bf16 descriptor is taken
    conv.TUNED[sig_of('wgrad', make_desc(T=400))] = (4, 0, {})
    desc = make_desc(T=380)
    conv._tune('wgrad', desc, Launch(desc), ((2, 0),), on_trust=True)
    assert state(desc) == ((4, 0), True, True)


class WgradLibrary(object):
    """msmc_conv_wgrad_workspace / msmc_conv_wgrad_ws of a library that needs no workspace: records (variant, split_shift, dW
    pointer, db pointer) of every launch"""
    def __init__(self, desc, refuse=()):
        self.desc, self.refuse, self.log = desc, set(refuse), []

    def msmc_conv_wgrad_workspace(self, dref, g):
        return 0

    def msmc_conv_wgrad_ws(self, dref, g, dw, db, ws, nbytes, stream):
        c = (self.desc.variant, self.desc.split_shift)
        self.log.append(c + (dw, db))
        return 5 if c in self.refuse else 0


def run_wgrad(monkeypatch, desc, refuse=(), with_db=True):
    L = WgradLibrary(desc, refuse)
    monkeypatch.setattr(lib, '_lib', L)
    dw = Accepted(torch.zeros(2 * 3 * 96 * 64))
    db = Accepted(torch.zeros(2 * 96)) if with_db else None
    seen = set()
    conv._wgrad(desc, 4096, dw, db, ctypes.c_void_p(0), 'msmc_conv_wgrad', seen)
    return L, dw, db, seen


@pytest.mark.parametrize('with_db', [True, False])
def test_weight_gradient_timing_launches_accumulate_into_scratch_only(with_db, monkeypatch):
    desc = make_desc()
    monkeypatch.setattr(conv, '_WGRAD_CANDIDATES', ((4, 0), (2, 0), (2, 1)))
    scripted_times(monkeypatch, desc, {(4, 0): 0.3, (2, 1): 0.2})
    L, dw, db, seen = run_wgrad(monkeypatch, desc, refuse=[(2, 0)], with_db=with_db)
    assert [c[:2] for c in L.log] == [(4, 0)] * 4 + [(2, 0)] + [(2, 1)] * 4 + [(2, 1)]
    timing, real = L.log[:-1], L.log[-1]
    assert real[2:] == (dw.data_ptr(), db.data_ptr() if with_db else None)
    assert len({c[2] for c in timing}) == 1 and timing[0][2] not in (None, 0, dw.data_ptr())
    assert all((c[3] is None) == (not with_db) and (not with_db or c[3] != db.data_ptr()) for c in timing)
    assert float(dw.t.abs().sum()) == 0.0
    assert state(desc) == ((2, 1), True, False) and seen == {2}
    assert conv.TUNED == {sig_of('wgrad', desc): (2, 1, {(4, 0): 0.3, (2, 1): 0.2})} and conv.TUNE_BUDGET[0] == BUDGET - 1


def test_weight_gradient_resets_a_borrowed_choice_its_real_launch_refuses(monkeypatch):
    conv.TUNED[sig_of('wgrad', make_desc(T=400))] = (9, -1, {})
    before = dict(conv.TUNED)
    desc = make_desc(T=380)
    L, dw, db, seen = run_wgrad(monkeypatch, desc, refuse=[(9, -1)])
    assert L.log == [(9, -1, dw.data_ptr(), db.data_ptr()), (0, 0, dw.data_ptr(), db.data_ptr())]
    assert state(desc) == ((0, 0), True, False) and seen == {0}
    assert conv.TUNED == before and conv.TUNE_BUDGET[0] == BUDGET
    # a second refusal is the caller's error, and so is the refusal of a choice that was not borrowed
    desc = make_desc(T=380)
    with pytest.raises(RuntimeError, match='msmc_conv_wgrad failed with code 5'):
        run_wgrad(monkeypatch, desc, refuse=[(9, -1), (0, 0)])
    desc = make_desc(T=400)
    with pytest.raises(RuntimeError, match='variant 9 split_shift -1'):
        L = run_wgrad(monkeypatch, desc, refuse=[(9, -1)])
    assert state(desc) == ((9, -1), True, False)


def members(*variants):
    snaps = []
    for i, v in enumerate(variants):
        snaps.append(lib.ConvDesc.from_buffer_copy(make_desc(T=100 * (i + 1), built=(v, 0))))
    return snaps


def test_group_choice_without_timing():
    calls = []
    fn = lambda: calls.append(1)
    assert conv._group_choice('gather-group', members(2), fn, fn) == (0, 0)


def test_group_choice_while_capturing_groups_without_a_launch(monkeypatch):
    monkeypatch.setattr(conv, '_capturing', lambda: True)
    calls = []
    fn = lambda: calls.append(1)
    assert conv._group_choice('wgrad-group', members(4, 4), fn, fn, fn) == (1, 0)
    assert calls == [] and conv.TUNED == {}


@pytest.mark.parametrize('ms,want', [((0.1, 0.2, 0.3), (1, 0)), ((0.2, 0.1, 0.3), (0, 0)), ((0.3, 0.2, 0.1), (2, 0))])
def test_group_choice_returns_the_code_of_the_fastest_way(ms, want, monkeypatch):
    names = ('group', 'single', 'group4')
    calls = []
    fns = [lambda name=name: calls.append(name) for name in names]
    script = dict(zip(fns, ms))
    monkeypatch.setattr(conv, '_time_ms', lambda fn: script[fn])
    snaps = members(4, 4, 2)
    assert conv._group_choice('wgrad-group', snaps, *fns) == want
    assert calls == list(names)                                    # one validating call each, in this order
    sig = ('wgrad-group',) + tuple(conv._signature(d) + (d.variant, d.split_shift) for d in snaps)
    assert conv.TUNED == {sig: want + ({(n, 0): t for n, t in zip(names, ms)},)}
    assert conv.TUNE_BUDGET[0] == BUDGET                           # (grouping decisions are outside the budget)
    calls[:] = []
    assert conv._group_choice('wgrad-group', snaps, *fns) == want and calls == []       # decided: no launch any more


def test_group_choice_offers_uniform_variants_only_where_the_members_differ(monkeypatch):
    grouped, single = (lambda: None), (lambda: None)
    forced = {5: (lambda: None), 9: (lambda: None)}                # the variants every member accepts
    asked = []

    def uniform(v):
        asked.append(v)
        return forced.get(v)
    script = {grouped: 0.3, single: 0.2, forced[5]: 0.15, forced[9]: 0.05}
    monkeypatch.setattr(conv, '_time_ms', lambda fn: script[fn])
    assert conv._group_choice('gather-group', members(2, 19), grouped, single, uniform_fn=uniform) == (3, 9)
    assert asked == list(conv._UNIFORM_CANDIDATES)
    (times,) = [v[2] for v in conv.TUNED.values()]
    assert times == {('group', 0): 0.3, ('single', 0): 0.2, ('uniform', 5): 0.15, ('uniform', 9): 0.05}
    asked[:] = []
    assert conv._group_choice('gather-group', members(19, 19), grouped, single, uniform_fn=uniform) == (0, 0)
    assert asked == []


def test_shipped_decisions_survive_load_and_save(tmp_path):
    shipped_path = os.path.join(os.path.dirname(os.path.abspath(conv.__file__)), 'tuned_gfx950.json')
    with open(shipped_path) as f:
        shipped = json.load(f)['choices']
    conv.load_tuned(shipped_path)
    assert len(conv.TUNED) == len(shipped) > 1000
    copy = str(tmp_path / 'tuned.json')
    conv.save_tuned(copy)
    with open(copy) as f:
        assert json.load(f)['choices'] == shipped                  # the same rows in the same order
    first = dict(conv.TUNED)
    conv.TUNED.clear()
    conv.load_tuned(copy)
    assert conv.TUNED == first


@pytest.mark.parametrize('host', ['w', 'bias'])
def test_forward_refuses_a_host_weight_or_bias_before_any_library_call(host):
    geom = conv.Geometry(1, 50, (1, 3), padding=(0, 1))
    x = Accepted(torch.zeros(2, 1, 50, 8))
    w, bias = torch.zeros(3, 16, 8), torch.zeros(16)
    w, bias = (w, Accepted(bias)) if host == 'w' else (Accepted(w), bias)
    with pytest.raises(RuntimeError, match='GPU only'):
        conv.conv_forward(x, w, geom, bias=bias)
