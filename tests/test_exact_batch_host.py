"""Host-side checks of the exact batches (mi355x_xbatch_*, mi355x_solve_problems(exact=True)) that need no
GPU: argument validation of the C entry points and the grouping of a problem list."""
import ctypes
import inspect

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_validation_without_a_device():
    L = capi.lib()
    st = np.zeros(4, dtype=np.int32)
    assert L.mi355x_xbatch_solve(None, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_solve_two_phase(None, None, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_download(None, 0, None, None, None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_trace(None, 0, None, None, 0, None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_bits(None, 0, None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_cancel(None) == capi.MI_BAD_ARG
    L.mi355x_xbatch_destroy(None)                                    # no-op
    num = np.ones((2, 3, 4), dtype=np.int64)
    den = np.ones((2, 3, 4), dtype=np.int64)
    basis = np.zeros((2, 2), dtype=np.int64)
    h = ctypes.c_void_p()
    create = L.mi355x_xbatch_create
    assert create(None, 2, 3, 4, _ptr(num), _ptr(den), _ptr(basis), 0, 0) == capi.MI_BAD_ARG
    assert create(ctypes.byref(h), 0, 3, 4, _ptr(num), _ptr(den), _ptr(basis), 0, 0) == capi.MI_BAD_ARG
    assert create(ctypes.byref(h), 2, 3, 4, None, _ptr(den), _ptr(basis), 0, 0) == capi.MI_BAD_ARG
    assert create(ctypes.byref(h), 2, 3, 4, _ptr(num), _ptr(den), None, 0, 0) == capi.MI_BAD_ARG
    assert create(ctypes.byref(h), 2, 3, 4, _ptr(num), _ptr(den), _ptr(basis), 0, 32) == capi.MI_BAD_ARG
    assert b"min_bits" in L.mi355x_last_error()
    for bad in (0, -3):
        den[1, 2, 3] = bad                                           # (in the second member)
        assert create(ctypes.byref(h), 2, 3, 4, _ptr(num), _ptr(den), _ptr(basis), 0, 0) == capi.MI_BAD_ARG
        assert b"denominator" in L.mi355x_last_error() and not h.value
    # a pair that cannot be one: the same handle twice (the checks that need two live handles run on the GPU)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    assert L.mi355x_xbatch_solve_two_phase(fake, fake, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_solve_two_phase(fake, None, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG


@pytest.mark.skipif(capi.device_count() > 0, reason="a GPU is present")
def test_create_without_a_device_fails_loudly():
    num = np.ones((2, 3, 4), dtype=np.int64)
    basis = np.zeros((2, 2), dtype=np.int64)
    h = ctypes.c_void_p()
    rc = capi.lib().mi355x_xbatch_create(ctypes.byref(h), 2, 3, 4, _ptr(num), _ptr(num), _ptr(basis), 0, 0)
    assert rc == capi.MI_NO_DEVICE and not h.value
    assert b"no HIP device" in capi.lib().mi355x_last_error()


def test_solve_problems_takes_the_exact_arguments():
    sig = inspect.signature(lp.simplex.mi355x_solve_problems)
    assert sig.parameters["exact"].default is False and sig.parameters["exact_bits"].default == 0


def test_grouping_of_a_problem_list():
    """The grouping of mi355x_solve_problems(exact=True) on random_problem seeds 0..199 against the shapes
    of the oracle's own build-tableau: 26 two-phase groups of two or more with 60 members, everything else
    one by one."""
    seeds = list(range(200))
    ps = [ec.random_problem(lp, s) for s in seeds]
    want, want1 = {}, {}
    for s, p in zip(seeds, ps):
        tabs = rr.build_tableau(ec.to_dict(p))
        if isinstance(tabs, tuple):
            key = tuple((len(t.matrix), len(t.matrix[0])) for t in tabs) + (tabs[1].is_max,)
            want.setdefault(key, []).append(s)
        else:
            want1.setdefault(((len(tabs.matrix), len(tabs.matrix[0])), tabs.is_max), []).append(s)
    lone = sorted(v[0] for g in (want, want1) for v in g.values() if len(v) == 1)
    want = {k: v for k, v in want.items() if len(v) >= 2}
    want1 = {k: v for k, v in want1.items() if len(v) >= 2}
    alone, groups, groups2, failed = lp.exact.group_exact_problems(ps)
    assert not failed and alone == lone
    assert {k: [m[0] for m in v] for k, v in groups.items()} == want1
    assert {k: [m[0] for m in v] for k, v in groups2.items()} == want
    assert len(groups2) == 26 and sum(len(v) for v in groups2.values()) == 60
    for members in groups2.values():
        for k, art, main in members:
            assert art.exact and main.exact and art._handle is None and main._handle is None   # (nothing touched a device)
    # integer members, members with a float and members alone in their group go one by one
    extra = ec.mixed_problem(lp, 6, 3, 2, 1, 0)
    flt = lp.Problem(type=extra.type, vars=list(extra.vars), objective_var="w",
                     objective_func=[(v, float(c)) for v, c in extra.objective_func], constraints=list(extra.constraints))
    integer = lp.Problem(type=extra.type, vars=list(extra.vars), objective_var="w", objective_func=list(extra.objective_func),
                         constraints=list(extra.constraints), integer_vars=["x0"])
    twin = ec.mixed_problem(lp, 6, 3, 2, 1, 1)
    alone, groups, groups2, failed = lp.exact.group_exact_problems([extra, flt, integer, twin, ec.beale(lp)])
    assert alone == [1, 2, 4] and not groups and not failed
    assert [[m[0] for m in v] for v in groups2.values()] == [[0, 3]]
    assert list(groups2) == [((11, 19), (11, 14), True)]
