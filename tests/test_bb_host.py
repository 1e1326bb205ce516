"""Branch-and-bound without a GPU: the oracle search (tests/bb_oracle.py, a literal restatement of
src/simplex.lisp:462-542) reproduces the reference's integer answers (tests/golden/
reference_ilp_cases.json) on the double-float path and on exact rationals, and the library's
branch-and-bound entry points validate their arguments and refuse to run without a device."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import bb_oracle as B
from tests.helpers import lp_amd

lp = lp_amd()
CASES = B.load_cases()


def _expected_ok(name, status, best):
    exp = CASES[name]["expected"]
    if exp["status"] == "infeasible":
        assert status == B.INFEASIBLE and best is None
        return
    assert status == B.OPTIMAL
    obj, vals = best
    if "objective" in exp:
        assert obj == Fraction(exp["objective"])
    for v, x in exp["variables"].items():
        assert vals[v] == Fraction(x), (name, v, vals[v])


@pytest.mark.parametrize("name", sorted(CASES))
def test_f64_oracle_reproduces_the_reference_answers(name):
    status, best, trace = B.branch_and_bound(B.problem_of(CASES[name]["problem"]))
    _expected_ok(name, status, best)
    assert trace[0][0] == -1 and trace[0][1] is None                 # the root entry ()


@pytest.mark.parametrize("name", sorted(CASES))
def test_rational_oracle_through_the_same_search_gives_the_same_answers(name):
    status, best, trace = B.branch_and_bound(B.problem_of(CASES[name]["problem"], exact=True), exact=True)
    _expected_ok(name, status, best)
    f_status, f_best, f_trace = B.branch_and_bound(B.problem_of(CASES[name]["problem"]))
    assert status == f_status and len(trace) == len(f_trace)
    assert [r[:3] + (r[4],) for r in trace] == [r[:3] + (r[4],) for r in f_trace]


def test_rock_of_gibraltar_reduced_costs_are_zero():
    """t/solver.lisp:50-55: solution-reduced-cost of x and y is 0 in the incumbent."""
    p = B.problem_of(CASES["rock_of_gibraltar_max"]["problem"])
    status, best, trace = B.branch_and_bound(p)
    assert status == B.OPTIMAL and best[1] == {"x": 3.0, "y": 1.0}
    assert [r[4] for r in trace].count(B.BB_INCUMBENT) >= 1


def test_random_cases_are_deterministic_and_search_trees():
    cases = B.random_cases(count=12)
    again = B.random_cases(count=12)
    assert [s for s, _, _ in cases] == [s for s, _, _ in again]
    assert [B.trace_key(r[2]) for _, _, r in cases] == [B.trace_key(r[2]) for _, _, r in again]
    assert any(len(r[2]) >= 5 for _, _, r in cases)


def test_int_tolerance_changes_only_what_counts_as_integral():
    p = lp.Problem(type="max", vars=["x", "y"], objective_func=[("x", 1.0), ("y", 0.0)], integer_vars=["x"],
                   constraints=[("<=", [("x", 0.1)], 0.3), ("<=", [("y", 1.0)], 1.0)])
    st0, _, tr0 = B.branch_and_bound(p)
    st1, best1, tr1 = B.branch_and_bound(p, int_tolerance=1024)
    assert tr0[0][4] == B.BB_BRANCHED and tr0[0][5] == tr1[0][5] == 0.1 * 0 + 0.3 / 0.1
    assert st1 == B.OPTIMAL and tr1 == [(-1, None, 0, 0.0, B.BB_INCUMBENT, 0.3 / 0.1)]
    assert best1[1]["x"] == 0.3 / 0.1                                   # the raw tableau value is reported


def _begin(L, prob, order=(0,), f=1024.0, tol=0.0, width=4, n_dev=1, ids=None):
    arr = np.asarray(order, dtype=np.int64)
    h = ctypes.c_void_p()
    rc = L.mi355x_simplex_solver_bb_begin(prob, arr.ctypes.data_as(ctypes.c_void_p) if len(arr) else None,
                                          len(arr), f, tol, width, n_dev, ids, ctypes.byref(h))
    return rc, h


def test_bb_entry_points_validate_their_arguments():
    L = lp.capi.lib()
    np_ = lp.native.NativeProblem(B.problem_of(CASES["rock_of_gibraltar_max"]["problem"]))
    BAD = lp.capi.MI_BAD_ARG
    assert _begin(L, None)[0] == BAD
    assert _begin(L, np_._h, order=(2,))[0] == BAD                     # only x, y exist
    assert _begin(L, np_._h, order=(-1,))[0] == BAD
    assert _begin(L, np_._h, width=0)[0] == BAD
    assert _begin(L, np_._h, n_dev=0)[0] == BAD
    assert _begin(L, np_._h, f=-1.0)[0] == BAD
    assert _begin(L, np_._h, tol=-1.0)[0] == BAD
    assert _begin(L, np_._h, tol=float("nan"))[0] == BAD
    assert _begin(L, np_._h, tol=float("inf"))[0] == BAD
    assert L.mi355x_simplex_solver_bb_begin(np_._h, None, 1, 1024.0, 0.0, 4, 1, None, None) == BAD
    n = ctypes.c_int64(7)
    assert L.mi355x_simplex_solver_bb_step(None, 0, ctypes.byref(n)) == BAD and n.value == 0
    assert L.mi355x_simplex_solver_bb_cancel(None) == BAD
    s = ctypes.c_void_p()
    assert L.mi355x_simplex_solver_bb_finish(None, ctypes.byref(s)) == BAD and not s.value
    assert L.mi355x_simplex_solver_bb_stats(None, None, None, None) == BAD
    assert L.mi355x_simplex_solver_bb_trace(None, None, None, None, None, None, None, 0, None) == BAD
    L.mi355x_simplex_solver_bb_abandon(None)                          # no-op


@pytest.mark.skipif(lp.capi.device_count() > 0, reason="a GPU is present")
def test_bb_without_a_device_is_a_loud_failure():
    L = lp.capi.lib()
    prob = B.problem_of(CASES["rock_of_gibraltar_max"]["problem"])
    np_ = lp.native.NativeProblem(prob)
    rc, h = _begin(L, np_._h, order=(0, 1))
    assert rc == lp.capi.MI_NO_DEVICE and not h.value
    with pytest.raises(lp.capi.Mi355xError):
        lp.solve_problem(prob, branch_and_bound=True)
    # the default is unchanged: integer problems are declined
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problem(prob)
