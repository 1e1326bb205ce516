"""Branch-and-bound on the GPU (mi355x_simplex_solver_bb_*, solve_problem(p, branch_and_bound=True)):
the search, its trace, the incumbent and every value are those of the oracle search of
tests/bb_oracle.py (src/simplex.lisp:462-542 restated; node LPs by the C oracle) bit for bit, for
every width of speculative node batches and with two logical devices."""
import threading

import numpy as np
import pytest

from tests import bb_oracle as B
from tests.helpers import lp_amd

lp = lp_amd()
pytestmark = pytest.mark.gpu
CASES = B.load_cases()
RANDOM = B.random_cases(count=40)


def _run(problem, width, devices=1, int_tolerance=0):
    bb = lp.native.BranchAndBound(problem, width=width, devices=devices, int_tolerance=int_tolerance)
    rc = bb.run()
    trace, stats = bb.trace(), bb.stats()
    best = None
    if rc == lp.capi.MI_OPTIMAL:
        s = bb.finish()
        best = (s.objective_value(), {v: s.variable(v) for v in problem.vars})
    return rc, best, trace, stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_integer_cases(name):
    case = CASES[name]
    p = B.problem_of(case["problem"])
    st, best, _ = B.branch_and_bound(p)
    exp = case["expected"]
    if exp["status"] == "infeasible":
        with pytest.raises(lp.InfeasibleProblemError):
            lp.solve_problem(p, branch_and_bound=True)
        return
    sol = lp.solve_problem(p, branch_and_bound=True)
    assert lp.solution_problem(sol) is p
    assert sol.objective_value() == best[0]                           # the oracle, bit for bit
    for v in p.vars:
        assert sol.variable(v) == best[1][v], v
    for v, x in exp["variables"].items():                             # the reference's answers
        assert sol.variable(v) == pytest.approx(float(x), rel=1e-9, abs=1e-12)
    if "objective" in exp:
        assert sol.objective_value() == float(exp["objective"])       # dyadic: exact
    for v, x in exp.get("reduced_costs", {}).items():
        assert sol.reduced_cost(v) == float(x)
    # the default is unchanged
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problem(p)


@pytest.mark.parametrize("width,devices", [(1, 1), (3, 1), (64, 1), (64, 2)])
def test_random_programs_match_the_oracle_search_bit_for_bit(width, devices):
    for seed, p, (st, best, trace) in RANDOM:
        if width == 1 and seed % 2:
            continue                     # (width 1 is the slowest: every second program)
        rc, got, gtrace, stats = _run(p, width, devices)
        assert rc == st, seed
        assert B.trace_key(gtrace) == B.trace_key(trace), seed
        assert stats["processed"] == len(trace) and stats["solved"] >= len(trace)
        if best is None:
            assert got is None
            continue
        assert got[0] == best[0], seed
        assert got[1] == best[1], seed


def test_unbounded_relaxation_and_no_integral_point():
    unb = lp.Problem(type="max", vars=["x", "y"], objective_func=[("x", 1.0)], integer_vars=["x"],
                     constraints=[("<=", [("y", 1.0)], 1.0)])
    with pytest.raises(lp.UnboundedProblemError):
        lp.solve_problem(unb, branch_and_bound=True)
    none = lp.Problem(type="max", vars=["x"], objective_func=[("x", 1.0)], integer_vars=["x"],
                      constraints=[(">=", [("x", 1.0)], 0.2), ("<=", [("x", 1.0)], 0.8)])
    assert B.branch_and_bound(none)[0] == B.INFEASIBLE
    with pytest.raises(lp.InfeasibleProblemError):
        lp.solve_problem(none, branch_and_bound=True, bb_width=2)


def test_max_nodes_chunks_resume_to_the_same_trace_and_cancel():
    seed, p, (st, best, trace) = max(RANDOM, key=lambda r: len(r[2][2]))
    assert len(trace) >= 10
    bb = lp.native.BranchAndBound(p, width=8)
    bb.cancel()                                       # sticky: the next step stops at once
    assert bb.step(0) == (lp.capi.MI_CANCELLED, 0)
    steps = []
    while True:
        rc, k = bb.step(3)
        steps.append(k)
        if rc != lp.capi.MI_MAX_PIVOTS:
            break
    assert rc == st and all(k <= 3 for k in steps) and sum(steps) == len(trace)
    assert B.trace_key(bb.trace()) == B.trace_key(trace)
    with pytest.raises(lp.SolverError):
        lp.solve_problem(p, branch_and_bound=True, max_nodes=2)
    # a cancel from another thread stops a search that is running
    knap = _knapsack()
    bb = lp.native.BranchAndBound(knap, width=1)
    started, seen = threading.Event(), []

    def search():
        seen.append(bb.step(1))                       # the first node is in
        started.set()
        seen.append(bb.run(chunk=1 << 20))            # a search that would not end by itself
    t = threading.Thread(target=search)
    t.start()
    assert started.wait(120)
    bb.cancel()
    t.join(120)
    assert not t.is_alive()
    assert seen[0] == (lp.capi.MI_MAX_PIVOTS, 1) and seen[1] == lp.capi.MI_CANCELLED
    done = bb.stats()["processed"]
    assert bb.run(max_nodes=3) == lp.capi.MI_MAX_PIVOTS            # it carries on where it stopped
    fresh = lp.native.BranchAndBound(knap, width=1)
    fresh.run(max_nodes=done + 3)
    assert B.trace_key(bb.trace()) == B.trace_key(fresh.trace())


def _knapsack(n=24, m=8, seed=3):
    """A 0-1 knapsack whose exact-integrality search dives for a long time (values a few ulps off an
    integer are branched on, as the reference would)."""
    rng = np.random.default_rng(seed)
    names = ["x%d" % i for i in range(n)]
    w = rng.integers(5, 60, size=(m, n)).astype(float)
    v = rng.integers(10, 100, size=n).astype(float)
    return lp.Problem(type="max", vars=names, objective_func=list(zip(names, v.tolist())), integer_vars=names,
                      var_bounds=[(x, (0.0, 1.0)) for x in names],
                      constraints=[("<=", list(zip(names, w[r].tolist())), float(np.floor(w[r].sum() / 2)) + 0.5)
                                   for r in range(m)])


def test_int_tolerance_matches_the_oracle_at_the_same_tolerance():
    p = lp.Problem(type="max", vars=["x", "y"], objective_func=[("x", 1.0), ("y", 0.0)], integer_vars=["x"],
                   constraints=[("<=", [("x", 0.1)], 0.3), ("<=", [("y", 1.0)], 1.0)])
    for tol in (0, 1024):
        st, best, trace = B.branch_and_bound(p, int_tolerance=tol)
        rc, got, gtrace, _ = _run(p, 4, int_tolerance=tol)
        assert rc == st and B.trace_key(gtrace) == B.trace_key(trace)
        assert (got is None) == (best is None) and (got is None or got == best)
    sol = lp.solve_problem(p, branch_and_bound=True, int_tolerance=1024)
    assert sol.variable("x") == 0.3 / 0.1
