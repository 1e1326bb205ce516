"""Exact branch-and-bound on the GPU: mi355x_simplex_solver(p, exact=True, branch_and_bound=True) against
the oracle search on Fractions (tests/bb_oracle.py over oracle/rational_ref.py), identically for every
width; the light read-back against the full download."""
import ctypes
import importlib
from fractions import Fraction

import numpy as np
import pytest

from oracle import rational_ref
from tests import bb_oracle as B
from tests import exact_bb_cases as X
from tests.exact_cases import to_dict
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
xbb = importlib.import_module("linear-programming_amd.exact_bb")
CASES = B.load_cases()
WIDTHS = (1, 4, 32)
_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _check(p, oracle_result, width):
    status, best, trace = oracle_result
    bb = xbb.ExactBranchAndBound(p, width=width)
    if status == B.INFEASIBLE:
        with pytest.raises(lp.InfeasibleProblemError):
            bb.run()
    elif status == B.UNBOUNDED:
        with pytest.raises(lp.UnboundedProblemError):
            bb.run()
    else:
        t = bb.run()
        assert isinstance(t, lp.ExactTableau) and lp.solution_problem(t) is p
        assert lp.solution_objective_value(t) == best[0]
        for v in p.vars:
            assert lp.solution_variable(t, v) == best[1][v], v
        # the reduced costs: the oracle's solved tableau of the incumbent's own node
        inc = max(k for k, r in enumerate(trace) if r[4] == B.BB_INCUMBENT)
        entry, k = [], inc
        while trace[k][0] >= 0:
            entry.append((trace[k][1], trace[k][2], Fraction(trace[k][3])))
            k = trace[k][0]
        ref = rational_ref.solve_any(rational_ref.build_tableau(to_dict(B.node_problem(p, tuple(entry), Fraction(1)))))
        for v in p.vars:
            if t.var_mapping[v][0] == "positive":
                assert lp.solution_reduced_cost(t, v) == rational_ref.tableau_reduced_cost(ref, v), v
    assert B.trace_key(bb.trace()) == B.trace_key(trace)
    # the objectives as Fractions: each row's against the oracle's node solver on the row's own entry
    entries = []
    for (parent, var, sense, bound, _, _), obj in zip(bb.trace(), bb.result.objectives):
        entries.append(() if parent < 0 else ((var, sense, Fraction(bound)),) + entries[parent])
        st, res = B.solve_node_exact(B.node_problem(p, entries[-1], Fraction(1)))
        assert obj == (res[0] if res else None) and (obj is None or type(obj) is Fraction)
    assert bb.stats()["declined"] == 0
    return bb


@pytest.mark.parametrize("width", WIDTHS)
def test_reference_integer_cases(width):
    for name in sorted(CASES):
        p = B.problem_of(CASES[name]["problem"], exact=True)
        _check(p, B.branch_and_bound(p, exact=True), width)


@pytest.mark.parametrize("width", WIDTHS)
def test_random_rational_programs(width):
    for seed, p, res in X.random_cases():
        _check(p, res, width)


def test_a_program_without_constraints():
    p = X.bounds_only_base()
    _check(p, B.branch_and_bound(p, exact=True), 4)


def test_through_the_solver_hook_and_the_node_cap():
    name = "rock_of_gibraltar_max"
    p = B.problem_of(CASES[name]["problem"], exact=True)
    t = lp.solve_problem(p, exact=True, branch_and_bound=True, bb_width=4)
    assert isinstance(t, lp.ExactTableau) and lp.solution_problem(t) is p
    for v, x in CASES[name]["expected"]["variables"].items():
        assert lp.solution_variable(t, v) == Fraction(x)
    with pytest.raises(lp.SolverError, match="node cap"):
        lp.solve_problem(p, exact=True, branch_and_bound=True, bb_width=4, max_nodes=2)


def test_a_node_that_starts_at_64_bits_and_finishes_at_128():
    p = X.wide_ilp()          # (the width model: every node needs more than 64 and at most 128 bits or stays small)
    res = B.branch_and_bound(p, exact=True, max_nodes=200)
    assert len(res[2]) == 9
    seen = []
    orig = xbb.readback

    def spy(xb):
        b = ctypes.c_int(0)
        for q in range(xb.n_lps):
            lp.capi.check(lp.capi.lib().mi355x_xbatch_bits(xb.handle, q, ctypes.byref(b)), "bits")
            seen.append(b.value)
        return orig(xb)
    xbb.readback = spy
    try:
        _check(p, res, 4)
    finally:
        xbb.readback = orig
    assert 128 in seen


def test_readback_is_the_download_of_the_solved_batch():
    p, nodes = X.assembly_case("tall_d1")                  # 300 rows: more than one trip
    g = xbb.GeneralForm(p)
    main, art = xbb.Base(g).create_nodes(nodes)
    assert art is None and main.rows > 256
    st, _ = lp.exact.batch_in_chunks(main, None, p.type == "max")
    light = xbb.readback(main)
    to_int = lp.exact._int128
    for q in range(main.n_lps):
        R, C = main.rows, main.cols
        T = np.empty(R * C * 2, dtype=np.int64)
        D = np.empty(2, dtype=np.int64)
        b = np.empty(R - 1, dtype=np.int64)
        lp.capi.check(lp.capi.lib().mi355x_xbatch_download(main.handle, q, _ptr(T), _ptr(D), _ptr(b)), "download")
        full = np.array([to_int(lo, hi) for lo, hi in T.reshape(-1, 2).tolist()], dtype=object).reshape(R, C)
        d, rhs, obj, basis = light[q]
        assert d == to_int(D[0], D[1]) and rhs == list(full[:, -1]) and obj == list(full[-1]) and basis.tolist() == b.tolist()
    assert (st == lp.capi.MI_OPTIMAL).any()
