"""Exact mode on the GPU (solve_problem(p, exact=True)): fraction-free integer tableaux
(kernels_exact.inc) against the Fraction oracle (oracle/rational_ref.py) -- status, pivot sequence,
basis and every final entry -- plus the width escalation (also inside a two-phase job and under bounded
calls), the 128-bit limit, bounded calls, cancel, the trace buffer's cap and handle cycles.

MI_EXACT_INEXACT is not tested here: no input reaches it through the public entry points.  A solve is
refused (MI_UNSUPPORTED) unless the basis columns are exact unit columns, and from such a start every
fraction-free division is exact (D0 is the product of the rows' denominator LCMs, so every 2 x 2 minor of
D0 * t0 is a multiple of D0; Sylvester's identity carries that on); the main tableau of a two-phase job
is rebuilt from the artificial one.  The kXInexact / kXOverflow split of a failed division is pinned on
the arithmetic itself, in tests/test_gpu_exact_arith.py (xdiv with planted remainders)."""
import ctypes
import json
import os
import threading
import time
from fractions import Fraction

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests import goldens
from tests.helpers import ROOT, lp_amd

lp = lp_amd()
pytestmark = pytest.mark.gpu
SEEDS = range(200)

_ERRORS = {"unbounded": lp.UnboundedProblemError, "infeasible": lp.InfeasibleProblemError,
           "art_nonzero": lp.SolverError, "art_stuck": lp.SolverError}


def _trace(sol):
    tr = [] if sol.phase1 is None else [tuple(x) for x in sol.phase1.pivot_trace().tolist()]
    return tr + [tuple(x) for x in sol.pivot_trace().tolist()]


def _check_against_oracle(p, **kw):
    """Solve p exactly on the GPU, compare with the oracle; returns (status, solution or None)."""
    tabs = rr.build_tableau(ec.to_dict(p))
    st, trace, t = ec.oracle_outcome(tabs)
    if st != "optimal":
        with pytest.raises(_ERRORS[st]):
            lp.solve_problem(p, exact=True, **kw)
        return st, None
    sol = lp.solve_problem(p, exact=True, **kw)
    assert isinstance(sol, lp.ExactTableau)
    assert _trace(sol) == trace
    assert sol.basis_columns.tolist() == t.basis
    assert sol.matrix.tolist() == t.matrix
    return st, sol


def test_golden_cases_exactly(golden):
    for name, case in golden["cases"].items():
        if case.get("float32_literals"):
            continue
        p = lp.Problem.from_dict(goldens.problem(case))
        st, sol = _check_against_oracle(p)
        if sol is None:
            assert case.get("error") in (None, st), name
            continue
        ov = lp.solution_objective_value(sol)
        assert isinstance(ov, Fraction)
        if "objective" in case:
            assert ov == goldens.frac(case["objective"]), name
        for v, x in case.get("variables", {}).items():
            got = lp.solution_variable(sol, v)
            assert isinstance(got, Fraction) and got == goldens.frac(x), (name, v)
        for v, x in case.get("reduced_costs", {}).items():
            got = lp.solution_reduced_cost(sol, v)
            assert isinstance(got, Fraction) and got == goldens.frac(x), (name, v)
        for v, (lo, hi) in case.get("variable_ranges", {}).items():
            assert lo <= lp.solution_variable(sol, v) <= hi
        for v in case.get("reduced_cost_errors", []):
            with pytest.raises((KeyError, ValueError)):
                lp.solution_reduced_cost(sol, v)
        for v in case.get("variable_errors", []):
            with pytest.raises(KeyError):
                lp.solution_variable(sol, v)


def _float32_problem(case):
    def num(x):
        return Fraction(x) if isinstance(x, str) else (float(np.float32(x)) if isinstance(x, float) else x)
    p = case["problem"]
    return lp.Problem(type=p["type"], vars=list(p["vars"]), objective_var=p.get("objective_var"),
                      objective_func=[(v, num(c)) for v, c in p["objective"]],
                      var_bounds=[(b[0], (None if b[1] is None else num(b[1]), None if b[2] is None else num(b[2])))
                                  for b in p["bounds"]],
                      constraints=[(op, [(v, num(c)) for v, c in e], num(r)) for op, e, r in p["constraints"]])


def test_float_cases_take_the_double_path_unchanged(golden):
    for name, case in golden["cases"].items():
        if not case.get("float32_literals"):
            continue
        p = _float32_problem(case)
        a, b = lp.solve_problem(p, exact=True), lp.solve_problem(p)
        assert type(a) is type(b) and not isinstance(a, lp.ExactTableau)
        names = [p.objective_var] + list(p.vars)
        assert [lp.solution_variable(a, v) for v in names] == [lp.solution_variable(b, v) for v in names]


def test_random_rational_problems_match_the_oracle():
    seen, widths = set(), set()
    for seed in SEEDS:
        p = ec.random_problem(lp, seed)
        tabs = rr.build_tableau(ec.to_dict(p))
        mst, _, _, stats = ec.model_solve(tabs)
        if stats["max_bits"] > 128:                        # outgrows the widest storage
            with pytest.raises(lp.UnsupportedConstraintError):
                lp.solve_problem(p, exact=True)
            seen.add("overflow")
            continue
        st, sol = _check_against_oracle(p)
        seen.add(st)
        if stats["driveouts"]:
            seen.add("driveout")
        if stats["negative_pivots"]:
            seen.add("negative")
        if sol is not None:
            bits = 64 if stats["max_bits"] <= 64 else 128
            assert sol.bits == bits and (sol.phase1 is None or sol.phase1.bits == bits), seed
            widths.add(bits)
    assert {"optimal", "unbounded", "infeasible", "driveout", "negative"} <= seen
    assert widths == {64, 128}


def test_width_128_from_the_start_gives_the_same_trace_and_values():
    for seed in SEEDS:
        p = ec.random_problem(lp, seed)
        try:
            a = lp.solve_problem(p, exact=True)
        except lp.SolverError:
            continue
        b = lp.solve_problem(p, exact=True, exact_bits=128)
        assert b.bits == 128
        assert _trace(a) == _trace(b)
        assert a.matrix.tolist() == b.matrix.tolist() and a.basis_columns.tolist() == b.basis_columns.tolist()


def test_exact_and_double_paths_disagree_where_rounding_breaks_ties():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "exact_divergent_cases.json")))["cases"]
    assert len(cases) >= 4
    for case in cases:
        p = lp.Problem.from_dict(goldens.problem(dict(case, problem=dict(case["problem"], bounds=[]))))
        exact_trace = [tuple(x) for x in case["exact_trace"]]
        assert exact_trace != [tuple(x) for x in case["double_trace"]]
        _, sol = _check_against_oracle(p)
        assert _trace(sol) == exact_trace
        dbl = lp.solve_problem(p, native=False)
        assert [tuple(x) for x in dbl.pivot_trace().tolist()] == [tuple(x) for x in case["double_trace"]]


def test_64_bit_overflow_escalates_to_128_bits():
    p = ec.wide_problem(lp, 0, 40)
    _, _, _, stats = ec.model_solve(rr.build_tableau(ec.to_dict(p)))
    assert 64 < stats["max_bits"] <= 128
    _, sol = _check_against_oracle(p)
    assert sol.bits == 128


def test_128_bit_overflow_is_declined():
    p = ec.wide_problem(lp, 2, 60)
    _, _, _, stats = ec.model_solve(rr.build_tableau(ec.to_dict(p)))
    assert stats["max_bits"] > 128
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problem(p, exact=True)
    t = lp.build_tableau(p, exact=True)
    n = ctypes.c_int64(0)
    assert lp.capi.lib().mi355x_xtab_solve(t._h, 1, 0, ctypes.byref(n)) == lp.capi.MI_EXACT_OVERFLOW


def test_bounded_calls_resume_to_the_one_call_trace():
    for seed in (1, 5, 11, 17, 40 + 1, 68, 120, 181):
        p = ec.random_problem(lp, seed)
        try:
            whole = lp.solve_problem(p, exact=True)
        except lp.SolverError:
            continue
        tabs = lp.build_tableau(p, exact=True)
        part = lp.exact.n_solve_exact(tabs, chunk=1)
        assert _trace(part) == _trace(whole)
        assert part.matrix.tolist() == whole.matrix.tolist()


def test_cancel_stops_a_cycling_exact_solve_and_leaves_the_tableau_whole():
    t = lp.build_tableau(ec.beale(lp), exact=True)
    n = ctypes.c_int64(0)
    L = lp.capi.lib()
    assert L.mi355x_xtab_solve(t._h, 1, 200, ctypes.byref(n)) == lp.capi.MI_MAX_PIVOTS and n.value == 200
    tr = t.pivot_trace()
    assert [tuple(x) for x in tr[:12].tolist()] == [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (5, 1)] * 2
    out = {}

    def run():
        out["rc"] = L.mi355x_xtab_solve(t._h, 1, 0, ctypes.byref(n))
    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.3)
    assert th.is_alive()
    lp.exact.cancel_solve(t)
    th.join(timeout=30)
    assert not th.is_alive() and out["rc"] == lp.capi.MI_CANCELLED and n.value > 0
    t._touch()
    k = len(t.pivot_trace())
    ref = rr.build_tableau(ec.to_dict(ec.beale(lp)))
    for _ in range(k % 6):                                  # the cycle's state after k pivots
        e = rr.price(ref)
        rr.pivot(ref, e, rr.ratio(ref, e))
    assert t.matrix.tolist() == ref.matrix and t.basis_columns.tolist() == ref.basis
    assert L.mi355x_xtab_solve(t._h, 1, 7, ctypes.byref(n)) == lp.capi.MI_MAX_PIVOTS and n.value == 7


def test_exact_handle_cycles_do_not_lose_device_memory():
    import torch
    p = ec.random_problem(lp, 68)

    def cycle():
        sol = lp.solve_problem(p, exact=True)
        sol.matrix
        del sol
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(100):
        cycle()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20


def _escalating_two_phase_problems():
    """By the model: a two-phase problem whose entries first outgrow 64 bits in phase 1, and one where that
    happens later (a drive-out, the hand-over or phase 2).  {where: (problem, trace, stats, n1)}"""
    found = {}
    for e in (24, 28):
        for seed in range(8):
            p = ec.wide_mixed_problem(lp, seed, e)
            tabs = rr.build_tableau(ec.to_dict(p))
            keep = {}
            st, trace, _, stats = ec.model_solve(tabs, keep=keep)
            if st != "optimal" or stats["over64"] is None or stats["max_bits"] > 128 or stats["inexact"]:
                continue
            where = "phase1" if stats["over64"][0] == "phase1" else "later"
            assert (stats["over64"][1] < keep["n1"]) == (where == "phase1")
            found.setdefault(where, (p, trace, stats, keep["n1"]))
    return found


@pytest.mark.parametrize("where", ["phase1", "later"])
def test_64_bit_overflow_inside_a_two_phase_job_restarts_both_phases(where):
    found = _escalating_two_phase_problems()
    assert where in found
    p, trace, stats, n1 = found[where]
    counts = (n1 + stats["driveouts"], len(trace) - n1)
    tabs = lp.build_tableau(p, exact=True)
    assert [t.bits for t in tabs] == [64, 64]                  # (the start fits: the overflow comes on the way)
    _, sol = _check_against_oracle(p)
    assert sol.bits == 128 and sol.phase1.bits == 128
    assert _trace(sol) == trace and tuple(sol.n_pivots) == counts
    # one pivot per call: the restart at 128 bits replays the pivots of the earlier calls, and counts none twice
    calls = []
    L = lp.capi.lib()
    art, main = tabs
    npv = (ctypes.c_int64 * 2)()
    while True:
        rc = L.mi355x_xtab_solve_two_phase(art._h, main._h, 1, 1, npv)
        calls.append((rc, npv[0], npv[1]))
        assert len(calls) <= sum(counts) + 2
        if rc != lp.capi.MI_MAX_PIVOTS:
            break
    assert rc == lp.capi.MI_OPTIMAL
    assert (sum(c[1] for c in calls), sum(c[2] for c in calls)) == counts
    assert all(c[1] + c[2] <= max(1, stats["driveouts"]) for c in calls)
    art._touch()
    main._touch()
    assert art.bits == 128 and main.bits == 128
    assert [tuple(x) for x in art.pivot_trace().tolist()] + [tuple(x) for x in main.pivot_trace().tolist()] == trace
    assert main.matrix.tolist() == sol.matrix.tolist() and main.basis_columns.tolist() == sol.basis_columns.tolist()
    # and through the package's own bounded calls
    part = lp.exact.n_solve_exact(lp.build_tableau(p, exact=True), chunk=1)
    assert part.bits == 128 and part.phase1.bits == 128
    assert _trace(part) == trace and tuple(part.n_pivots) == counts
    assert part.matrix.tolist() == sol.matrix.tolist()


def test_trace_buffer_stops_at_its_cap_while_the_count_goes_on():
    CAP = 1 << 18
    total = CAP + 60
    t = lp.build_tableau(ec.beale(lp), exact=True)
    L = lp.capi.lib()
    n = ctypes.c_int64(0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mi355x_xtab_solve(t._h, 1, total, ctypes.byref(n)) == lp.capi.MI_MAX_PIVOTS and n.value == total
    period = [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (5, 1)]
    want = np.array(period * (CAP // 6 + 1), dtype=np.int64)[:CAP]
    e, r = np.full(CAP + 1000, -7, dtype=np.int64), np.full(CAP + 1000, -7, dtype=np.int64)
    assert L.mi355x_xtab_trace(t._h, ptr(e), ptr(r), e.size, ctypes.byref(n)) == lp.capi.MI_OK
    assert n.value == total                                                  # the count goes on past the buffer
    assert (e[CAP:] == -7).all() and (r[CAP:] == -7).all()                   # exactly 2^18 entries are filled
    assert np.array_equal(e[:CAP], want[:, 0]) and np.array_equal(r[:CAP], want[:, 1])
    e, r = np.full(200, -7, dtype=np.int64), np.full(200, -7, dtype=np.int64)
    assert L.mi355x_xtab_trace(t._h, ptr(e), ptr(r), 100, ctypes.byref(n)) == lp.capi.MI_OK and n.value == total
    assert np.array_equal(e[:100], want[:100, 0]) and np.array_equal(r[:100], want[:100, 1])
    assert (e[100:] == -7).all() and (r[100:] == -7).all()
    t._touch()
    ref = rr.build_tableau(ec.to_dict(ec.beale(lp)))
    for _ in range(total % 6):                                               # the cycle's state after `total` pivots
        c = rr.price(ref)
        rr.pivot(ref, c, rr.ratio(ref, c))
    assert t.matrix.tolist() == ref.matrix and t.basis_columns.tolist() == ref.basis
