"""The pivot rules of the exact solves on the GPU (mi355x_xtab_set_pivot_rule / mi355x_xbatch_set_pivot_rule,
`pivot_rule=` in Python) against their restatement in tests/pivot_rule_cases.py: status, pivot trace and final
state (D, every entry, the basis) of single tableaux at every width, of batch members, of two-phase pairs
(the flag cleared at the hand-over), across calls (the flag kept between launches), across the restart at a
wider width (the flag cleared with the start state), through exact branch-and-bound and through the public
functions.  Every solve carries a finite cap: with a wrong rule the textbook LPs cycle for ever."""
import ctypes
import dataclasses
import functools
import importlib
from fractions import Fraction

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import bb_oracle as B
from tests import exact_cases as ec
from tests import pivot_rule_cases as pc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
xbb = importlib.import_module("linear-programming_amd.exact_bb")
CODES = {"optimal": capi.MI_OPTIMAL, "unbounded": capi.MI_UNBOUNDED, "infeasible": capi.MI_INFEASIBLE,
         "art_nonzero": capi.MI_ART_NONZERO, "art_stuck": capi.MI_ART_STUCK, "max_pivots": capi.MI_MAX_PIVOTS}
SMALL_CAP, SLACK_CAP = 200, 3000


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pairs(a):
    return [tuple(x) for x in a.tolist()]


def _ints(T):
    return [[int(x) for x in row] for row in (T.tolist() if isinstance(T, np.ndarray) else T)]


def _same_state(t, model):
    """An ExactTableau's device state against a model's: D, the basis, every entry."""
    T, D, basis = t.raw()
    assert D == model.D and basis.tolist() == [int(b) for b in model.basis]
    assert _ints(T) == _ints(model.T)


def _solve(t, cap):
    """mi355x_xtab_solve on an ExactTableau with a cap: (status, pivots of the call)."""
    n = ctypes.c_int64(-1)
    rc = capi.lib().mi355x_xtab_solve(t._h, int(t.is_max), cap, ctypes.byref(n))
    t._touch()
    return rc, n.value


def _int_tableau(T, basis, rule, min_bits=0, max_bits=128):
    """An ExactTableau on an integer start state (a max problem, every denominator 1)."""
    R, C = T.shape
    return lp.ExactTableau(None, lp.Problem(type="max"), [[Fraction(int(x)) for x in row] for row in T], basis, C - 1,
                           R - 1, {}, min_bits=min_bits, max_bits=max_bits, pivot_rule=rule)


# ---- 1. the textbook cycling LPs, single tableaux, every rule at every width ---------------------------------
@functools.lru_cache(maxsize=None)
def _cycling_model(name, rule):
    tabs = rr.build_tableau(ec.to_dict(pc.CYCLING[name][0](lp)))
    return pc.solve_tabs(tabs, rule, 60 if rule == "dantzig" else SMALL_CAP)


@pytest.mark.parametrize("bits", [64, 128, 256])
@pytest.mark.parametrize("rule", pc.RULES)
@pytest.mark.parametrize("name", sorted(pc.CYCLING))
def test_cycling_lps_as_single_tableaux(name, rule, bits):
    st, trace, model, stats = _cycling_model(name, rule)
    assert stats["max_bits"] <= 64 and not stats["inexact"]
    if rule == "dantzig":
        assert st == "max_pivots" and trace == pc.PERIOD * 10
    else:
        assert st == "optimal" and trace == pc.CYCLING[name][1]
    t = lp.build_tableau(pc.CYCLING[name][0](lp), exact=True, min_bits=bits, max_bits=256 if bits == 256 else 128)
    t.set_pivot_rule(rule)
    rc, n = _solve(t, 60 if rule == "dantzig" else SMALL_CAP)
    assert (rc, n) == (CODES[st], len(trace)), capi.lib().mi355x_last_error()
    assert _pairs(t.pivot_trace()) == trace and t.bits == bits
    _same_state(t, model)
    if st == "optimal":
        assert lp.solution_objective_value(t) == pc.CYCLING[name][2]


# ---- 2. / 3. more columns and more rows than the workgroup has threads ---------------------------------------
@functools.lru_cache(maxsize=None)
def _slack_model(shape, seed, rule):
    kw = dict(pc.WIDE_SLACK if shape == "wide" else pc.TALL_SLACK, seed=seed)
    T, b = pc.slack(**kw)
    st, trace, m = pc.solve_state(T, b, rule, SLACK_CAP)
    assert st == "optimal" and not m.stats["inexact"] and m.stats["max_bits"] <= 64
    return T, b, trace, m


@pytest.mark.parametrize("rule", ["bland", "dantzig-bland"])
@pytest.mark.parametrize("shape", ["wide", "tall"])
def test_slack_shapes_beyond_one_trip_of_the_workgroup(shape, rule):
    """wide: 41 x 341, 340 priced columns (a second trip, a tree that does not start at a full power of two);
    tall: 301 x 341, 300 ratio rows."""
    seed = pc.WIDE_SLACK["seed"] if shape == "wide" else pc.TALL_SLACK["seed"]
    T, b, trace, model = _slack_model(shape, seed, rule)
    assert T.shape == ((41, 341) if shape == "wide" else (301, 341))
    assert trace != _slack_model(shape, seed, "dantzig")[2]
    t = _int_tableau(T, b, rule)
    rc, n = _solve(t, SLACK_CAP)
    assert (rc, n) == (capi.MI_OPTIMAL, len(trace)), capi.lib().mi355x_last_error()
    assert _pairs(t.pivot_trace()) == trace and t.bits == 64
    _same_state(t, model)


# ---- 4. the flag survives between calls ----------------------------------------------------------------------
def test_rule_2_in_calls_of_five_pivots_makes_the_one_call_trace():
    T, b, trace, model = _slack_model("wide", pc.WIDE_SLACK["seed"], "dantzig-bland")
    deg = pc.degenerate_flags(T, b, trace)
    assert any(deg[k - 1] for k in range(5, len(trace), 5))          # a call starts with the flag set
    t = _int_tableau(T, b, "dantzig")
    lp.exact.n_solve_exact(t, max_pivots=SLACK_CAP, chunk=5, pivot_rule="dantzig-bland")
    assert t.n_pivots == len(trace) and _pairs(t.pivot_trace()) == trace
    _same_state(t, model)


# ---- 5. two-phase: the flag is cleared at the hand-over ------------------------------------------------------
# (seed 7: the issue's case; seeds 24 and 26: phase 1 ends on a degenerate pivot under rule 2, and a flag kept
# over the hand-over would make phase 2 start with another pivot -- tests/test_pivot_rule_host.py shows it)
MIXED_SEEDS = (7, 24, 26, 7)


@functools.lru_cache(maxsize=None)
def _mixed_model(seed, rule):
    p = ec.mixed_problem(lp, 6, 3, 2, 1, seed=seed)
    keep = {}
    st, trace, mm, stats = pc.solve_tabs(rr.build_tableau(ec.to_dict(p)), rule, SMALL_CAP, keep=keep)
    assert st == "optimal" and stats["driveouts"] == 2 and not stats["inexact"] and stats["max_bits"] <= 64
    return p, trace, mm, keep


def _trace(sol):
    return _pairs(sol.phase1.pivot_trace()) + _pairs(sol.pivot_trace())


@pytest.mark.parametrize("rule", pc.RULES)
def test_two_phase_pair_and_two_phase_batch_members(rule):
    assert _mixed_model(7, rule)[2].matrix()[-1][-1] == Fraction(158, 9)
    assert len({tuple(_mixed_model(7, r)[1]) for r in pc.RULES}) == 3
    for seed in (7, 24):
        p, trace, mm, keep = _mixed_model(seed, rule)
        sol = lp.solve_problem(p, exact=True, pivot_rule=rule, max_pivots=SMALL_CAP)
        assert _trace(sol) == trace and tuple(sol.n_pivots) == (keep["n1"] + 2, len(trace) - keep["n1"])
        _same_state(sol, mm)
        _same_state(sol.phase1, keep["art"])
    # ... and as members of one pair of batches
    refs = [_mixed_model(s, rule) for s in MIXED_SEEDS]
    got = lp.solve_problems([r[0] for r in refs], exact=True, pivot_rule=rule, max_pivots=SMALL_CAP, errorp=False)
    for g, (_, tr, m, k) in zip(got, refs):
        assert isinstance(g, lp.ExactTableau) and g._batch is not None, g
        assert _trace(g) == tr
        _same_state(g, m)
        _same_state(g.phase1, k["art"])


# ---- 6. a batch of same-shape members, one of them cycling under the default rule ----------------------------
def _variant_batch(rule):
    ps = pc.beale_variants(lp)
    tabs = [lp.build_tableau(p, exact=True) for p in ps]
    assert {t._matrix.shape for t in tabs} == {(4, 8)}
    return ps, tabs, lp.exact.XBatch(tabs, pivot_rule=rule)


def _member(xb, q):
    """(T, D, basis, trace) of member q."""
    t = lp.ExactTableau.__new__(lp.ExactTableau)
    t._matrix = np.empty((xb.rows, xb.cols), dtype=object)
    t._batch, t._handle = (xb, q), None
    T, D, basis = t.raw()
    return T, D, basis, _pairs(t.pivot_trace())


@pytest.mark.parametrize("rule", ["bland", "dantzig-bland"])
def test_a_member_that_would_cycle_ends_beside_the_others(rule):
    ps, tabs, xb = _variant_batch(rule)
    rc, st, npv = xb.solve(True, SMALL_CAP)
    assert rc == capi.MI_OK and st.tolist() == [capi.MI_OPTIMAL] * 4
    for q, p in enumerate(ps):
        mst, trace, model, stats = pc.solve_tabs(rr.build_tableau(ec.to_dict(p)), rule, SMALL_CAP)
        assert mst == "optimal" and not stats["inexact"]
        T, D, basis, gtrace = _member(xb, q)
        assert gtrace == trace and npv[q] == len(trace)
        assert D == model.D and basis.tolist() == model.basis and _ints(T) == _ints(model.T)
    assert _member(xb, 0)[3] == pc.BEALE_TRACE and _member(xb, 3)[3] == pc.CHVATAL_TRACE
    xb.close()


def test_under_the_default_rule_the_cycling_members_stop_at_the_cap_and_the_others_end():
    ps, tabs, xb = _variant_batch("dantzig")
    rc, st, npv = xb.solve(True, 60)
    assert rc == capi.MI_OK and st.tolist() == [capi.MI_MAX_PIVOTS, capi.MI_OPTIMAL, capi.MI_OPTIMAL, capi.MI_MAX_PIVOTS]
    assert _member(xb, 0)[3] == pc.PERIOD * 10 and _member(xb, 3)[3] == pc.PERIOD * 10
    for q in (1, 2):
        assert npv[q] == len(pc.solve_tabs(rr.build_tableau(ec.to_dict(ps[q])), "dantzig", SMALL_CAP)[1])
    xb.close()


# ---- 7. a batch from states, members of more columns than threads; in one call and in short calls ------------
@pytest.mark.parametrize("chunk", [None, 7])
def test_batch_from_states_of_the_wide_slack_shape(chunk):
    refs = [_slack_model("wide", seed, "dantzig-bland") for seed in range(4)]
    assert len({tuple(r[2]) for r in refs}) == 4
    for seed, r in enumerate(refs):
        assert r[2] != _slack_model("wide", seed, "dantzig")[2]
    num = np.stack([r[0] for r in refs])
    xb = lp.exact.XBatch.from_states(num, np.ones_like(num), np.stack([r[1] for r in refs]), pivot_rule="dantzig-bland")
    st, total = lp.exact.batch_in_chunks(xb, None, True, SLACK_CAP, chunk)
    assert st.tolist() == [capi.MI_OPTIMAL] * 4
    for q, (_, _, trace, model) in enumerate(refs):
        T, D, basis, gtrace = _member(xb, q)
        assert gtrace == trace and total[q] == len(trace)
        assert D == model.D and basis.tolist() == model.basis and _ints(T) == _ints(model.T)
    xb.close()


# ---- 8. the restart at a wider width clears the flag ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restart_model():
    T, b = pc.restart_state()
    st, trace, m = pc.solve_state(T, b, "dantzig-bland", pc.RESTART_CAP)
    deg = pc.degenerate_flags(T, b, trace)
    stage, at = m.stats["over64"]
    assert st == "max_pivots" and 64 < m.stats["max_bits"] <= 128 and not m.stats["inexact"]
    assert any(deg[:at]) and deg[at - 1] and deg[at]       # a degenerate pivot, then the overflow, the flag standing
    first = pc.BlandVec.from_state(T, 1, b, T.shape[1] - 1)
    e = first.price(True)
    assert (e, first.ratio(e)) != trace[0]                 # a replay that kept the flag would start elsewhere
    return T, b, trace, m


def test_restart_at_128_bits_replays_the_same_pivots_single_tableau():
    T, b, trace, model = _restart_model()
    t = _int_tableau(T, b, "dantzig-bland")
    assert t.bits == 64
    rc, n = _solve(t, pc.RESTART_CAP)
    assert (rc, n) == (capi.MI_MAX_PIVOTS, len(trace)), capi.lib().mi355x_last_error()
    assert t.bits == 128 and _pairs(t.pivot_trace()) == trace
    _same_state(t, model)


def test_restart_at_128_bits_replays_the_same_pivots_batch_member():
    T, b, trace, model = _restart_model()
    small = T.copy()
    small[:-1, :8] = np.sign(small[:-1, :8]) * (np.abs(small[:-1, :8]) >> 17)     # the same shape, entries below 8
    small[-1, :8] = -(np.abs(small[-1, :8]) >> 17) - 1
    sst, strace, smodel = pc.solve_state(small, b, "dantzig-bland", pc.RESTART_CAP)
    assert smodel.stats["max_bits"] <= 64 and not smodel.stats["inexact"]
    num = np.stack([T, small])
    xb = lp.exact.XBatch.from_states(num, np.ones_like(num), np.stack([b, b]), pivot_rule="dantzig-bland")
    rc, st, npv = xb.solve(True, pc.RESTART_CAP)
    assert rc == capi.MI_OK and st.tolist() == [capi.MI_MAX_PIVOTS, CODES[sst]]
    bits = ctypes.c_int(0)
    for q, (tr, m, want_bits) in enumerate(((trace, model, 128), (strace, smodel, 64))):
        Tq, D, basis, gtrace = _member(xb, q)
        assert gtrace == tr and npv[q] == len(tr)
        assert D == m.D and basis.tolist() == m.basis and _ints(Tq) == _ints(m.T)
        assert capi.lib().mi355x_xbatch_bits(xb.handle, q, ctypes.byref(bits)) == capi.MI_OK and bits.value == want_bits
    xb.close()


# ---- 9. exact branch-and-bound ---------------------------------------------------------------------------------
def _exact(p):
    """bb_oracle.random_ilp's float problem (every number a multiple of 1/4) with the same numbers as Fractions."""
    F = Fraction
    return dataclasses.replace(p, objective_func=[(v, F(c)) for v, c in p.objective_func],
                               var_bounds=[(v, (None if lo is None else F(lo), None if hi is None else F(hi)))
                                           for v, (lo, hi) in p.var_bounds],
                               constraints=[(op, [(v, F(c)) for v, c in e], F(r)) for op, e, r in p.constraints])


def _model_round(problem, rule):
    """exact_bb.search's solve_round with the rule's model as node solver."""
    def solve_round(entries):
        out = []
        for e in entries:
            try:
                tabs = rr.build_tableau(ec.to_dict(B.node_problem(problem, e, Fraction(1))))
            except rr.Unbounded:
                out.append((capi.MI_UNBOUNDED, None, None))
                continue
            st, _, m, stats = pc.solve_tabs(tabs, rule, SLACK_CAP)
            assert not stats["inexact"]
            if st != "optimal":
                out.append((CODES[st], None, None))
                continue
            t = (tabs[1] if isinstance(tabs, tuple) else tabs).copy()
            t.matrix, t.basis = m.matrix(), list(m.basis)
            out.append((capi.MI_OPTIMAL, rr.objective_value(t), {v: rr.tableau_variable(t, v) for v in problem.vars}))
        return out
    return solve_round


@functools.lru_cache(maxsize=None)
def _bb_problems():
    cases = B.load_cases()
    ps = [(name, B.problem_of(cases[name]["problem"], exact=True)) for name in sorted(cases)]
    seeds, seed = [], 1000
    while len(seeds) < 3:                                   # three random programs whose default search branches
        p = _exact(B.random_ilp(seed))
        try:
            res = B.branch_and_bound(p, exact=True, max_nodes=40)
        except RuntimeError:
            res = None
        if res is not None and len(res[2]) >= 3:
            seeds.append(("random_ilp(%d)" % seed, p))
        seed += 1
    return ps + seeds


@functools.lru_cache(maxsize=None)
def _bb_reference(rule):
    """Per problem: the CPU replay of the search under the rule, and the default rule's oracle result."""
    return [(name, p, xbb.search(p, _model_round(p, rule), 1), B.branch_and_bound(p, exact=True))
            for name, p in _bb_problems()]


@pytest.mark.parametrize("width", [1, 8])
@pytest.mark.parametrize("rule", ["bland", "dantzig-bland"])
def test_exact_branch_and_bound_follows_the_rules_model(rule, width):
    for name, p, want, (ost, obest, _) in _bb_reference(rule):
        rounds = xbb.DeviceRounds(p, max_pivots=SLACK_CAP, pivot_rule=rule)
        got = xbb.search(p, rounds, width)
        assert got.status == want.status, name
        assert B.trace_key(got.trace) == B.trace_key(want.trace), name             # the same nodes
        assert got.objectives == want.objectives and got.objective == want.objective, name
        if want.values is not None:
            assert {v: got.values[v] for v in p.vars} == {v: want.values[v] for v in p.vars}, name
        assert got.objective == (obest[0] if obest else None), name                # the default rule's optimum
        assert rounds.declined == 0


def test_branch_and_bound_through_the_solver_hook():
    name, p, want, (ost, obest, _) = [r for r in _bb_reference("dantzig-bland") if r[3][1] is not None][0]
    t = lp.solve_problem(p, exact=True, branch_and_bound=True, bb_width=4, pivot_rule="dantzig-bland", max_pivots=SLACK_CAP)
    assert isinstance(t, lp.ExactTableau) and lp.solution_objective_value(t) == obest[0]
    for v in p.vars:
        assert lp.solution_variable(t, v) == want.values[v]


# ---- 10. the public interface ----------------------------------------------------------------------------------
def test_solve_problem_ends_on_beales_lp():
    p = ec.beale(lp)
    t = lp.solve_problem(p, exact=True, pivot_rule="dantzig-bland", max_pivots=SMALL_CAP)
    assert isinstance(t, lp.ExactTableau) and t.pivot_rule == "dantzig-bland"
    assert lp.solution_objective_value(t) == Fraction(5, 4) and _pairs(t.pivot_trace()) == pc.BEALE_TRACE
    st, _, model, _ = _cycling_model("beale", "dantzig-bland")
    ref = rr.build_tableau(ec.to_dict(p)).copy()
    ref.matrix, ref.basis = model.matrix(), list(model.basis)
    for v in p.vars:
        x = lp.solution_variable(t, v)
        assert type(x) is Fraction and x == rr.tableau_variable(ref, v)
    assert [lp.solution_variable(t, v) for v in p.vars] == [Fraction(1), Fraction(0), Fraction(1), Fraction(0)]


def test_solve_problems_with_a_float_member():
    p = ec.beale(lp)
    fl = dataclasses.replace(p, objective_func=[(v, float(c)) for v, c in p.objective_func])
    got = lp.solve_problems([p, fl, p], exact=True, pivot_rule="bland", max_pivots=SMALL_CAP, errorp=False)
    for g in (got[0], got[2]):
        assert isinstance(g, lp.ExactTableau) and g._batch is not None
        assert lp.solution_objective_value(g) == Fraction(5, 4) and _pairs(g.pivot_trace()) == pc.BEALE_TRACE
    assert isinstance(got[1], lp.UnsupportedConstraintError)
    assert tuple(got[1].constraint) == ("exact", "pivot-rule", "bland")
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problems([p, fl, p], exact=True, pivot_rule="bland", max_pivots=SMALL_CAP)


def test_setter_errors():
    L = capi.lib()
    t = lp.build_tableau(ec.beale(lp), exact=True)
    assert L.mi355x_xtab_set_pivot_rule(t._h, 3) == capi.MI_BAD_ARG
    assert L.mi355x_xtab_set_pivot_rule(t._h, -1) == capi.MI_BAD_ARG
    assert L.mi355x_xtab_set_pivot_rule(t._h, capi.MI_RULE_BLAND) == capi.MI_OK
    assert L.mi355x_xtab_set_pivot_rule(t._h, capi.MI_RULE_DANTZIG_BLAND) == capi.MI_OK      # still no pivot
    assert _solve(t, 2) == (capi.MI_MAX_PIVOTS, 2)
    assert L.mi355x_xtab_set_pivot_rule(t._h, capi.MI_RULE_BLAND) == capi.MI_BAD_ARG
    assert b"first pivot" in L.mi355x_last_error()
    with pytest.raises(capi.Mi355xError):
        t.set_pivot_rule("bland")
    assert t.pivot_rule == "dantzig"                        # (the Python attribute follows successful calls only)
    rc, n = _solve(t, SMALL_CAP)                            # the rule it had goes on: the rest of the trace
    assert rc == capi.MI_OPTIMAL and _pairs(t.pivot_trace()) == pc.BEALE_TRACE
    ps, tabs, xb = _variant_batch("dantzig")
    assert L.mi355x_xbatch_set_pivot_rule(xb.handle, 3) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_set_pivot_rule(xb.handle, capi.MI_RULE_DANTZIG_BLAND) == capi.MI_OK
    rc, st, npv = xb.solve(True, 1)
    assert rc == capi.MI_OK and npv.tolist() == [1, 1, 1, 1]
    assert L.mi355x_xbatch_set_pivot_rule(xb.handle, capi.MI_RULE_BLAND) == capi.MI_BAD_ARG
    with pytest.raises(capi.Mi355xError):
        xb.set_pivot_rule("bland")
    rc, st, npv = xb.solve(True, SMALL_CAP)
    assert st.tolist() == [capi.MI_OPTIMAL] * 4 and _member(xb, 0)[3] == pc.BEALE_TRACE
    xb.close()
