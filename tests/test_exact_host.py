"""Exact mode without a GPU: the Fraction builder equals the oracle's build-tableau, the fraction-free
start state reproduces the initial tableau, and a pure-Python model of the Bareiss arithmetic the
exact kernels implement (start state, folded objective LCM, sign-normalised pivots, cross-multiplied
ratio test, hand-over with the full L_c) reproduces the Fraction oracle pivot for pivot."""
from fractions import Fraction

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests import goldens
from tests.helpers import lp_amd

lp = lp_amd()
SEEDS = range(200)


def _golden_problems():
    return [(name, lp.Problem.from_dict(goldens.problem(case))) for name, case in goldens.load()["cases"].items()
            if not case.get("float32_literals")]


def _tabs_equal(ours, ref):
    assert ours.var_count == ref.var_count and ours.constraint_count == ref.constraint_count
    assert ours.matrix.tolist() == ref.matrix
    assert all(isinstance(x, Fraction) for x in ours.matrix.flat)
    assert ours.basis_columns.tolist() == ref.basis
    assert ours.var_mapping == ref.var_mapping


def _check_builder(p):
    try:
        ref = rr.build_tableau(ec.to_dict(p))
    except rr.Unbounded:
        with pytest.raises(lp.UnboundedProblemError):
            lp.build_tableau(p, exact=True)
        return
    ours = lp.build_tableau(p, exact=True)
    if isinstance(ref, tuple):
        assert isinstance(ours, list) and len(ours) == 2
        _tabs_equal(ours[0], ref[0])
        _tabs_equal(ours[1], ref[1])
    else:
        assert isinstance(ours, lp.ExactTableau)
        _tabs_equal(ours, ref)


def test_exact_builder_equals_the_oracle_on_the_goldens():
    for _, p in _golden_problems():
        _check_builder(p)


@pytest.mark.parametrize("seed", SEEDS)
def test_exact_builder_equals_the_oracle_on_random_problems(seed):
    _check_builder(ec.random_problem(lp, seed))


def test_double_builder_is_unchanged_by_the_exact_option():
    for seed in range(20):
        p = ec.random_problem(lp, seed)
        a, b = lp.build_tableau(p), lp.build_tableau(p, exact=False)
        for x, y in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            assert x.matrix.dtype == float and (x.matrix == y.matrix).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_start_state_reproduces_the_initial_tableau(seed):
    tabs = rr.build_tableau(ec.to_dict(ec.random_problem(lp, seed)))
    for t in (tabs if isinstance(tabs, tuple) else (tabs,)):
        T, D = ec.start_state(t.matrix)
        assert D > 0 and [[Fraction(x, D) for x in row] for row in T] == t.matrix


def test_all_integer_problems_start_with_denominator_one():
    tabs = rr.build_tableau(ec.to_dict(lp.Problem.from_dict(goldens.problem(goldens.load()["cases"]["basic"]))))
    assert ec.start_state(tabs.matrix)[1] == 1


def _model_matches_oracle(p):
    tabs = rr.build_tableau(ec.to_dict(p))
    st, trace, t = ec.oracle_outcome(tabs)
    mst, mtrace, mm, stats = ec.model_solve(tabs)
    assert stats["inexact"] == 0
    assert (mst, mtrace) == (st, trace)
    if t is not None:
        assert mm.basis == t.basis and mm.matrix() == t.matrix
    return st, stats


def test_fraction_free_model_reproduces_the_oracle():
    outcomes, negative_driveouts = set(), 0
    for seed in SEEDS:
        st, stats = _model_matches_oracle(ec.random_problem(lp, seed))
        outcomes.add(st)
        if stats["driveouts"]:
            outcomes.add("driveout")
        negative_driveouts += stats["negative_pivots"] > 0
    assert {"optimal", "unbounded", "infeasible", "driveout"} <= outcomes
    assert negative_driveouts > 0
    for _, p in _golden_problems():
        if p.constraints:
            _model_matches_oracle(p)


def test_vectorised_model_equals_the_model_and_the_oracle():
    """exact_cases.VecModel (the reference of the multi-workgroup shapes, tests/test_gpu_exact_shapes.py)
    against exact_cases.Model on the 200 seeds -- status, trace, basis, T, D and the statistics -- and
    directly against the Fraction oracle's final tableau."""
    outcomes, two_phase = set(), 0
    for seed in SEEDS:
        tabs = rr.build_tableau(ec.to_dict(ec.random_problem(lp, seed)))
        st, trace, mm, stats = ec.model_solve(tabs)
        vst, vtrace, vm, vstats = ec.model_solve(tabs, cls=ec.VecModel)
        assert (vst, vtrace, vstats) == (st, trace, stats), seed
        assert (vm is None) == (mm is None)
        outcomes.add(st)
        two_phase += isinstance(tabs, tuple)
        if mm is not None:
            assert vm.basis == mm.basis and vm.D == mm.D and vm.rows() == mm.T, seed
            _, _, t = ec.oracle_outcome(tabs)
            assert [[Fraction(x, vm.D) for x in row] for row in vm.rows()] == t.matrix and vm.basis == t.basis
    assert {"optimal", "unbounded", "infeasible"} <= outcomes and two_phase >= 50
    # both storage forms of the vectorised model: int64 and, past 62 bits, Python ints
    wide = rr.build_tableau(ec.to_dict(ec.wide_problem(lp, 0, 40)))
    st, trace, mm, stats = ec.model_solve(wide)
    vst, vtrace, vm, vstats = ec.model_solve(wide, cls=ec.VecModel)
    assert stats["max_bits"] > 64 and vm.T.dtype == object
    assert (vst, vtrace, vstats) == (st, trace, stats) and vm.rows() == mm.T and vm.D == mm.D
    # ties: the first of equal objective entries and of equal ratios, for max and for min
    T, basis = ec.slack_tableau(12, 9, 3)
    T[-1, :9] = -2
    T[:12, 0], T[:12, -1] = 3, 1
    for is_max in (True, False):
        S = T if is_max else np.concatenate([T[:-1], -T[-1:]])
        a, b = ec.Model.from_state(S.tolist(), 1, basis, 21), ec.VecModel.from_state(S, 1, basis, 21)
        ta, tb = [], []
        assert a.solve(is_max, ta) == b.solve(is_max, tb) and ta == tb and ta[0] == (0, 0)
        assert a.T == b.rows() and a.D == b.D and a.basis == b.basis


def test_model_records_where_64_bits_are_first_exceeded():
    tabs = rr.build_tableau(ec.to_dict(ec.wide_problem(lp, 0, 40)))
    t = ec.Model(tabs.matrix, tabs.basis, tabs.var_count)
    assert t.stats["over64"] is None and t.stats["max_bits"] <= 64
    trace, k = [], 0
    while t.stats["max_bits"] <= 64:
        assert t.solve(tabs.is_max, trace, max_pivots=1) == "max_pivots"
        k += 1
    assert t.stats["over64"] == ("phase1", k - 1) and t.stats["pivots"] == k


def test_exact_route_selection():
    """exact=True takes the exact path iff every number is an int or a Fraction; with branch-and-bound
    it is declined before anything runs."""
    p = ec.random_problem(lp, 3)
    assert lp.exact.rational_problem(p)
    q = lp.Problem(type=p.type, vars=p.vars, objective_var=p.objective_var,
                   objective_func=[(v, float(c)) for v, c in p.objective_func],
                   var_bounds=p.var_bounds, constraints=p.constraints)
    assert not lp.exact.rational_problem(q)
    assert not lp.exact.rational_number(True) and lp.exact.rational_number(Fraction(1, 3))
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problem(p, exact=True, branch_and_bound=True)


def test_exact_status_codes_are_new_negative_codes():
    assert lp.capi.MI_EXACT_OVERFLOW == -7 and lp.capi.MI_EXACT_INEXACT == -8
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.exact.check(lp.capi.MI_EXACT_OVERFLOW, "test")
