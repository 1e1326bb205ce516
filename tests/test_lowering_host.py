"""One copy of build-tableau across the precisions (linear-programming_amd/lowering.py), without a GPU.

On problems whose numbers are all integers of magnitude <= 8 every intermediate of build-tableau is exact in
binary32, so the double, the exact and the single-float build must state the same tableaux -- shapes, bases,
mapping structure, and every entry as a rational -- and the three read-backs of the unsolved tableaux must agree
in the same sense.  Handles are created lazily: nothing here touches a device."""
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import lps_cases
from tests.helpers import lp_amd

lp = lp_amd()
lowering = lp.lowering
N_PROBLEMS = 56
BOUNDS = {"plain": [None], "lower": [(1, None), (-2, None), (3, None)], "upper+": [(None, 0), (None, 2), (None, 5)],
          "upper-": [(None, -1), (None, -3)], "both+": [(-1, 4), (0, 2), (2, 8)], "both-": [(-6, -2), (-8, -1)],
          "free": [(None, None)]}
assert set(BOUNDS) == set(lps_cases.KINDS)


def problem(seed, constraints=True):
    """Integers of magnitude <= 8 only; over the seeds every kind of bound and every sense, right-hand sides that
    are negative from the start or through an offset, zero coefficients, a repeated variable."""
    rng = random.Random(seed)
    names = ["x%d" % i for i in range(rng.randint(2, 4))]
    kinds = [lps_cases.KINDS[(seed + i) % len(lps_cases.KINDS)] if i < 2 else rng.choice(lps_cases.KINDS)
             for i in range(len(names))]
    bounds = [(v, rng.choice(BOUNDS[k])) for v, k in zip(names, kinds) if k != "plain"]
    cons = []
    for i in range(rng.randint(1, 4) if constraints else 0):
        expr = [(v, rng.randint(-3, 3)) for v in names if rng.random() < 0.8] or [(names[0], 1)]
        if rng.random() < 0.2:
            expr.append((expr[0][0], rng.randint(-3, 3)))                # a later term of the same variable
        cons.append((lps_cases.OPS[(seed + i) % 3], expr, rng.randint(-4, 8)))
    obj = [(v, rng.choice((-2, -1, 1, 2, 3))) for v in names]
    p = lp.Problem(type=("max", "min")[seed % 2], vars=names, objective_var="w", objective_func=obj,
                   var_bounds=bounds, constraints=cons)
    return p, set(kinds), {op for op, _, _ in cons}


def builds(p):
    """The double, exact and single-float builds, each as a list of one or two tableaux."""
    out = [lp.build_tableau(p), lp.build_tableau(p, exact=True), lp.build_tableau_single(p)]
    assert [type(t if not isinstance(t, list) else t[0]) for t in out] == [lp.Tableau, lp.ExactTableau, lp.SingleTableau]
    return [t if isinstance(t, list) else [t] for t in out]


def same_number(d, x, s):
    """Fraction(double) == exact == Fraction(float(single)), each of its precision's type."""
    assert type(d) in (float, np.float64) and type(x) is Fraction and type(s) in (np.float32, int)
    assert Fraction(float(d)) == x == Fraction(float(s)), (d, x, s)


def same_tableaux(td, tx, ts):
    assert td._handle is None and tx._handle is None and ts._handle is None
    assert td.matrix.shape == tx.matrix.shape == ts.matrix.shape
    assert (td.var_count, td.constraint_count) == (tx.var_count, tx.constraint_count) == (ts.var_count, ts.constraint_count)
    assert td.matrix.dtype == np.float64 and tx.matrix.dtype == object and ts.matrix.dtype == np.float32
    assert td.basis_columns.tolist() == tx.basis_columns.tolist() == ts.basis_columns.tolist()
    assert td.instance_problem.type == tx.instance_problem.type == ts.instance_problem.type
    for d, x, s in zip(td.matrix.flat, tx.matrix.flat, ts.matrix.flat):
        same_number(d, x, s)
    assert list(td.var_mapping) == list(tx.var_mapping) == list(ts.var_mapping)           # key order
    for var in td.var_mapping:
        md, mx, ms = td.var_mapping[var], tx.var_mapping[var], ts.var_mapping[var]
        assert md[:2] == mx[:2] == ms[:2] and len(md) == len(mx) == len(ms) == (2 if md[0] == "signed" else 3)
        if len(md) == 3:
            same_number(md[2], mx[2], ms[2])


def same_readback(td, tx, ts):
    tabs = (td, tx, ts)
    same_number(*(lp.tableau_objective_value(t) for t in tabs))
    for var in list(td.problem.vars) + [td.instance_problem.objective_var]:
        if var is None:
            continue
        got = [lp.tableau_variable(t, var) for t in tabs]
        assert type(got[2]) is np.float32
        same_number(*got)
        if var in td.var_mapping and td.var_mapping[var][0] == "positive":
            got = [lp.tableau_reduced_cost(t, var) for t in tabs]
            assert type(got[2]) is np.float32
            same_number(*got)
        elif var in td.var_mapping:
            for t in tabs:
                with pytest.raises(ValueError):
                    lp.tableau_reduced_cost(t, var)
    for t in tabs:
        with pytest.raises(KeyError):
            lp.tableau_variable(t, "no such variable")


def test_three_precisions_build_the_same_tableaux_and_read_them_back_alike():
    kinds, senses, two_phase = set(), set(), 0
    for seed in range(N_PROBLEMS):
        p, k, s = problem(seed)
        kinds |= k
        senses |= s
        bd, bx, bs = builds(p)
        assert len(bd) == len(bx) == len(bs)
        two_phase += len(bd) == 2
        for td, tx, ts in zip(bd, bx, bs):
            same_tableaux(td, tx, ts)
            same_readback(td, tx, ts)
        if len(bd) == 2:                                                  # the pair shares one mapping
            assert all(b[0].var_mapping is b[1].var_mapping for b in (bd, bx, bs))
    assert N_PROBLEMS >= 50 and two_phase >= 10, two_phase
    assert kinds == set(lps_cases.KINDS) and senses == set(lps_cases.OPS)


def test_problems_without_constraints_agree_across_the_precisions():
    """The branch of its own (src/simplex.lisp:153-186): the same tableau, or unbounded in all three."""
    built = unbounded = 0
    for seed in range(N_PROBLEMS):
        p, _, _ = problem(seed, constraints=False)
        outcomes = []
        for build in (lp.build_tableau, lambda q: lp.build_tableau(q, exact=True), lp.build_tableau_single):
            try:
                outcomes.append(build(p))
            except lp.UnboundedProblemError:
                outcomes.append(None)
        if outcomes[0] is None:
            assert outcomes == [None, None, None]
            unbounded += 1
            continue
        built += 1
        same_tableaux(*outcomes)
        same_readback(*outcomes)
        assert all(t.instance_problem is p for t in outcomes)
    assert built >= 5 and unbounded >= 5, (built, unbounded)


def test_the_rows_a_device_built_batch_starts_from_are_build_tableaus_first_stage():
    """lower (what lower_problem_rows / lower_problem hand to the device) followed by assemble is build_tableau,
    bit for bit, in every number system; lower_problem_rows' L is lower's."""
    for seed in range(N_PROBLEMS):
        p, _, _ = problem(seed)
        for ns, tabs in zip((lowering.DOUBLE, lowering.EXACT, lp.single.SINGLE), builds(p)):
            L, ncv, constraints, mapping = lowering.lower(p, ns)
            assert L.shape == (len(constraints) + 1, ncv + 1)
            M, basis, A, abasis = lowering.assemble(L, ncv, constraints, ns)
            main, art = tabs[-1], (tabs[0] if len(tabs) == 2 else None)
            assert (A is None) == (art is None)
            for t, G, b in ((main, M, basis), (art, A, abasis)):
                if t is None:
                    continue
                G = ns.matrix(G)
                assert b.tolist() == t.basis_columns.tolist() and G.shape == t.matrix.shape
                if G.dtype == object:
                    assert all(x == y for x, y in zip(G.flat, t.matrix.flat))
                else:
                    assert G.dtype == t.matrix.dtype and G.tobytes() == t.matrix.tobytes()
            assert ns.mapping(mapping) == main.var_mapping
            if ns is lowering.DOUBLE:
                rows = lp.lower_problem_rows(p)
                assert rows.L.tobytes() == L.tobytes() and rows.mapping == main.var_mapping
                assert rows.sense.tolist() == [lps_cases.OPS.index(op) for op, _, _ in constraints]
