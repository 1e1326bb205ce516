"""The single-float path without a GPU: the float32 model of tests/single_cases.py against the reference's own
single-float known answers, the number rule, build_tableau_single against hand-written float32 tableaux, the
keyword's argument errors, and the new C entries' behaviour without a device."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import oracle
from tests import single_cases as sc
from tests.helpers import lp_amd

lp = lp_amd()
F32 = np.float32
README = dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", 1), ("y", 4), ("z", 3)], bounds=[],
              constraints=[("<=", [("x", 2), ("y", 1)], 8), ("<=", [("y", 1), ("z", 1)], 7)])


def lp_problem(d):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[(b[0], (b[1], b[2])) for b in d["bounds"]],
                      constraints=list(d["constraints"]))


def test_epsilon_and_thresholds():
    eps = 2.0 ** -24 * (1 + 2.0 ** -23)
    assert float(sc.EPS_S) == eps == 5.960465188081798e-08 == float(lp.single.EPSILON_SINGLE)
    assert lp.capi.lib().mi355x_epsilon_single() == eps
    for f in (1024, 16):
        p, r, z = sc.thresholds(f)
        assert all(isinstance(x, np.float32) for x in (p, r, z))
        # an eighth and a half of these factors are exact, and so are their products with eps_s
        assert (float(p), float(r), float(z)) == (f / 8 * eps, f / 2 * eps, f * eps)
        assert lp.single.thresholds(f) == (p, r, z)
    assert "%.6e %.6e" % tuple(sc.thresholds(1024)[:2]) == "7.629395e-06 3.051758e-05"


def test_readme_lp():
    r = sc.solve_problem(README)
    assert r["status"] == sc.OPTIMAL and r["trace"] == [(1, 1), (0, 0)]
    z = sc.objective(r["M"])
    assert isinstance(z, np.float32) and z == F32(28.5)
    assert [sc.variable(r["M"], r["basis"], r["mapping"], v) for v in "xyz"] == [F32(0.5), F32(7), F32(0)]
    assert sc.reduced_cost(r["M"], r["mapping"], "z") == F32(0.5)


def _golden(golden, name):
    p = golden["cases"][name]["problem"]

    def cv(x):
        return x if isinstance(x, int) or x is None else F32(x)
    return dict(type=p["type"], vars=p["vars"], objective_var=p["objective_var"],
                objective=[(v, cv(c)) for v, c in p["objective"]], bounds=[(b[0], cv(b[1]), cv(b[2])) for b in p["bounds"]],
                constraints=[(op, [(v, cv(c)) for v, c in e], cv(r)) for op, e, r in p["constraints"]])


def test_float32_literal_goldens(golden):
    """t/integration.lisp:72-80 in the reference's own form, computed in float32: (fp= 0.9372585 z) with the default
    factor 16 and single-float-epsilon; and t/integration.lisp:109-118."""
    case = golden["cases"]["numerical_issue"]
    assert case["float32_literals"] and case["objective_fp_eq"]["epsilon"] == "single-float-epsilon"
    r = sc.solve_problem(_golden(golden, "numerical_issue"))
    assert r["status"] == sc.OPTIMAL
    z = sc.objective(r["M"])
    assert isinstance(z, np.float32)
    assert abs(F32(z - F32(case["objective_fp_eq"]["value"]))) <= F32(F32(case["objective_fp_eq"]["factor"]) * sc.EPS_S)
    r = sc.solve_problem(_golden(golden, "variable_bounds_bug"))
    assert r["status"] == sc.OPTIMAL
    assert [sc.variable(r["M"], r["basis"], r["mapping"], v) for v in "xy"] == [F32(1), F32(1)]


def test_tiny_coefficient_tells_the_precisions_apart():
    """max 1e-6 x s.t. x <= 1: 0 pivots and objective 0 in single-float, 1 pivot on the same numbers as doubles."""
    d = sc.tiny_coefficient_problem()
    b = sc.build(d)
    assert b["art"] is None and b["main"][0][-1, 0] == -F32(1e-6)
    r = sc.solve_problem(d)
    assert r["status"] == sc.OPTIMAL and r["pivots"] == 0 and sc.objective(r["M"]) == F32(0)
    M, basis = b["main"][0].astype(np.float64), b["main"][1].copy()
    st, n, _ = oracle.solve(M, basis, is_max=True, factor=1024.0)
    assert st == oracle.OPTIMAL and n == 1 and M[-1, -1] == float(F32(1e-6))


def test_overflow_case_follows_the_scan_order_rules():
    M0, b0 = sc.overflow_tableau()
    assert M0.shape == (4, 7) and M0.max() == F32(3e38)
    st, tr, M, b = sc.solve(M0, b0, True, cap=20)
    one = M0.copy()
    sc.pivot(one, b0.copy(), 0, 0)
    assert np.isposinf(one[0, 1]) and np.isneginf(one[1, 1]) and np.isnan(one[2, 1]) and np.isposinf(one[3, 1])
    # the second pivot leaves inf - inf in the objective row; that NaN (not in column 0) never enters: optimal
    assert (st, tr) == (sc.OPTIMAL, [(0, 0), (2, 1)]) and np.isnan(M[3, 1])
    assert sc.price(M, True) is None
    # a NaN in column 0 is never replaced, and (fp< NaN 0) fails: optimal whatever follows it
    obj = M0.copy()
    obj[3, 0] = np.nan
    assert sc.price(obj, True) is None and sc.price(obj, False) is None
    # a NaN quotient wins only as the first eligible row
    q = np.array([[1, 1, 0, np.nan], [1, 0, 1, 2], [-1, 0, 0, 0]], dtype=F32)
    assert sc.ratio(q, 0) == 0
    q[[0, 1]] = q[[1, 0]]
    assert sc.ratio(q, 0) == 0


def test_number_rule():
    ok = [0, 1, -3, 2 ** 24, -2 ** 24, F32(0.1), 0.5, 1.0, float(F32(0.6861807)), np.float64(0.25), np.int64(7)]
    bad = [0.1, 1e-6, 2 ** 24 + 1, -2 ** 24 - 1, Fraction(1, 2), 1e300, float("nan"), True, "1"]
    assert all(lp.single.single_number(x) for x in ok)
    assert not any(lp.single.single_number(x) for x in bad)
    for x in (0.1, Fraction(1, 3), 2 ** 24 + 1):
        for where in ("objective", "constraint", "rhs", "bound"):
            d = dict(README, objective=list(README["objective"]), constraints=[list(c) for c in README["constraints"]],
                     bounds=[])
            if where == "objective":
                d["objective"][1] = ("y", x)
            elif where == "constraint":
                d["constraints"][0][1] = [("x", x), ("y", 1)]
            elif where == "rhs":
                d["constraints"][1][2] = x
            else:
                d["bounds"] = [("x", x, None)]
            d["constraints"] = [tuple(c) for c in d["constraints"]]
            with pytest.raises(lp.UnsupportedConstraintError) as e:
                lp.build_tableau_single(lp_problem(d))
            assert e.value.constraint == ("single", x) and e.value.solver_name == "mi355x-simplex"
            with pytest.raises(lp.UnsupportedConstraintError) as e:
                lp.solve_problem(lp_problem(d), precision="single")
            assert e.value.constraint == ("single", x)


def test_build_tableau_single_against_hand_written_tableaux():
    # a lower bound that shifts an RHS inexactly: rhs - coef * lb = 1 - 0.1f * 0.3f in float32 operations
    c, lb = F32(0.1), F32(0.3)
    d = dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", c), ("y", 2)], bounds=[("x", lb, None)],
             constraints=[("<=", [("x", c), ("y", 1)], 1)])
    t = lp.build_tableau_single(lp_problem(d))
    rhs = F32(F32(1) - F32(c * lb))
    assert rhs != F32(1 - float(c) * float(lb))              # the double intermediate would round elsewhere
    want = np.array([[c, 1, 1, rhs], [-c, -2, 0, F32(F32(0) + F32(c * lb))]], dtype=F32)
    assert t.matrix.dtype == np.float32 and sc.same_bits(t.matrix, want) and t.basis_columns.tolist() == [2]
    assert t.var_mapping == {"x": ("positive", 0, lb), "y": ("positive", 1, 0)}
    assert sc.same_bits(sc.build(d)["main"][0], want)
    # a free variable: two columns, coef and -coef
    d = dict(type="min", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", F32(0.5))], bounds=[("x", None, None)],
             constraints=[(">=", [("x", F32(1.5)), ("y", 1)], 2)])
    art, main = lp.build_tableau_single(lp_problem(d))
    h = F32(1.5)
    assert sc.same_bits(main.matrix, np.array([[h, -h, 1, -1, 2], [-1, 1, -F32(0.5), 0, 0]], dtype=F32))
    assert sc.same_bits(art.matrix, np.array([[h, -h, 1, -1, 1, 2], [h, -h, 1, -1, 0, 2]], dtype=F32))
    assert main.basis_columns.tolist() == [5] and art.basis_columns.tolist() == [4] and art.instance_problem.type == "min"
    b = sc.build(d)
    assert sc.same_bits(b["main"][0], main.matrix) and sc.same_bits(b["art"][0], art.matrix)
    # both bounds: the upper bound becomes a `<=` row in front, shifted by the lower bound
    d = dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", 1)],
             bounds=[("y", F32(0.25), F32(2.5))], constraints=[("<=", [("x", 1), ("y", 2)], 8)])
    t = lp.build_tableau_single(lp_problem(d))
    want = np.array([[0, 1, 1, 0, F32(2.25)], [1, 2, 0, 1, F32(7.5)], [-1, -1, 0, 0, F32(0.25)]], dtype=F32)
    assert sc.same_bits(t.matrix, want) and t.basis_columns.tolist() == [2, 3]
    assert sc.same_bits(sc.build(d)["main"][0], want)
    # integers stay exact among themselves: as float32 products these two would sum to 4
    d = dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", 2 ** 24 - 1), ("y", -(2 ** 24 - 2))],
             bounds=[("x", 3, None), ("y", 3, None)], constraints=[("<=", [("x", 1), ("y", 1)], 10)])
    assert F32(F32(2 ** 24 - 1) * F32(3)) + F32(F32(-(2 ** 24 - 2)) * F32(3)) == 4
    t = lp.build_tableau_single(lp_problem(d))
    assert t.matrix[-1, -1] == F32(3) and t.matrix[0, -1] == F32(4) and sc.same_bits(sc.build(d)["main"][0], t.matrix)


def test_read_back_returns_float32():
    t = lp.build_tableau_single(lp_problem(README))
    assert isinstance(lp.single.tableau_objective_value(t), np.float32)
    assert isinstance(lp.tableau_variable(t, "x"), np.float32) and lp.tableau_variable(t, "x") == 0
    assert isinstance(lp.tableau_reduced_cost(t, "y"), np.float32) and lp.tableau_reduced_cost(t, "y") == -4
    assert lp.tableau_variable(t, "w") == 0


def test_keyword_argument_errors():
    p = lp_problem(README)
    for kw, name in ((dict(exact=True), "exact"), (dict(branch_and_bound=True), "branch_and_bound"),
                     (dict(devices=2), "devices"), (dict(native=True), "native"), (dict(full_tableau=True), "full_tableau"),
                     (dict(pivot_rule="bland", exact=False), "pivot_rule")):
        with pytest.raises(ValueError) as e:
            lp.solve_problem(p, precision="single", **kw)
        assert "single" in str(e.value) and name in str(e.value)
    with pytest.raises(ValueError) as e:
        lp.solve_problem(p, precision="half")
    assert "half" in str(e.value)


@pytest.mark.skipif(lp.capi.device_count() > 0, reason="a GPU is present")
def test_new_entries_without_a_device():
    L = lp.capi.lib()
    M = np.zeros((3, 4), dtype=F32)
    b = np.zeros(2, dtype=np.int64)
    h = ctypes.c_void_p()
    rc = L.mi355x_stab_create(ctypes.byref(h), 3, 4, M.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), 0)
    assert rc == lp.capi.MI_NO_DEVICE and not h.value
    assert b"no HIP device" in L.mi355x_last_error()
    with pytest.raises(lp.capi.Mi355xError):
        lp.solve_problem(lp_problem(README), precision="single")


def test_new_entries_validate_their_arguments():
    L = lp.capi.lib()
    BAD = lp.capi.MI_BAD_ARG
    h = ctypes.c_void_p()
    M = np.zeros((3, 4), dtype=F32)
    assert L.mi355x_stab_create(None, 3, 4, M.ctypes.data_as(ctypes.c_void_p), None, 0) == BAD
    assert L.mi355x_stab_create(ctypes.byref(h), 3, 4, None, None, 0) == BAD
    assert L.mi355x_stab_create(ctypes.byref(h), 0, 4, M.ctypes.data_as(ctypes.c_void_p), None, 0) == BAD
    assert L.mi355x_stab_create(ctypes.byref(h), 3, 4, M.ctypes.data_as(ctypes.c_void_p), None, 0) == BAD   # rows > 1: a basis
    n = ctypes.c_int64()
    assert L.mi355x_stab_price(None, 1, 1024.0, ctypes.byref(n)) == BAD
    assert L.mi355x_stab_ratio(None, 0, 1024.0, ctypes.byref(n)) == BAD
    assert L.mi355x_stab_pivot(None, 0, 0) == BAD
    assert L.mi355x_stab_solve(None, 1, 1024.0, 0, None) == BAD
    assert L.mi355x_stab_solve_two_phase(None, None, 1, 1024.0, 0, None) == BAD
    assert L.mi355x_stab_download(None, None, None, None, None) == BAD
    assert L.mi355x_stab_trace(None, None, None, 0, None) == BAD
    assert L.mi355x_stab_info(None, None, None, None, None, None) == BAD
    assert L.mi355x_tune_set_single_form(3) == BAD and L.mi355x_tune_set_single_form(0) == 0
    L.mi355x_stab_destroy(None)                              # no-op
