"""Device-built exact batches, host side (no GPU): exact_lps.lower_problem and the integer assembly rule of
k_xb_assemble_lps (tests/exact_lps_cases.assemble) against build_tableau(exact=True) + exact_cases.start_state,
the grouping, and mi355x_xbatch_create_lps's argument validation."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_cases as ec
from tests import exact_lps_cases as xc
from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi
xl = lp.exact_lps


def _check(p):
    """lower_problem + the integer rule == start_state(build_tableau(exact=True)): True for a two-phase problem."""
    main, art = xc.host_states(lp, p)
    low = xl.lower_problem(p)
    assert low is not None and low.num.dtype == low.den.dtype == np.int64 and low.sense.dtype == np.int32
    assert low.mapping == lp.build_tableau(p, exact=True, general=True).var_mapping
    assert low.is_max == (p.type == "max")
    Dm, M, mb, Da, A, ab = xc.assemble(low.num, low.den, low.sense)
    assert (M, Dm, mb) == main
    assert (art is None) == (A is None)
    if art is not None:
        assert (A, Da, ab) == art
        n_eq, n_art = xl.row_counts(low.num, low.sense)
        assert n_art == len(A[0]) - len(M[0]) and n_eq == sum(op == "=" for op, _, _ in p.constraints)
    return art is not None


def test_lowering_and_the_integer_rule_equal_build_tableau_and_start_state():
    two_phase = sum(_check(ec.random_problem(lp, seed)) for seed in range(400))
    assert two_phase >= 368
    assert all(_check(ec.mixed_problem(lp, 6, 3, 2, 1, s)) for s in range(24))
    assert not any(_check(ec.divergent_problem(lp, s)) for s in range(20))
    assert not any(_check(xc.dense_slack_problem(lp, 8, s)) for s in range(4))


def test_an_integral_artificial_objective_row_keeps_the_scale():
    p = xc.reduction_problem(lp)
    low = xl.lower_problem(p)
    Dm, M, mb, Da, A, ab = xc.assemble(low.num, low.den, low.sense)
    assert Da == 36 and Dm == 36
    assert A[2] == [36, 36, -36, -36, 0, 0, 72] and ab == [5, 4]
    (_, _, _), (T, D, basis) = xc.host_states(lp, p)
    assert D == 36 and T == A and basis == ab
    assert _check(p)


def test_a_repeated_variable_and_every_kind_of_bound_lower_as_build_tableau_does():
    F = Fraction
    p = lp.Problem(type="min", vars=["a", "b", "c", "d", "e"], objective_var="w",
                   objective_func=[("a", 2), ("b", F(-1, 3)), ("c", 1), ("d", F(5, 2)), ("e", -1)],
                   var_bounds=[("a", (F(1, 2), 4)), ("b", (None, F(7, 3))), ("c", (None, None)), ("d", (-2, None)),
                               ("e", (-5, -1))],
                   constraints=[("<=", [("a", 1), ("b", 2), ("a", F(3, 4))], 5), (">=", [("c", 1), ("d", F(1, 7))], -3),
                                ("=", [("b", 1), ("c", -1), ("e", 2)], F(1, 5))])
    assert _check(p)


def test_grouping_names_what_stays_on_the_host_route():
    F = Fraction
    names = ["x", "y"]

    def prob(cons, **kw):
        return lp.Problem(type="max", vars=names, objective_var="w", objective_func=[("x", 1), ("y", 2)], constraints=cons, **kw)
    le = lambda b: ("<=", [("x", 1), ("y", F(1, 2))], b)
    ge = lambda b: (">=", [("x", 1), ("y", 3)], b)
    eq = lambda b: ("=", [("x", 2), ("y", 1)], b)
    ps = [prob([le(4), ge(1)]),                        # 0: one artificial row
          prob([le(5), ge(2)]),                        # 1: the same counts
          prob([le(4), ge(-1)]),                       # 2: the `>=` row flips: no artificial row
          prob([le(-4), ge(-1)]),                      # 3: both flip: one artificial row again
          prob([le(4), eq(1)]),                        # 4: an `=` row: one slack column fewer
          prob([le(4), eq(2)]),                        # 5
          prob([le(4), ge(0)]),                        # 6: a right-hand side of 0 does not flip
          prob([le(4), ge(1)], integer_vars=["x"]),    # 7
          prob([le(4.5), ge(1)]),                      # 8
          prob([], var_bounds=[("x", (0, 3)), ("y", (0, 3))]),      # 9
          prob([le(4), ge(1), eq(3)]),                 # 10: alone in its group
          prob([le(1 << 70), ge(1)])]                  # 11: beyond 64 bits
    host, groups = xl.group_lowered(ps)
    assert host == {2: "alone", 7: "integer variables", 8: "float", 9: "no constraints", 10: "alone", 11: "coefficient"}
    assert {key: [k for k, _ in members] for key, members in groups.items()} == \
        {(2, 2, 0, 1, True): [0, 1, 3, 6], (2, 2, 1, 1, True): [4, 5]}
    assert xl.lower_problem(ps[7]) is None and xl.lower_problem(ps[8]) is None and xl.lower_problem(ps[9]) is None
    with pytest.raises(lp.UnsupportedConstraintError) as e:
        xl.lower_problem(ps[11])
    assert tuple(e.value.constraint)[:2] == ("exact", "coefficient")
    with pytest.raises(ValueError):
        lp.solve_problems(ps[:2], device_build=True)


def _create(num, den, sense, m=None, ncv=None, min_bits=0):
    num, den = np.ascontiguousarray(num, dtype=np.int64), np.ascontiguousarray(den, dtype=np.int64)
    sense = np.ascontiguousarray(sense, dtype=np.int32)
    n = num.shape[0]
    m = num.shape[1] - 1 if m is None else m
    ncv = num.shape[2] - 1 if ncv is None else ncv
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = capi.lib().mi355x_xbatch_create_lps(ctypes.byref(hm), ctypes.byref(ha), n, m, ncv, p(num), p(den), p(sense), 0, min_bits)
    return rc, hm, ha


def test_argument_validation_without_device():
    num = np.array([[[1, 2, 3], [1, 1, 0]], [[2, 1, 4], [1, 1, 0]]], dtype=np.int64)
    den = np.ones_like(num)
    sense = np.zeros((2, 1), dtype=np.int32)

    def bad(num=num, den=den, sense=sense, what=b"", **kw):
        rc, hm, ha = _create(num, den, sense, **kw)
        assert rc == capi.MI_BAD_ARG and not hm.value and not ha.value
        assert what in capi.lib().mi355x_last_error()
    n2, d2 = num.copy(), den.copy()
    n2[1, 0, 1], d2[1, 0, 1] = 2, 4
    bad(num=n2, den=d2, what=b"member 1")                             # an unreduced fraction
    d2 = den.copy()
    d2[0, 1, 0] = 0
    bad(den=d2, what=b"member 0")                                     # den <= 0
    d2[0, 1, 0] = -1
    bad(den=d2, what=b"member 0")
    d2 = den.copy()
    d2[1, 1, 2] = 2
    bad(den=d2, what=b"member 1")                                     # zero as 0 / 2
    bad(sense=np.array([[0], [3]], dtype=np.int32), what=b"member 1")  # a sense of 3
    bad(sense=np.array([[0], [1]], dtype=np.int32), what=b"member 1")  # one artificial row against none
    bad(sense=np.array([[2], [1]], dtype=np.int32), what=b"member 1")  # the same artificial count, another `=` count
    n2 = num.copy()
    n2[1, 0, 2] = -4
    bad(num=n2, what=b"member 1")                                     # the flip makes member 1's row artificial
    bad(m=0)
    bad(ncv=0)
    bad(min_bits=32)
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.mi355x_xbatch_create_lps(None, ctypes.byref(h), 2, 1, 2, None, None, None, 0, 0) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_create_lps(ctypes.byref(h), ctypes.byref(h), 2, 1, 2, None, None, None, 0, 0) == capi.MI_BAD_ARG
    if capi.device_count() == 0:                                      # valid arguments: only now is a device looked at
        rc, hm, ha = _create(num, den, sense)
        assert rc == capi.MI_NO_DEVICE and not hm.value and not ha.value


def test_the_array_front_end_checks_its_operands():
    a = np.ones((2, 1, 2), dtype=np.int64)
    ok = dict(b=np.ones((2, 1), dtype=np.int64), c=np.ones((2, 2), dtype=np.int64), sense=np.zeros((2, 1), dtype=np.int32))
    for kw in (dict(ok, b=np.ones((2, 2), dtype=np.int64)), dict(ok, sense=np.full((2, 1), 3)), dict(ok, c=np.ones((2, 2))),
               dict(ok, b=(np.ones((2, 1), dtype=np.int64), np.zeros((2, 1), dtype=np.int64))), dict(ok, pivot_rule="steepest")):
        with pytest.raises(ValueError):
            xl.solve_lps_exact(a, **kw)
    n, d = xl._fractions((np.array([4, -6, 0, 3]), np.array([6, -4, -5, 1])), "x")
    assert n.tolist() == [2, 3, 0, 3] and d.tolist() == [3, 2, 1, 1]
