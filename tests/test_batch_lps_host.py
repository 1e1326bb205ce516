"""Host side of the device-built double-precision batches (linear-programming_amd/batch_lps.py): the lowering of a
problem to its rows and the numpy statement of the assembly kernels (tests/lps_cases.assemble) together give
build_tableau bit for bit; the grouping; the C ABI's argument checks (made before a device is looked for); the
argument errors of from_rows.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import lps_cases as lc
from tests.helpers import lp_amd

lp = lp_amd()
SEEDS = range(320)


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed in SEEDS:
        p, kinds = lc.problem(lp, seed)
        out.append((seed, p, kinds, lp.lower_problem_rows(p), lc.host_tableaux(lp, p)))
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(lc.bits(a), lc.bits(b))


def test_lowering_and_assembly_give_build_tableau_bit_for_bit(cases):
    assert len(cases) >= 300
    for seed, p, _, low, (M, basis, A, abasis, mapping) in cases:
        assert low is not None, seed
        L, sense, low_mapping, is_max = low
        assert L.dtype == np.float64 and sense.dtype == np.int32 and is_max == (p.type == "max")
        m2, b2, a2, ab2 = lc.assemble(L, sense)
        assert same_bits(m2, M), seed
        assert np.array_equal(b2, basis), seed
        assert (a2 is None) == (A is None), seed
        if A is not None:
            assert same_bits(a2, A), seed
            assert np.array_equal(ab2, abasis), seed
        assert low_mapping == mapping and list(low_mapping) == list(mapping), seed
        assert all(type(x) is type(y) for v in mapping for x, y in zip(low_mapping[v], mapping[v])), seed


def test_the_set_covers_what_it_claims(cases):
    two_phase = sum(1 for c in cases if c[4][2] is not None)
    assert 50 <= two_phase <= len(cases) - 50, two_phase
    seen = set()
    for c in cases:
        seen |= c[2]
    assert seen == set(lc.KINDS)

    def negative_zero_in_slack(c):
        M, ncv = c[4][0], c[3].L.shape[1] - 1
        slack = M[:-1, ncv:-1]
        return bool((np.signbit(slack) & (slack == 0)).any())
    assert sum(1 for c in cases if negative_zero_in_slack(c)) >= 20
    # a zero coefficient in a negated row: -0.0 among the structural entries
    assert any((np.signbit(c[4][0][:-1, :c[3].L.shape[1] - 1]) & (c[4][0][:-1, :c[3].L.shape[1] - 1] == 0)).any() for c in cases)
    # a right-hand side that is negative only through an offset, a non-zero objective constant, every sense
    def rhs_negative_through_offset(c):
        p, L = c[1], c[3].L
        n_bound_rows = L.shape[0] - 1 - len(p.constraints)
        return any(float(rhs) >= 0 and L[n_bound_rows + i, -1] < 0 for i, (_, _, rhs) in enumerate(p.constraints))
    assert sum(1 for c in cases if rhs_negative_through_offset(c)) >= 10
    assert sum(1 for c in cases if c[3].L[-1, -1] != 0) >= 50
    assert {int(s) for c in cases for s in c[3].sense} == {0, 1, 2}


def test_what_is_not_lowered():
    x = lp.Problem(type="max", vars=["x"], objective_var="w", objective_func=[("x", 1)], constraints=[("<=", [("x", 1)], 4)])
    assert lp.lower_problem_rows(x) is not None
    assert lp.lower_problem_rows(lp.Problem(type="max", vars=["x"], objective_func=[("x", 1)], integer_vars=["x"],
                                            constraints=[("<=", [("x", 1)], 4)])) is None
    assert lp.lower_problem_rows(lp.Problem(type="max", vars=["x"], objective_func=[("x", 1)],
                                            var_bounds=[("x", (0, 3))])) is None
    assert lp.lower_problem_rows(lp.Problem(type="max", vars=["x"], objective_func=[("x", 1)],
                                            constraints=[("<", [("x", 1)], 4)])) is None


def test_a_repeated_variable_is_assigned_not_accumulated():
    p = lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1), ("y", 1)],
                   var_bounds=[("x", (2, None))],
                   constraints=[("<=", [("x", 1), ("y", 1), ("x", 3)], 10)])
    L = lp.lower_problem_rows(p).L
    assert L[0].tolist() == [3.0, 1.0, 10.0 - 1.0 * 2.0 - 3.0 * 2.0]
    assert same_bits(lc.assemble(L, [0])[0], lp.build_tableau(p)._matrix)


def test_grouping():
    def P(ops, rhs, kind="max", n=2, **kw):
        names = ["x%d" % i for i in range(n)]
        return lp.Problem(type=kind, vars=names, objective_var="w", objective_func=[(v, 1) for v in names],
                          constraints=[(op, [(v, 1) for v in names], r) for op, r in zip(ops, rhs)], **kw)
    ps = [P(["<=", ">="], [4, 1]),                       # 0  (2, 2, 0, 1, max)
          P(["<=", "<="], [4, 5]),                       # 1  (2, 2, 0, 0, max)
          P([">=", "<="], [-4, -1]),                     # 2  negated: `<=`, `>=` -> with 0
          P(["<=", "<="], [1, 2]),                       # 3  with 1
          P(["<=", "<="], [1, 2], kind="min"),           # 4  alone: the sense
          P(["<=", "="], [4, 1]),                        # 5  alone: an `=` row
          P(["<=", ">="], [4, -1]),                      # 6  single phase with a negated row: "basis"
          P(["<=", "<="], [4, 5], integer_vars=["x0"]),  # 7
          P([], []),                                     # 8
          P(["<=", ">="], [4, 1], n=3),                  # 9  alone: ncv
          P([">="], [-1]),                               # 10 one row, negated: its own slack only -> a group with 11
          P(["<="], [3])]                                # 11
    host, groups = lp.group_lowered_rows(ps)
    assert host == {4: "alone", 5: "alone", 6: "basis", 7: "integer variables", 8: "no constraints", 9: "alone"}
    assert {key: [k for k, _ in members] for key, members in groups.items()} == \
        {(2, 2, 0, 1, True): [0, 2], (2, 2, 0, 0, True): [1, 3], (1, 2, 0, 0, True): [10, 11]}
    # what "basis" mirrors: the default route's unit-basis-p declines exactly these single-phase members
    from importlib import import_module
    unit = import_module("linear-programming_amd.simplex")._unit_basis
    assert not unit(lp.build_tableau(ps[6])) and unit(lp.build_tableau(ps[10])) and unit(lp.build_tableau(ps[1]))


def _create(fn, multi, n, m, ncv, L, S, outs=True):
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    args = [ctypes.byref(hm) if outs else None, ctypes.byref(ha), n, m, ncv, ptr(L), ptr(S)] + ([1, None] if multi else [0])
    rc = fn(*args)
    assert not hm.value and not ha.value
    return rc, lp.capi.lib().mi355x_last_error().decode()


@pytest.mark.parametrize("multi", [False, True])
def test_argument_errors_come_before_the_device(multi):
    L_ = lp.capi.lib()
    fn = L_.mi355x_multibatch_create_lps if multi else L_.mi355x_batch_create_lps
    L = np.zeros((3, 3, 3))
    L[:, :2, :2] = 1.0
    L[:, :2, 2] = 1.0
    S = np.zeros((3, 2), dtype=np.int32)
    BAD = lp.capi.MI_BAD_ARG
    assert _create(fn, multi, 3, 2, 2, L, S, outs=False) == (BAD, "out is NULL")
    assert _create(fn, multi, 3, 2, 2, None, S) == (BAD, "lps is NULL")
    assert _create(fn, multi, 3, 2, 2, L, None) == (BAD, "sense is NULL")
    assert _create(fn, multi, 0, 2, 2, L, S) == (BAD, "n_lps=0 must be >= 1")
    assert _create(fn, multi, 3, 0, 2, L, S) == (BAD, "m=0 ncv=2 must be >= 1")
    assert _create(fn, multi, 3, 2, 0, L, S) == (BAD, "m=2 ncv=0 must be >= 1")
    S2 = S.copy()
    S2[2, 1] = 3
    assert _create(fn, multi, 3, 2, 2, L, S2) == (BAD, "member 2: sense 3 of row 1")
    S2[2, 1] = -1
    assert _create(fn, multi, 3, 2, 2, L, S2) == (BAD, "member 2: sense -1 of row 1")
    S2[2, 1] = 2                                          # an `=` row in member 2 only
    assert _create(fn, multi, 3, 2, 2, L, S2) == \
        (BAD, "member 2 has 1 `=` and 1 artificial rows, the members before it 0 and 0")
    L2 = L.copy()
    L2[1, 0, 2] = -1.0                                    # member 1: `<=` with a negative right-hand side -> artificial
    assert _create(fn, multi, 3, 2, 2, L2, S) == \
        (BAD, "member 1 has 0 `=` and 1 artificial rows, the members before it 0 and 0")
    L2[1, 0, 2] = -0.0                                    # -0.0 and NaN are not negative: the members agree, and only
    L2[2, 1, 2] = np.nan                                  # now is a device looked for
    if lp.capi.device_count() == 0:
        rc, msg = _create(fn, multi, 3, 2, 2, L2, S)
        assert rc == lp.capi.MI_NO_DEVICE and "no HIP device" in msg


def test_readback_argument_errors():
    L_ = lp.capi.lib()
    assert L_.mi355x_batch_readback(None, None, None, None) == lp.capi.MI_BAD_ARG
    assert L_.mi355x_last_error().decode() == "batch is NULL"
    assert L_.mi355x_multibatch_readback(None, None, None, None) == lp.capi.MI_BAD_ARG
    assert L_.mi355x_last_error().decode() == "handle is NULL"


def test_from_rows_argument_errors():
    p = lp.Problem(type="max", vars=["x"], objective_var="w", objective_func=[("x", 1)], constraints=[("<=", [("x", 1)], 4)])
    with pytest.raises(ValueError, match="device_build"):
        lp.mi355x_solve_problems([p, p], exact=True, from_rows=True)
    with pytest.raises(ValueError, match="many"):
        lp.mi355x_solve_problems([p, p], native="many", from_rows=True)
    with pytest.raises(ValueError, match="needs exact=True"):
        lp.mi355x_solve_problems([p, p], device_build=True, from_rows=True)
    with pytest.raises(ValueError):
        lp.MultiDeviceBatch.from_lps(np.zeros((2, 3, 3)), np.zeros((2, 3), dtype=np.int32), n_devices=1)
