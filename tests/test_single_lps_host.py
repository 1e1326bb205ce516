"""Host side of the single-float batches built from problem rows (no GPU): the lowering feeds a plain-NumPy
restatement of rules (a)-(c) that must give the model's build-tableau bit for bit, the grouping with every reason
word, and mi355x_sbatch_create_lps's argument validation.

The reference is the float32 model of tests/single_cases.py; build_tableau_single is a second witness.

On the parent commit every test here fails: there is no single_lps module and no mi355x_sbatch_create_lps symbol."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_lps_cases as C
from tests.helpers import lp_amd

lp = lp_amd()
F32 = np.float32


def _all_groups():
    groups = [("sweep %dx%d" % key, g) for key, g in C.sweep_groups().items()]
    groups += [("moving", C.moving_group()), ("zero rhs", C.zero_rhs_group()), ("bounds", C.bounds_group()),
               ("main 32", C.ld_step_group(main_cols=32)), ("main 33", C.ld_step_group(main_cols=33)),
               ("art 64", C.ld_step_group(art_cols=64)), ("art 65", C.ld_step_group(art_cols=65)),
               ("outcomes", C.outcome_group()), ("driveout", C.driveout_group()), ("single phase", C.single_phase_group()),
               ("medium", C.medium_group()), ("medium min", C.medium_group("min")), ("extreme rows", C.extreme_rows_group()),
               ("96x300", C.big_group(False)), ("%dx300" % C.BIG_TWO_PHASE_M, C.big_group(True))]
    return groups


def _check_lowering(d, witness=True):
    """lower_problem_rows_single's arrays through the restated rules == the model's build, bit for bit."""
    p = C.to_problem(lp, d)
    low = lp.single_lps.lower_problem_rows_single(p)
    assert low.L.dtype == np.float32 and low.sense.dtype == np.int32 and low.col_int_sum.dtype == np.float64
    assert not low.float_zero and low.is_max == (d["type"] == "max")
    want = sc.build(d)
    M, basis, A, abasis = C.assemble_rows(low.L, low.sense, low.col_int_sum)
    assert sc.same_bits(M, want["main"][0]) and np.array_equal(basis, want["main"][1])
    assert (A is None) == (want["art"] is None)
    if A is not None:
        assert sc.same_bits(A, want["art"][0]) and np.array_equal(abasis, want["art"][1])
    assert {v: (mp[0], mp[1]) for v, mp in low.mapping.items()} == {v: (mp[0], mp[1]) for v, mp in want["mapping"].items()}
    if witness:
        tabs = lp.build_tableau_single(p)
        main = tabs[1] if isinstance(tabs, list) else tabs
        assert sc.same_bits(main.matrix, M) and np.array_equal(main.basis_columns, basis)
        assert main.var_mapping == low.mapping
        if A is not None:
            assert sc.same_bits(tabs[0].matrix, A) and np.array_equal(tabs[0].basis_columns, abasis)
    return low


def test_lowered_rows_through_the_restated_rules_equal_the_models_build():
    seen_ops, signs = set(), set()
    for name, group in _all_groups():
        for d in group:
            low = _check_lowering(d, witness="x300" not in name)
            flip = low.L[:-1, -1] < 0
            seen_ops |= {(int(s), bool(f)) for s, f in zip(low.sense, flip)}
            signs |= {bool(np.signbit(x)) for x in low.L[:-1, -1] if x == 0}
    assert seen_ops == {(s, f) for s in (0, 1, 2) for f in (False, True)}
    assert signs == {False, True}                            # right-hand sides 0 and -0.0: neither is flipped


def test_groups_are_groups_and_cover_the_shapes():
    for name, group in _all_groups():
        host, groups = lp.group_lowered_rows_single([C.to_problem(lp, d) for d in group])
        assert host == {} and len(groups) == 1, name
        (key, members), = groups.items()
        assert [k for k, _ in members] == list(range(len(group))), name
    assert {key[:2] for key in (next(iter(lp.group_lowered_rows_single([C.to_problem(lp, d) for d in g])[1]))
                                for g in C.sweep_groups().values())} == {(m, n) for m in range(1, 8) for n in range(1, 6)}
    # the members of the moving group differ in slack columns and in artificial ranks
    built = [sc.build(d) for d in C.moving_group()]
    assert len({tuple(b["main"][1]) for b in built}) == 4 and len({tuple(b["art"][1]) for b in built}) == 4
    assert len({tuple(np.flatnonzero(b["main"][0][:-1, 3:-1].any(axis=1))) for b in built}) > 1
    # the leading-dimension steps
    for kw, col in [(dict(main_cols=32), 32), (dict(main_cols=33), 33), (dict(art_cols=64), 64), (dict(art_cols=65), 65)]:
        b = sc.build(C.ld_step_group(**kw)[0])
        assert (b["art"] if "art_cols" in kw else b["main"])[0].shape[1] == col
    # the largest two-phase m x 300 inside the budget, and the first outside it
    m = C.BIG_TWO_PHASE_M
    b = sc.build(C.big_group(True)[0])
    assert b["art"][0].shape == (m + 1, 300 + 2 * m + 1) and C.fits(*b["art"][0].shape)
    assert C.lds_bytes(m + 1, 300 + 2 * m + 1) == 159456 and not C.fits(m + 2, 300 + 2 * (m + 1) + 1)
    assert sc.build(C.big_group(False)[0])["main"][0].shape == (97, 397) and C.fits(97, 397)
    # no member's rows exceed one trip of the 256-thread assembly: the budget ends at m = 196
    assert C.fits(197, 198) and not C.fits(198, 199)


def test_a_float_zero_in_a_negated_row_is_minus_zero_in_lisp():
    d = C.float_zero_member()
    want = sc.build(d)["main"][0][0]
    assert want.tolist() == [-1, 0, 0, -1, 0, 3] and np.signbit(want).tolist() == [True, True, False, True, False, False]
    low = lp.single_lps.lower_problem_rows_single(C.to_problem(lp, d))
    assert low.float_zero
    M = C.assemble_rows(low.L, low.sense, low.col_int_sum)[0]
    assert not np.signbit(M[0, 1])                           # what the device would write: the member stays on the host
    # an integer zero and a coefficient that is not mentioned do not mark a member
    for g in (C.zero_rhs_group(), C.moving_group()):
        assert not any(lp.single_lps.lower_problem_rows_single(C.to_problem(lp, x)).float_zero for x in g)
    # a float zero in a row that is NOT negated is harmless (and stays +0.0)
    d2 = dict(d, constraints=[("<=", [("x", 1), ("y", F32(0.0)), ("z", 0)], 3)] + d["constraints"][1:])
    assert not lp.single_lps.lower_problem_rows_single(C.to_problem(lp, d2)).float_zero
    _check_lowering(d2)


def test_extreme_rows_sums_depend_on_the_order_and_tiny_rows_are_negated_exactly():
    """Conditions on C.extreme_rows_group() (the model alone): the artificial objective row's entries in columns x and
    y are the increasing-row-order sums, every other order of the same three rows gives another float32, and the
    negated row holds the exact negatives of its subnormals."""
    import itertools
    wanted = [(F32(np.inf), F32(1)), (C.BIG, F32(1)), (C.BIG, F32(1 + 2.0 ** -23))]
    for d, (wx, wy) in zip(C.extreme_rows_group(), wanted):
        b = sc.build(d)
        A, M = b["art"][0], b["main"][0]
        assert A.shape == (6, 12) and M.shape == (6, 9) and sorted(np.where(b["main"][1] == 9)[0]) == [0, 1, 2]
        assert A[-1, 0] == wx and A[-1, 1] == wy
        for col, want in ((0, wx), (1, wy)):
            sums = set()
            with np.errstate(all="ignore"):
                for order in itertools.permutations(range(3)):
                    s = F32(0)
                    for r in order:
                        s = F32(s + A[r, col])
                    sums.add(float(s))
            assert float(want) in sums and len(sums) > 1
        assert A[:3, 0].tolist().count(C.BIG) == 2 and sorted(A[:3, 1].tolist()) == [2.0 ** -24, 2.0 ** -24, 1]
        # row 3: `>=` with a subnormal negative right-hand side -> `<=`, every entry the exact negative
        assert M[3, -1] == C.SUB and M[3, 2] == C.SUB and M[3, 3] == F32(3e-39) and M[3, 0] == 1
        assert 0 < M[3, -1] < np.finfo(F32).tiny and 0 < M[3, 3] < np.finfo(F32).tiny
        assert b["main"][1][3] < 8 and M[3, b["main"][1][3]] == 1               # a slack column: no artificial
        # row 4: -0.0 is not < 0: not flipped
        assert M[4, -1] == 0 and np.signbit(M[4, -1]) and M[4, :3].tolist() == [1, -1, 1.5]
    host, groups = lp.group_lowered_rows_single([C.to_problem(lp, d) for d in C.extreme_rows_group()])
    assert host == {} and len(groups) == 1                   # the guard accepts all three members
    wants = C.model_solution(C.extreme_rows_group)
    assert all(w["status"] == sc.INFEASIBLE and w["n"][0] >= 1 and not np.isfinite(w["A"][-1]).all() for w in wants)
    assert np.isnan(wants[0]["A"][-1, -1]) and len({w["n"] for w in wants}) == 2


def test_the_guard_integer_sums_beyond_2_to_24():
    d = C.integer_sum_member()
    low = lp.single_lps.lower_problem_rows_single(C.to_problem(lp, d))
    assert low.col_int_sum.tolist() == [2.0 ** 24 + 2, 4.0, 2.0 ** 24 + 2]
    assert C.assemble_rows(low.L, low.sense, low.col_int_sum) is None
    want = sc.build(d)["art"][0]
    assert want[-1, 0] == F32(16777218)
    running = C.assemble_rows(low.L, low.sense, low.col_int_sum, guard=False)[2]
    assert running[-1, 0] == F32(16777216)                   # what a float32 running sum makes of 2^24 + 1 + 1
    # floats with integer values are not counted: Lisp adds them as floats, as the device does
    d2 = dict(d, constraints=[("=", [("x", F32(2 ** 24)), ("y", 1)], F32(2 ** 24))] + d["constraints"][1:])
    low2 = _check_lowering(d2)
    assert low2.col_int_sum.tolist() == [2.0, 4.0, 2.0]


def test_grouping_of_a_mixed_list_reaches_every_reason():
    ds = [C.single_phase_group()[0],                         # 0
          C.float_zero_member(),                             # 1: "float zero"
          C.driveout_group()[0],                             # 2
          C.integer_sum_member(),                            # 3: "integer sum"
          C.single_phase_group()[1],                         # 4: with 0
          C.lone_member(),                                   # 5: "alone"
          C.declined_member(),                               # 6: a number no binary32 holds
          C.driveout_group()[1],                             # 7: with 2
          C.no_constraints_member(),                         # 8: "no constraints"
          dict(C.single_phase_group()[2], type="min")]       # 9: the other sense: "alone"
    ps = [C.to_problem(lp, d) for d in ds] + [C.to_problem(lp, C.single_phase_group()[2], integer_vars=["x"])]   # 10
    host, groups = lp.group_lowered_rows_single(ps)
    e = host.pop(6)
    assert isinstance(e, lp.UnsupportedConstraintError) and e.args[0] == ("single", 0.1)
    assert host == {1: "float zero", 3: "integer sum", 5: "alone", 8: "no constraints", 9: "alone", 10: "integer variables"}
    assert {key: [k for k, _ in v] for key, v in groups.items()} == {(3, 3, 0, 0, True): [0, 4], (2, 3, 1, 1, True): [2, 7]}
    low = groups[(2, 3, 1, 1, True)][1][1]
    assert isinstance(low, lp.single_lps.LoweredRowsSingle) and low.L.shape == (3, 4)
    assert lp.single_lps.lower_problem_rows_single(ps[8]) is None and lp.single_lps.lower_problem_rows_single(ps[10]) is None
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.single_lps.lower_problem_rows_single(ps[6])


def test_from_lps_and_solve_lps_single_check_their_arrays():
    L = np.zeros((2, 3, 4), dtype=np.float64)
    with pytest.raises(TypeError, match="float32"):
        lp.SingleBatch.from_lps(L, np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(ValueError):
        lp.SingleBatch.from_lps(L.astype(F32)[0], np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="sense"):
        lp.SingleBatch.from_lps(L.astype(F32), np.zeros((2, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="col_int_sum"):
        lp.SingleBatch.from_lps(L.astype(F32), np.zeros((2, 2), dtype=np.int32), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="int_mask"):
        lp.solve_lps_single(L.astype(F32), np.zeros((2, 2), dtype=np.int32), int_mask=np.zeros((2, 3, 3), dtype=bool))


def test_sbatch_create_lps_argument_validation_without_a_device():
    """MI_BAD_ARG comes before MI_NO_DEVICE, and the guard's MI_UNSUPPORTED before any device is looked for."""
    Lib, BAD = lp.capi.lib(), lp.capi.MI_BAD_ARG
    L = np.zeros((3, 3, 3), dtype=F32)                       # n = 3, m = 2, ncv = 2
    L[:, :2, -1] = 1
    s = np.array([[0, 1], [1, 0], [0, 1]], dtype=np.int32)
    sums = np.zeros((3, 3), dtype=np.float64)
    pL, ps, pc = (a.ctypes.data_as(ctypes.c_void_p) for a in (L, s, sums))
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    om, oa = ctypes.byref(hm), ctypes.byref(ha)
    create = Lib.mi355x_sbatch_create_lps
    assert create(None, oa, 3, 2, 2, pL, ps, pc, 0) == BAD and create(om, None, 3, 2, 2, pL, ps, pc, 0) == BAD
    assert create(om, oa, 3, 2, 2, None, ps, pc, 0) == BAD and b"lps" in Lib.mi355x_last_error()
    assert create(om, oa, 3, 2, 2, pL, None, pc, 0) == BAD and b"sense" in Lib.mi355x_last_error()
    assert create(om, oa, 0, 2, 2, pL, ps, pc, 0) == BAD
    assert create(om, oa, 3, 0, 2, pL, ps, pc, 0) == BAD
    assert create(om, oa, 3, 2, 0, pL, ps, pc, 0) == BAD
    s[1, 1] = 3
    assert create(om, oa, 3, 2, 2, pL, ps, pc, 0) == BAD
    assert b"member 1" in Lib.mi355x_last_error() and b"sense 3" in Lib.mi355x_last_error()
    s[1, 1] = 0
    s[2] = [0, 0]                                            # no artificial row where the others have one
    assert create(om, oa, 3, 2, 2, pL, ps, pc, 0) == BAD and b"member 2" in Lib.mi355x_last_error()
    s[2] = [2, 0]                                            # one artificial row, but an `=` row
    assert create(om, oa, 3, 2, 2, pL, ps, pc, 0) == BAD and b"member 2" in Lib.mi355x_last_error()
    s[2] = [0, 0]
    L[2, 1, -1] = -1                                         # the flip makes the second row `>=`: the counts agree again
    sums[1, 2] = 2.0 ** 24 + 2
    assert create(om, oa, 3, 2, 2, pL, ps, pc, 0) == lp.capi.MI_UNSUPPORTED
    assert b"member 1" in Lib.mi355x_last_error() and not hm.value and not ha.value
    sums[1, 2] = 2.0 ** 24
    if lp.capi.device_count() == 0:
        assert create(om, oa, 3, 2, 2, pL, ps, pc, 0) == lp.capi.MI_NO_DEVICE and not hm.value and not ha.value
        assert create(om, oa, 3, 2, 2, pL, ps, None, 0) == lp.capi.MI_NO_DEVICE
    else:
        assert create(om, oa, 3, 2, 2, pL, ps, pc, 1 << 20) == BAD and not hm.value and not ha.value
    assert Lib.mi355x_sbatch_debug_stored(None, 0, None, None) == BAD
