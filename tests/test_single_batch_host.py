"""Host side of the single-float batch route (no GPU): how group_single_problems sorts a mixed list, the argument
clashes of mi355x_solve_problems(..., precision="single"), and mi355x_sbatch_create's argument validation.

On the parent commit every test here fails: single.group_single_problems and the mi355x_sbatch_* symbols do not exist,
and mi355x_solve_problems has no `precision` parameter (a TypeError)."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests.helpers import lp_amd

lp = lp_amd()
F32 = np.float32


def _lp_problem(d, integer_vars=()):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[(b[0], (b[1], b[2])) for b in d["bounds"]],
                      constraints=list(d["constraints"]), integer_vars=list(integer_vars))


def _max2(c, rhs):
    """max c0 x + c1 y  s.t. x + 2 y <= rhs0, 3 x + y <= rhs1: a 3 x 5 single-phase tableau."""
    return dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", c[0]), ("y", c[1])], bounds=[],
                constraints=[("<=", [("x", 1), ("y", 2)], rhs[0]), ("<=", [("x", 3), ("y", 1)], rhs[1])])


def _max3(c):
    """three variables, one row: a 2 x 5 tableau."""
    return dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", c), ("y", 1), ("z", 1)], bounds=[],
                constraints=[("<=", [("x", 1), ("y", 1), ("z", 1)], F32(2.5))])


def test_group_single_problems_on_a_mixed_list():
    no_float32 = 0.1                                         # a double that no binary32 holds
    assert float(F32(no_float32)) != no_float32
    ds = [_max2((1, F32(0.5)), (4, F32(6.5))),               # 0: 3 x 5, max
          sc.DRIVEOUT_LP,                                    # 1: two-phase
          _max2((F32(2.5), 1), (5, 7)),                      # 2: 3 x 5, max -- with 0
          _max3(F32(1.5)),                                   # 3: 2 x 5, alone in its shape
          _max2((1, no_float32), (4, 6)),                    # 4: declined
          sc.DRIVEOUT_LP,                                    # 5: two-phase -- with 1
          dict(_max2((1, 2), (4, 6)), type="min")]           # 6: 3 x 5, min: a group of its own
    ps = [_lp_problem(d) for d in ds] + [_lp_problem(_max2((1, 1), (4, 6)), integer_vars=["x"])]   # 7: integer
    slots, groups, groups2 = lp.single.group_single_problems(ps, 1024, 0)
    assert [k for k, s in enumerate(slots) if s is None] == [0, 1, 2, 3, 5, 6]
    assert slots[7] == "alone"
    e = slots[4]
    assert isinstance(e, lp.UnsupportedConstraintError) and e.args[0] == ("single", no_float32)
    assert {key: [k for k, _ in v] for key, v in groups.items()} == \
        {((3, 5), True): [0, 2], ((2, 5), True): [3], ((3, 5), False): [6]}
    built = sc.build(sc.DRIVEOUT_LP)
    ashape, mshape = built["art"][0].shape, built["main"][0].shape
    assert {key: [k for k, _, _ in v] for key, v in groups2.items()} == {(ashape, mshape, True): [1, 5]}
    # the members carry what build_tableau_single builds, bit for bit the model's
    for _, t in groups[((3, 5), True)]:
        assert isinstance(t, lp.SingleTableau) and t.matrix.dtype == np.float32
    assert sc.same_bits(groups[((3, 5), True)][0][1].matrix, sc.build(ds[0])["main"][0])
    _, art, main = groups2[(ashape, mshape, True)][1]
    assert sc.same_bits(art.matrix, built["art"][0]) and sc.same_bits(main.matrix, built["main"][0])
    assert np.array_equal(art.basis_columns, built["art"][1])


@pytest.mark.parametrize("kw", [dict(exact=True), dict(native="many"), dict(from_rows=True),
                                dict(device_build=True), dict(devices=2), dict(pivot_rule="bland")])
def test_single_precision_argument_clashes(kw):
    ps = [_lp_problem(_max2((1, 1), (4, 6)))] * 2
    with pytest.raises(ValueError, match="single"):
        lp.solve_problems(ps, precision="single", **kw)


def test_unknown_precision_is_an_argument_error():
    with pytest.raises(ValueError, match="precision"):
        lp.solve_problems([_lp_problem(_max2((1, 1), (4, 6)))], precision="half")


def test_sbatch_create_argument_validation_without_a_device():
    """MI_BAD_ARG comes before MI_NO_DEVICE, as for mi355x_stab_create."""
    L = lp.capi.lib()
    M = np.zeros((2, 3, 4), dtype=F32)
    b = np.zeros((2, 2), dtype=np.int64)
    pm, pb = M.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    bad = lp.capi.MI_BAD_ARG
    assert L.mi355x_sbatch_create(None, 2, 3, 4, pm, pb, 0) == bad
    assert L.mi355x_sbatch_create(ctypes.byref(h), 2, 3, 4, None, pb, 0) == bad and not h.value
    assert L.mi355x_sbatch_create(ctypes.byref(h), 0, 3, 4, pm, pb, 0) == bad
    assert L.mi355x_sbatch_create(ctypes.byref(h), 2, 0, 4, pm, pb, 0) == bad
    assert L.mi355x_sbatch_create(ctypes.byref(h), 2, 3, 0, pm, pb, 0) == bad
    assert L.mi355x_sbatch_create(ctypes.byref(h), 2, 3, 4, pm, None, 0) == bad and not h.value
    assert b"basis" in L.mi355x_last_error()
    if lp.capi.device_count() == 0:
        assert L.mi355x_sbatch_create(ctypes.byref(h), 2, 3, 4, pm, pb, 0) == lp.capi.MI_NO_DEVICE and not h.value
    else:
        assert L.mi355x_sbatch_create(ctypes.byref(h), 2, 3, 4, pm, pb, 1 << 20) == bad and not h.value
    assert L.mi355x_sbatch_solve(None, 1, 1024.0, 0, None, None) == bad
    assert L.mi355x_sbatch_solve_two_phase(None, None, 1, 1024.0, 0, None, None) == bad
    assert L.mi355x_sbatch_download(None, 0, None, None, None, None) == bad
    assert L.mi355x_sbatch_trace(None, 0, None, None, 0, None) == bad
    assert L.mi355x_sbatch_info(None, None, None, None, None, None, None, None) == bad
    assert L.mi355x_sbatch_cancel(None) == bad
    L.mi355x_sbatch_destroy(None)                            # no-op
    assert L.mi355x_tune_set_sbatch_threads(512) == bad and L.mi355x_tune_set_sbatch_threads(0) == 0
    assert L.mi355x_tune_set_sbatch_launch_cap(-1) == bad and L.mi355x_tune_set_sbatch_launch_cap(0) == 0
