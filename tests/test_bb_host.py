"""Branch-and-bound without a GPU: the oracle search (tests/bb_oracle.py, a literal restatement of
src/simplex.lisp:462-542) reproduces the reference's integer answers (tests/golden/
reference_ilp_cases.json) on the double-float path and on exact rationals, and the library's
branch-and-bound entry points validate their arguments and refuse to run without a device."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import bb_oracle as B
from tests.helpers import lp_amd

lp = lp_amd()
CASES = B.load_cases()


def _expected_ok(name, status, best):
    exp = CASES[name]["expected"]
    if exp["status"] == "infeasible":
        assert status == B.INFEASIBLE and best is None
        return
    assert status == B.OPTIMAL
    obj, vals = best
    if "objective" in exp:
        assert obj == Fraction(exp["objective"])
    for v, x in exp["variables"].items():
        assert vals[v] == Fraction(x), (name, v, vals[v])


@pytest.mark.parametrize("name", sorted(CASES))
def test_f64_oracle_reproduces_the_reference_answers(name):
    status, best, trace = B.branch_and_bound(B.problem_of(CASES[name]["problem"]))
    _expected_ok(name, status, best)
    assert trace[0][0] == -1 and trace[0][1] is None                 # the root entry ()


@pytest.mark.parametrize("name", sorted(CASES))
def test_rational_oracle_through_the_same_search_gives_the_same_answers(name):
    status, best, trace = B.branch_and_bound(B.problem_of(CASES[name]["problem"], exact=True), exact=True)
    _expected_ok(name, status, best)
    f_status, f_best, f_trace = B.branch_and_bound(B.problem_of(CASES[name]["problem"]))
    assert status == f_status and len(trace) == len(f_trace)
    assert [r[:3] + (r[4],) for r in trace] == [r[:3] + (r[4],) for r in f_trace]


def test_rock_of_gibraltar_reduced_costs_are_zero():
    """t/solver.lisp:50-55: solution-reduced-cost of x and y is 0 in the incumbent."""
    p = B.problem_of(CASES["rock_of_gibraltar_max"]["problem"])
    status, best, trace = B.branch_and_bound(p)
    assert status == B.OPTIMAL and best[1] == {"x": 3.0, "y": 1.0}
    assert [r[4] for r in trace].count(B.BB_INCUMBENT) >= 1


def test_random_cases_are_deterministic_and_search_trees():
    cases = B.random_cases(count=12)
    again = B.random_cases(count=12)
    assert [s for s, _, _ in cases] == [s for s, _, _ in again]
    assert [B.trace_key(r[2]) for _, _, r in cases] == [B.trace_key(r[2]) for _, _, r in again]
    assert any(len(r[2]) >= 5 for _, _, r in cases)


def test_int_tolerance_changes_only_what_counts_as_integral():
    p = lp.Problem(type="max", vars=["x", "y"], objective_func=[("x", 1.0), ("y", 0.0)], integer_vars=["x"],
                   constraints=[("<=", [("x", 0.1)], 0.3), ("<=", [("y", 1.0)], 1.0)])
    st0, _, tr0 = B.branch_and_bound(p)
    st1, best1, tr1 = B.branch_and_bound(p, int_tolerance=1024)
    assert tr0[0][4] == B.BB_BRANCHED and tr0[0][5] == tr1[0][5] == 0.1 * 0 + 0.3 / 0.1
    assert st1 == B.OPTIMAL and tr1 == [(-1, None, 0, 0.0, B.BB_INCUMBENT, 0.3 / 0.1)]
    assert best1[1]["x"] == 0.3 / 0.1                                   # the raw tableau value is reported


def _begin(L, prob, order=(0,), f=1024.0, tol=0.0, width=4, n_dev=1, ids=None):
    arr = np.asarray(order, dtype=np.int64)
    h = ctypes.c_void_p()
    rc = L.mi355x_simplex_solver_bb_begin(prob, arr.ctypes.data_as(ctypes.c_void_p) if len(arr) else None,
                                          len(arr), f, tol, width, n_dev, ids, ctypes.byref(h))
    return rc, h


def test_bb_entry_points_validate_their_arguments():
    L = lp.capi.lib()
    np_ = lp.native.NativeProblem(B.problem_of(CASES["rock_of_gibraltar_max"]["problem"]))
    BAD = lp.capi.MI_BAD_ARG
    assert _begin(L, None)[0] == BAD
    assert _begin(L, np_._h, order=(2,))[0] == BAD                     # only x, y exist
    assert _begin(L, np_._h, order=(-1,))[0] == BAD
    assert _begin(L, np_._h, width=0)[0] == BAD
    assert _begin(L, np_._h, n_dev=0)[0] == BAD
    assert _begin(L, np_._h, f=-1.0)[0] == BAD
    assert _begin(L, np_._h, tol=-1.0)[0] == BAD
    assert _begin(L, np_._h, tol=float("nan"))[0] == BAD
    assert _begin(L, np_._h, tol=float("inf"))[0] == BAD
    assert L.mi355x_simplex_solver_bb_begin(np_._h, None, 1, 1024.0, 0.0, 4, 1, None, None) == BAD
    n = ctypes.c_int64(7)
    assert L.mi355x_simplex_solver_bb_step(None, 0, ctypes.byref(n)) == BAD and n.value == 0
    assert L.mi355x_simplex_solver_bb_cancel(None) == BAD
    s = ctypes.c_void_p()
    assert L.mi355x_simplex_solver_bb_finish(None, ctypes.byref(s)) == BAD and not s.value
    assert L.mi355x_simplex_solver_bb_stats(None, None, None, None) == BAD
    assert L.mi355x_simplex_solver_bb_trace(None, None, None, None, None, None, None, 0, None) == BAD
    L.mi355x_simplex_solver_bb_abandon(None)                          # no-op


@pytest.mark.skipif(lp.capi.device_count() > 0, reason="a GPU is present")
def test_bb_without_a_device_is_a_loud_failure():
    L = lp.capi.lib()
    prob = B.problem_of(CASES["rock_of_gibraltar_max"]["problem"])
    np_ = lp.native.NativeProblem(prob)
    rc, h = _begin(L, np_._h, order=(0, 1))
    assert rc == lp.capi.MI_NO_DEVICE and not h.value
    with pytest.raises(lp.capi.Mi355xError):
        lp.solve_problem(prob, branch_and_bound=True)
    # the default is unchanged: integer problems are declined
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problem(prob)


# ---- the reference of the node-assembly tests (tests/test_gpu_bb_assembly.py), pinned without a GPU ----------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", B.ASSEMBLY_CASES)
def test_host_build_tableau_equals_the_restatement_at_the_assembly_shapes(name):
    """mi355x_build_tableau of every node problem against the plain-Python restatement of the header comment
    of linear-programming_amd/csrc/kernels_bb.inc: row placement, slack and artificial columns, the negation rule,
    the artificial objective row -- bit for bit, -0.0 included."""
    p, nodes = B.assembly_case(name)
    for entry, (hm, hb, ha, hab) in zip(nodes, B.host_node_tableaux(name)):
        M, basis, A, abasis = B.restated_node_tableaux(p, entry)
        assert np.array_equal(_bits(hm), _bits(M)) and hb.tolist() == basis, (name, entry[:3])
        assert (ha is None) == (A is None)
        if A is not None:
            assert np.array_equal(_bits(ha), _bits(A)) and hab.tolist() == abasis, (name, entry[:3])


def _artificial_rows(name):
    """Per node of the case: the rows whose main-basis entry is the number of columns."""
    return [np.nonzero(hb == hm.shape[1])[0] for hm, hb, _, _ in B.host_node_tableaux(name)]


def test_assembly_cases_reach_the_shapes_they_are_made_for():
    # tall: past one workgroup of k_bb_rows (256 rows) and past k_assemble's row grid (1024), with
    # artificial and negated rows in every range
    for name, edges in (("tall_300", (0, 256, 512)), ("tall_1030", (0, 256, 512, 1024, 2048))):
        p, nodes = B.assembly_case(name)
        for (hm, hb, ha, hab), art in zip(B.host_node_tableaux(name), _artificial_rows(name)):
            assert hm.shape[0] - 1 > edges[-2] and ha is not None
            for lo, hi in zip(edges, edges[1:]):
                assert ((art >= lo) & (art < hi)).any(), (name, lo)
                assert (np.signbit(hm[lo:hi]) & (hm[lo:hi] == 0))[:, :6].any(), (name, lo)   # a negated row
            # (artificial columns dealt in decreasing row order: the lowest artificial row holds the last one)
            assert hab[art[0]] == ha.shape[1] - 2 and hab[art[-1]] == hm.shape[1] - 1
    assert B.host_node_tableaux("tall_1030")[0][0].shape[0] - 1 > 1024
    # wide: main past k_assemble's column grid (16 * 256 entries of a padded row); main inside it and the
    # artificial tableau past it, for any row padding up to 256 entries
    for hm, _, ha, _ in B.host_node_tableaux("wide_main"):
        assert hm.shape[1] > 4096 and ha.shape[1] > hm.shape[1]
    for hm, _, ha, _ in B.host_node_tableaux("wide_art"):
        assert hm.shape[1] + 256 <= 4096 < ha.shape[1]
    # deep: depth 40, variables met several times in both senses, negated base rows
    p, nodes = B.assembly_case("deep")
    for entry, (hm, hb, _, _) in zip(nodes, B.host_node_tableaux("deep")):
        assert len(entry) == 40
        senses = {}
        for v, s, _ in entry:
            senses.setdefault(v, []).append(s)
        assert sum(len(s) >= 3 and len(set(s)) == 2 for s in senses.values()) >= 3
        negated = (np.signbit(hm[:-1]) & (hm[:-1] == 0)).any(axis=1)    # rows that carry -0.0
        assert negated[2 + 40:].sum() >= 2 and negated[2:2 + 40].any() and not negated[2:2 + 40].all()


def test_shifted_nodes_round_and_keep_signed_zeros():
    """The right-hand side of a node row is bound - 1.0 * offset: some round, bound = offset gives +0.0 and
    no flip, a bound of -0.0 stays -0.0 where the offset is zero (the free variable included) and is not a
    negative right-hand side."""
    from fractions import Fraction
    p, nodes = B.assembly_case("shifted")
    offset = {"v0": 0.0, "v1": 0.1, "v2": 0.3, "v3": 0.7, "v4": 0.0, "v5": 1.0 / 3.0}
    nb = 1                                                               # v2's bound row
    seen = {"rounds": 0, "plus_zero": 0, "minus_zero": set(), "flipped_zero_bound": 0}
    for entry, (hm, hb, _, _) in zip(nodes, B.host_node_tableaux("shifted")):
        ncols = hm.shape[1]
        for k, (v, s, b) in enumerate(entry):
            rhs = b - 1.0 * offset[v] if v != "v4" else b
            row = hm[nb + k]
            flipped = rhs < 0.0
            assert _bits(row[-1:])[0] == _bits(np.array([-rhs if flipped else rhs]))[0]
            slack = row[7 + nb + k]                                      # 7 structural columns (v4: two)
            assert slack == (1.0 if (s == 0) != flipped else -1.0)
            assert (hb[nb + k] == ncols) == ((s == 1) != flipped)
            if Fraction(b) - Fraction(offset[v]) != Fraction(rhs):
                seen["rounds"] += 1
            if b == offset[v] and not np.signbit(b):
                assert rhs == 0.0 and not np.signbit(rhs) and not flipped
                seen["plus_zero"] += 1
            if b == 0.0 and np.signbit(b):
                if offset[v] == 0.0:
                    assert np.signbit(row[-1]) and row[-1] == 0.0 and not flipped
                    seen["minus_zero"].add(v)
                else:
                    seen["flipped_zero_bound"] += flipped
    assert seen["rounds"] >= 6 and seen["plus_zero"] >= 12 and seen["minus_zero"] == {"v0", "v4"}
    assert seen["flipped_zero_bound"] >= 6
    kinds = {v: lp.native.NativeProblem(p).var_mapping(v)[0] for v in p.vars}
    assert kinds == {"v0": "positive", "v1": "positive", "v2": "positive", "v3": "negative", "v4": "signed",
                     "v5": "positive"}


def test_artificial_objective_of_the_inexact_case_depends_on_the_order_of_its_sum():
    """The precondition of the device test (tests/bb_oracle.py: assert_sum_order_sensitive), without a GPU."""
    B.assert_sum_order_sensitive("inexact")
