"""Single-float branch-and-bound without a GPU: the host statement of the device assembly against the model's
build-tableau of the node problem, the guard of the artificial objective row, the parameterised search, and the
keyword behaviour of the public call."""
import numpy as np
import pytest

from tests import single_bb_cases as C
from tests import single_cases as sc
from tests.helpers import lp_amd

lp = lp_amd()
sbb = lp.single_bb
F32 = np.float32


def _same_node(g, d, entry):
    M, basis, A, abasis = sbb.node_tableaux_single(g, entry)
    wM, wb, wA, wab = C.build_node(d, entry)
    assert sc.same_bits(M, wM) and np.array_equal(basis, wb)
    assert (A is None) == (wA is None)
    if A is not None:
        assert sc.same_bits(A, wA) and np.array_equal(abasis, wab)
    return M, A


@pytest.mark.parametrize("depth,art_bound,n_ge,n_eq", [(1, False, 0, 0), (2, False, 1, 0), (3, True, 1, 1), (2, True, 0, 0),
                                                       (3, False, 2, 1)])
def test_node_tableaux_equal_the_models_build_bit_for_bit(depth, art_bound, n_ge, n_eq):
    d = C.assembly_base(24 + depth, depth, art_bound, n_ge, n_eq, seed=depth)
    g = sbb.GeneralFormSingle(C.to_problem(lp, d))
    seen_art, seen_flip, seen_kinds = set(), set(), set()
    for want in range(0, min(depth, 3 - min(3, int(art_bound) + n_ge + n_eq)) + 1):
        for entry in C.assembly_nodes(10 * depth + want, depth, 12, want):
            assert g.device_ok(entry)
            M, A = _same_node(g, d, entry)
            n_art = 0 if A is None else A.shape[1] - M.shape[1]
            assert n_art == int(art_bound) + n_ge + n_eq + want
            assert sum(g.row_artificial(*r) for r in entry) == want
            seen_art.add(n_art)
            for var, sense, bound in entry:
                seen_flip.add(bound - C._OFFSET[var] < 0)
                seen_kinds.add(g.kind[g.index[var]])
            # a node row, flipped or not, holds +0.0 outside its own entries (fact a)
            rows = M[g.nb:g.nb + depth]
            assert not np.signbit(rows[rows == 0]).any()
    assert seen_flip == {False, True} and seen_kinds == {0, 1, 2}
    assert seen_art <= {0, 1, 2, 3} and len(seen_art) >= 1


def test_every_number_of_artificial_rows_from_0_to_3_is_covered():
    got = set()
    for depth, art_bound, n_ge, n_eq in [(1, False, 0, 0), (2, False, 1, 0), (3, True, 1, 1), (2, True, 0, 0)]:
        d = C.assembly_base(24 + depth, depth, art_bound, n_ge, n_eq, seed=depth)
        g = sbb.GeneralFormSingle(C.to_problem(lp, d))
        for want in range(depth + 1):
            entry = C.assembly_nodes(want, depth, 1, want)[0]
            _, A = _same_node(g, d, entry)
            got.add(0 if A is None else g.n_art + want)
    assert {0, 1, 2, 3} <= got


def test_inserted_columns_of_a_negated_base_row_are_plus_zero():
    d = C.assembly_base(26, 2, n_ge=1, seed=5)
    g = sbb.GeneralFormSingle(C.to_problem(lp, d))
    # the base row 2 v1 + v0 >= 3 was negated: its v1 entry is -2 and its right-hand side +2
    r = next(r for r in range(g.matrix.shape[0] - 1) if g.matrix[r, g.col[1]] == -2 and g.matrix[r, -1] == 2)
    entry = C.assembly_nodes(1, 2, 1)[0]
    M, A = _same_node(g, d, entry)
    at = g.ncv + g.nb
    for T in (M, A):
        inserted = T[r + 2, at:at + 2]
        assert (inserted == 0).all() and not np.signbit(inserted).any()
    # (a float row negated whole would carry -0.0 there)
    assert np.signbit(-np.zeros(2, dtype=F32)).all()


def test_guard_refuses_an_artificial_column_that_sums_past_2_to_24():
    d = C.big_sum_base()
    p = C.to_problem(lp, d)
    g = sbb.GeneralFormSingle(p)
    entry = (("y", 0, 3),)
    assert g.col_int_sum[g.col[0]] == 2 ** 24 + 3 and not g.device_ok(entry)
    art, _ = sbb.host_tableaux(p, entry)
    wM, wb, wA, wab = C.build_node(d, entry)
    assert sc.same_bits(art.matrix, wA) and np.array_equal(art.basis_columns, wab)
    assert art.matrix[-1, g.col[0]] == F32(2 ** 24 + 2)
    # what a float32 running sum would have made of it
    _, _, A, _ = sbb.node_tableaux_single(g, entry)
    assert A[-1, g.col[0]] == F32(2 ** 24)
    # a base whose integers stay small passes
    small = sbb.GeneralFormSingle(C.to_problem(lp, C.kind_case("both")))
    assert small.device_ok((("x", 0, 2), ("y", 1, 1)))
    assert not small.device_ok((("x", 0, 2 ** 24 + 8),))              # an integer right-hand side beyond 2^24


def test_search_with_default_parameters_is_the_exact_search():
    import math
    from tests import bb_oracle as B
    from tests import exact_bb_cases as X
    seed, p, (status, best, trace) = next(c for c in X.random_cases() if len(c[2][2]) >= 9)
    r = lp.exact_bb.search(p, X.oracle_round(p), 4)
    assert r.status == status and B.trace_key(r.trace) == B.trace_key(trace)
    r2 = lp.exact_bb.search(p, X.oracle_round(p), 4, fractional=lambda v: v.denominator != 1, floor=math.floor,
                            ceil=math.ceil)
    assert B.trace_key(r2.trace) == B.trace_key(r.trace) and r2.objectives == r.objectives


def test_search_with_the_float32_readings_replays_the_model():
    """exact_bb.search over the model's node solver: the one loop gives the model's trace at every width."""
    for name in C.search_cases():
        d, want = C.case(name)
        p = C.to_problem(lp, d)

        def solve_round(entries):
            out = []
            for e in entries:
                st, M, basis, mapping = C.solve_node(d, e)
                if st != sc.OPTIMAL:
                    out.append((st, None, None))
                else:
                    out.append((st, sc.objective(M), {v: sc.variable(M, basis, mapping, v) for v in d["vars"]}))
            return out
        for width in (1, 4, 16):
            r = lp.exact_bb.search(p, solve_round, width, fractional=sbb.fractional(0), floor=sbb.floor, ceil=sbb.ceil)
            assert C.same_trace(r.trace, want.trace), (name, width)
            assert r.status == want.status


def test_the_cases_cover_the_ground():
    outcomes, flips, arts = set(), 0, set()
    for name in C.search_cases():
        d, r = C.case(name)
        outcomes |= {row[4] for row in r.trace}
        g = sbb.GeneralFormSingle(C.to_problem(lp, d))
        entries = {-1: ()}
        for i, (parent, var, sense, bound, _, _) in enumerate(r.trace):
            entries[i] = () if parent < 0 else ((var, sense, int(bound)),) + entries[parent]
            if parent >= 0:
                flips += bool(g.row_rhs(var, int(bound)) < 0)
                arts.add(g.n_art + sum(g.row_artificial(*row) for row in entries[i]))
    assert {C.INFEASIBLE, C.PRUNED, C.BRANCHED, C.INCUMBENT} <= outcomes
    assert flips > 0 and {0, 1, 2, 3} <= arts
    assert any(row[3] < 0 for row in C.case("kind_free")[1].trace)        # a negative branching bound
    deep = C.search(C.random_ilp(*C.DEEP_CASE), max_nodes=80)
    assert deep.status == C.NODE_CAP and deep.depth > 8


def test_keyword_behaviour():
    ilp = C.to_problem(lp, C.kind_case("both"))
    plain = C.to_problem(lp, dict(C.kind_case("both"), integer_vars=[]))
    with pytest.raises(ValueError) as e:
        lp.solve_problem(plain, precision="single", branch_and_bound=True)
    assert "single" in str(e.value) and "branch_and_bound" in str(e.value)
    with pytest.raises(lp.UnsupportedConstraintError) as e:
        lp.solve_problem(ilp, precision="single")
    assert "integer" in str(e.value)
    with pytest.raises(ValueError) as e:
        lp.solve_problem(ilp, precision="single", branch_and_bound=True, exact=True)
    assert "single" in str(e.value) and "exact" in str(e.value)
    with pytest.raises(ValueError):
        lp.solve_problem(ilp, precision="single", branch_and_bound=True, bb_width=0)
    import inspect
    assert "branch_and_bound" not in inspect.signature(lp.mi355x_solve_problems).parameters


@pytest.mark.skipif(lp.capi.device_count() > 0, reason="a GPU is present")
def test_the_route_is_taken_and_needs_a_device():
    """Without a device the pair reaches the library (no ValueError any more) and fails loudly there."""
    with pytest.raises(lp.capi.Mi355xError):
        lp.solve_problem(C.to_problem(lp, C.kind_case("both")), precision="single", branch_and_bound=True)


def test_new_entries_validate_their_arguments():
    import ctypes
    L, BAD = lp.capi.lib(), lp.capi.MI_BAD_ARG
    h, h2 = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.mi355x_sbb_base_create(ctypes.byref(h), 0, 4, None, None, 1, 0, 1, None, None, None, None, 0) == BAD
    assert L.mi355x_sbatch_create_nodes(ctypes.byref(h), ctypes.byref(h2), None, 1, 1, None, None, None) == BAD
    assert L.mi355x_sbatch_readback(None, None, None, None) == BAD
    L.mi355x_sbb_base_destroy(None)
