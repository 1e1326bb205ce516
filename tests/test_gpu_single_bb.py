"""Single-float branch-and-bound on the GPU: the device assembly of node tableaux before any pivot, the search
against the model (tests/single_bb_cases.py) at every width and both workgroup sizes, the ways a search ends,
int_tolerance, the two fall-backs, and the public call."""
import numpy as np
import pytest

from tests import single_bb_cases as C
from tests import single_cases as sc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi, sbb = lp.capi, lp.single_bb
F32 = np.float32
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)


# ------------------------------------------------------------------ assembly, before any pivot
# (main columns of a node, depth, members, artificial bound row in front, `>=` rows, `=` rows, artificial node rows)
ASSEMBLY = [(31, 1, 1, False, 0, 0, 0),        # one below the padding boundary, no artificial row
            (32, 2, 3, False, 0, 0, 1),        # at the boundary; the node's own artificial row alone
            (33, 5, 65, True, 1, 0, 1),        # one above; the node's artificial row between base artificial rows
            (32, 1, 65, False, 2, 0, 1),       # the node's artificial row first
            (33, 2, 3, True, 0, 0, 2),         # the node's artificial rows last
            (30, 2, 3, False, 1, 1, 1),        # 33 artificial-tableau columns: the boundary inside the artificial columns
            (31, 5, 3, False, 0, 0, 0)]


@pytest.mark.parametrize("node_cols,d,n,art_bound,n_ge,n_eq,want", ASSEMBLY)
def test_assembly_equals_the_models_build_bit_for_bit(node_cols, d, n, art_bound, n_ge, n_eq, want):
    base = C.assembly_base(node_cols, d, art_bound, n_ge, n_eq, seed=node_cols + d)
    g = sbb.GeneralFormSingle(C.to_problem(lp, base))
    entries = C.assembly_nodes(100 * d + n, d, n, want)
    n_art = int(art_bound) + n_ge + n_eq + want
    b = sbb.Base(g)
    main, art = b.create_nodes(entries)
    b.close()
    assert (main.n_lps, main.cols) == (n, node_cols) and main.info()["ld"] == (node_cols + 31) // 32 * 32
    assert (art is None) == (n_art == 0)
    if art:
        assert art.cols == node_cols + n_art and art.rows == main.rows
    for q, e in enumerate(entries):
        wM, wb, wA, wab = C.build_node(base, e)
        M, mb = main.download(q)
        assert same_bits(M, wM) and np.array_equal(mb, wb), q
        assert main.trace(q).shape[0] == 0
        if art:
            A, ab = art.download(q)
            assert same_bits(A, wA) and np.array_equal(ab, wab), q
            assert art.trace(q).shape[0] == 0
    # every member starts MI_RUNNING: one call solves each to the model's end
    is_max = base["type"] == "max"
    st = (art.solve_two_phase(main, is_max, 1024, C.PIVOT_CAP) if art else main.solve(is_max, 1024, C.PIVOT_CAP))[0]
    for q in range(min(n, 3)):
        assert int(st[q]) == C.solve_node(base, entries[q])[0], q


# ------------------------------------------------------------------ the search
def _library_search(d, width=1, threads=0, **kw):
    lp.single.set_batch_threads(threads)
    s = sbb.SingleBranchAndBound(C.to_problem(lp, d), width=width, max_pivots=C.PIVOT_CAP, **kw)
    return s, s.run()


def _same_incumbent(d, t, want):
    assert isinstance(t, lp.SingleTableau)
    assert same_bits(t.matrix, want.M) and np.array_equal(t.basis_columns, want.basis)
    for v in d["vars"]:
        got = lp.tableau_variable(t, v)
        assert isinstance(got, F32) and same_bits(np.array([got]), np.array([want.values[v]])), v
    assert same_bits(np.array([lp.tableau_objective_value(t)]), np.array([want.objective]))


@pytest.mark.parametrize("name", C.search_cases())
def test_search_equals_the_model(name):
    d, want = C.case(name)
    for threads in (256, 1024):
        for width in (1, 4, 16):
            if want.status == sc.INFEASIBLE:
                s = sbb.SingleBranchAndBound(C.to_problem(lp, d), width=width, max_pivots=C.PIVOT_CAP)
                lp.single.set_batch_threads(threads)
                with pytest.raises(lp.InfeasibleProblemError):
                    s.run()
            else:
                s, t = _library_search(d, width, threads)
                _same_incumbent(d, t, want)
            assert C.same_trace(s.trace(), want.trace), (threads, width)
            st = s.stats()
            assert st["processed"] == len(want.trace) and st["max_depth"] == want.depth
            assert st["host_built"] == st["one_by_one"] == st["declined"] == 0


def test_integer_infeasible_problem():
    d = C.infeasible_case()
    want = C.search(d)
    assert want.status == sc.INFEASIBLE and [r[4] for r in want.trace] == [C.BRANCHED, C.INFEASIBLE, C.INFEASIBLE]
    s = sbb.SingleBranchAndBound(C.to_problem(lp, d), width=4, max_pivots=C.PIVOT_CAP)
    with pytest.raises(lp.InfeasibleProblemError):
        s.run()
    assert C.same_trace(s.trace(), want.trace)


def test_unbounded_root_ends_the_search():
    d = C.unbounded_case()
    want = C.search(d)
    assert want.status == sc.UNBOUNDED and [r[4] for r in want.trace] == [C.FAILED]
    s = sbb.SingleBranchAndBound(C.to_problem(lp, d), width=4, max_pivots=C.PIVOT_CAP)
    with pytest.raises(lp.UnboundedProblemError):
        s.run()
    assert C.same_trace(s.trace(), want.trace)


def test_max_nodes_stops_the_deep_case():
    d = C.random_ilp(*C.DEEP_CASE)
    want = C.search(d, max_nodes=24)                # (that it is deep -- past depth 8 -- is test_single_bb_host.py's)
    assert want.status == C.NODE_CAP and len(want.trace) == 24
    for width in (1, 8):
        s = sbb.SingleBranchAndBound(C.to_problem(lp, d), width=width, max_pivots=C.PIVOT_CAP, max_nodes=24)
        with pytest.raises(lp.SolverError) as e:
            s.run()
        assert "node cap" in str(e.value)
        assert C.same_trace(s.trace()[:24], want.trace) and len(s.trace()) == 24


def test_int_tolerance():
    d = C.tolerance_case()
    strict, loose = C.search(d), C.search(d, int_tolerance=8)
    root_x = sc.variable(*[C.solve_node(d, ())[k] for k in (1, 2, 3)], "x")
    assert 0 < abs(F32(root_x - F32(3))) <= F32(F32(4) * sc.EPS_S)
    assert [r[4] for r in strict.trace] == [C.BRANCHED, C.INCUMBENT, C.INFEASIBLE]
    assert [r[4] for r in loose.trace] == [C.INCUMBENT]
    for tol, want in ((0, strict), (8, loose)):
        s, t = _library_search(d, 2, int_tolerance=tol)
        assert C.same_trace(s.trace(), want.trace)
        _same_incumbent(d, t, want)
    assert strict.values["x"] == F32(3) and loose.values["x"] == root_x


def test_a_group_that_fails_the_guard_is_built_on_the_host():
    d = C.guard_case()
    want = C.search(d)
    assert want.status == sc.OPTIMAL and len(want.trace) >= 5
    s, t = _library_search(d, 4)
    assert C.same_trace(s.trace(), want.trace)
    _same_incumbent(d, t, want)
    assert s.stats()["host_built"] == s.stats()["solved"] - 1 and s.stats()["one_by_one"] == 0
    # and the library itself refuses such a group
    g = sbb.GeneralFormSingle(C.to_problem(lp, d))
    b = sbb.Base(g)
    with pytest.raises(capi.Mi355xError) as e:
        b.create_nodes([(("y", 0, 3),)])
    assert e.value.code == capi.MI_UNSUPPORTED
    b.close()


def test_a_node_shape_beyond_the_lds_budget_goes_node_by_node():
    d = C.tall_case()
    want = C.search(d)
    assert want.status == sc.OPTIMAL and len(want.trace) >= 5
    s, t = _library_search(d, 4)
    assert C.same_trace(s.trace(), want.trace)
    _same_incumbent(d, t, want)
    assert s.stats()["one_by_one"] == s.stats()["solved"] - 1 and s.stats()["host_built"] == 0


def test_public_call():
    d, want = C.case("kind_both")
    p = C.to_problem(lp, d)
    t = lp.solve_problem(p, precision="single", branch_and_bound=True, max_pivots=C.PIVOT_CAP)
    assert isinstance(t, lp.SingleTableau)
    test = sbb.fractional(0)
    for v in p.integer_vars:
        assert not test(lp.tableau_variable(t, v))
    _same_incumbent(d, t, want)
    t4 = lp.solve_problem(p, precision="single", branch_and_bound=True, bb_width=4, max_pivots=C.PIVOT_CAP, chunk=3)
    assert same_bits(t4.matrix, t.matrix)
