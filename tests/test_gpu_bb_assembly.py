"""k_assemble<BbSrc>: branch-and-bound node tableaux assembled on the device (mi355x_bb_debug_assemble) are
bit-identical -- main tableau, artificial tableau and both bases, -0.0 included -- to the host
build-tableau (mi355x_build_tableau) of the node problem."""
import ctypes

import numpy as np
import pytest

from tests import bb_oracle as B
from tests.helpers import lp_amd

lp = lp_amd()
pytestmark = pytest.mark.gpu


def _base(seed):
    """Every mapping kind (default >= 0, lower bound offset, both bounds, upper bound only, free) and
    base rows of all three senses, some with negative shifted right-hand sides."""
    rng = np.random.default_rng(seed)
    names = ["v%d" % i for i in range(7)]
    bounds = [("v1", (2.5, None)), ("v2", (-1.0, 3.25)), ("v3", (None, 4.5)), ("v4", (None, None)),
              ("v5", (1.0, 2.0)), ("v6", (-2.5, None))]
    cons = [("<=", [(v, float(rng.integers(1, 5))) for v in names], 30.5),
            (">=", [("v0", 1.0), ("v1", 2.0), ("v3", -1.0)], 1.5),
            ("=", [("v4", 1.0), ("v5", 1.5), ("v6", -0.5)], 0.75),
            ("<=", [("v1", 1.0), ("v2", 1.0)], 0.5),            # rhs - offsets < 0: negated, sense flips
            (">=", [("v6", 1.0), ("v0", 0.5)], 0.0)]
    return lp.Problem(type="max" if seed % 2 else "min", vars=names, integer_vars=list(names),
                      objective_func=[(v, float(rng.integers(-3, 5)) + 0.5) for v in names],
                      var_bounds=bounds, constraints=cons)


def _host(p, rows):
    tabs = lp.native.NativeProblem(B.node_problem(p, rows)).build_tableau()
    return (tabs[1], tabs[0]) if len(tabs) == 2 else (tabs[0], None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_assembly_is_bit_identical_to_build_tableau(seed):
    L = lp.capi.lib()
    p = _base(seed)
    npb = lp.native.NativeProblem(p)
    rng = np.random.default_rng(100 + seed)
    checked = 0
    for depth in range(1, 9):
        # node rows newest first; bounds around the offsets so that some shifted rhs are negative
        nodes = [tuple((p.vars[int(rng.integers(0, 7))], int(rng.integers(0, 2)), float(rng.integers(-4, 5)))
                       for _ in range(depth)) for _ in range(37 if depth != 3 else 300)]
        host = [_host(p, n) for n in nodes]
        groups = {}
        for q, (main, art) in enumerate(host):
            groups.setdefault(0 if art is None else art[0].shape[1], []).append(q)
        for acols, qs in groups.items():
            n = len(qs)
            var = np.array([[npb.index[v] for v, _, _ in nodes[q]] for q in qs], dtype=np.int64)
            sen = np.array([[s for _, s, _ in nodes[q]] for q in qs], dtype=np.int32)
            bnd = np.array([[b for _, _, b in nodes[q]] for q in qs], dtype=np.float64)
            R, C, AC = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            args = [npb._h, n, depth, ptr(var), ptr(sen), ptr(bnd), 0, ctypes.byref(R), ctypes.byref(C), ctypes.byref(AC)]
            lp.capi.check(L.mi355x_bb_debug_assemble(*args, None, None, None, None), "mi355x_bb_debug_assemble")
            assert AC.value == acols
            M = np.empty((n, R.value, C.value)); MB = np.empty((n, R.value - 1), np.int64)
            A = np.empty((n, R.value, max(AC.value, 1))); AB = np.empty((n, R.value - 1), np.int64)
            lp.capi.check(L.mi355x_bb_debug_assemble(*args, ptr(M), ptr(MB), ptr(A) if acols else None,
                                                     ptr(AB) if acols else None), "mi355x_bb_debug_assemble")
            for i, q in enumerate(qs):
                (hm, hb), art = host[q]
                assert np.array_equal(_bits(M[i]), _bits(hm)), (seed, depth, nodes[q])
                assert np.array_equal(MB[i], hb), (seed, depth, nodes[q])
                if art is not None:
                    assert np.array_equal(_bits(A[i]), _bits(art[0])), (seed, depth, nodes[q])
                    assert np.array_equal(AB[i], art[1]), (seed, depth, nodes[q])
                checked += 1
    assert checked == 7 * 37 + 300


def _assemble(npb, nodes):
    """mi355x_bb_debug_assemble of entries of one depth and one artificial-row count:
    (main, main bases, art or None, art bases or None, art_cols)."""
    L = lp.capi.lib()
    n, depth = len(nodes), len(nodes[0])
    var = np.array([[npb.index[v] for v, _, _ in e] for e in nodes], dtype=np.int64)
    sen = np.array([[s for _, s, _ in e] for e in nodes], dtype=np.int32)
    bnd = np.array([[b for _, _, b in e] for e in nodes], dtype=np.float64)
    R, C, AC = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = [npb._h, n, depth, ptr(var), ptr(sen), ptr(bnd), 0, ctypes.byref(R), ctypes.byref(C), ctypes.byref(AC)]
    lp.capi.check(L.mi355x_bb_debug_assemble(*args, None, None, None, None), "mi355x_bb_debug_assemble")
    acols = AC.value
    M = np.empty((n, R.value, C.value)); MB = np.empty((n, R.value - 1), np.int64)
    A = np.empty((n, R.value, max(acols, 1))); AB = np.empty((n, R.value - 1), np.int64)
    lp.capi.check(L.mi355x_bb_debug_assemble(*args, ptr(M), ptr(MB), ptr(A) if acols else None,
                                             ptr(AB) if acols else None), "mi355x_bb_debug_assemble")
    return M, MB, (A if acols else None), (AB if acols else None), acols


def _check_case(name):
    """Every node of the case, grouped by artificial-column count, against the host build-tableau: both
    tableaux and both bases bit for bit.  -> the groups' (main shape, artificial columns)."""
    p, nodes = B.assembly_case(name)
    host = B.host_node_tableaux(name)
    npb = lp.native.NativeProblem(p)
    groups = {}
    for q, (hm, hb, ha, hab) in enumerate(host):
        groups.setdefault(0 if ha is None else ha.shape[1], []).append(q)
    shapes = []
    for acols, qs in groups.items():
        M, MB, A, AB, got_acols = _assemble(npb, [nodes[q] for q in qs])
        assert got_acols == acols
        for i, q in enumerate(qs):
            hm, hb, ha, hab = host[q]
            assert M[i].shape == hm.shape
            assert np.array_equal(_bits(M[i]), _bits(hm)), (name, q, np.argwhere(_bits(M[i]) != _bits(hm))[:4])
            assert np.array_equal(MB[i], hb), (name, q)
            if ha is not None:
                assert A[i].shape == ha.shape
                assert np.array_equal(_bits(A[i]), _bits(ha)), (name, q, np.argwhere(_bits(A[i]) != _bits(ha))[:4])
                assert np.array_equal(AB[i], hab), (name, q)
        shapes.append((M.shape[1:], acols))
    return shapes


@pytest.mark.parametrize("name,rows_over", [("tall_300", 256), ("tall_1030", 1024)])
def test_tall_nodes_past_one_workgroup_and_past_the_row_grid(name, rows_over):
    """k_bb_rows strides over more than 256 rows and its rank scan crosses the trips; k_assemble's row
    grid (1024 blocks) wraps.  Artificial and negated rows lie in every range (tests/test_bb_host.py)."""
    for (rows, cols), acols in _check_case(name):
        assert rows - 1 > rows_over and acols > cols


def test_wide_nodes_past_the_column_grid():
    """k_assemble's column loop (16 blocks of 256 threads) makes a second trip: over the main tableau's
    row, and -- main inside one trip whatever the row padding up to 256 -- over the artificial tableau's."""
    for (rows, cols), acols in _check_case("wide_main"):
        assert cols > 4096 and acols > cols
    for (rows, cols), acols in _check_case("wide_art"):
        assert cols + 256 <= 4096 < acols


def test_inexact_artificial_objective_is_summed_in_increasing_row_order():
    """Non-dyadic entries over many binades: the host's artificial objective row is the increasing-order sum
    and differs from the decreasing-order and the pairwise sum at every node of the case (checked first)."""
    B.assert_sum_order_sensitive("inexact")
    _check_case("inexact")


def test_shifted_right_hand_sides_that_round_and_signed_zero_bounds():
    """bound - offset with non-dyadic offsets, bound = offset (+0.0, no flip) and bounds of -0.0 on every
    mapping kind (what the rows hold on the host: tests/test_bb_host.py)."""
    assert len(_check_case("shifted")) >= 3


def test_deep_nodes():
    """Depth 40: variables met several times in both senses, the -0.0 fill of negated base rows over forty
    inserted slack columns."""
    for (rows, cols), acols in _check_case("deep"):
        assert rows == 1 + 2 + 40 + 6


def test_debug_assemble_validates_its_arguments():
    L = lp.capi.lib()
    npb = lp.native.NativeProblem(_base(0))
    v = np.array([9], np.int64); s = np.array([0], np.int32); b = np.array([1.0])
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mi355x_bb_debug_assemble(npb._h, 1, 1, ptr(v), ptr(s), ptr(b), 0, *([None] * 7)) == lp.capi.MI_BAD_ARG
    assert L.mi355x_bb_debug_assemble(None, 1, 1, ptr(v), ptr(s), ptr(b), 0, *([None] * 7)) == lp.capi.MI_BAD_ARG
