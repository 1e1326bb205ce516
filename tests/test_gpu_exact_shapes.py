"""Exact tableaux larger than one workgroup, through the C ABI (mi355x_xtab_create / _solve /
_solve_two_phase / _download / _trace) with numpy arrays: the strided loops of k_x_select (more than
256 columns, more than 256 rows), its "lowest index wins" rule between elements of different threads
and strides, k_x_update with several blocks in x, an x-stride (more than 16 384 columns) and a y-stride
(more than 4 096 rows), x_snapshot of long rows, k_x_handover with several blocks, k_x_force on a long
row, and width escalation on a multi-block tableau.

The reference is exact_cases.VecModel (pinned to exact_cases.Model and the Fraction oracle by
tests/test_exact_host.py): every case is compared pivot for pivot (trace), then basis, D and every
entry of T.  What a case must reach -- pivot counts, ties, widths -- is asserted from the model before
the GPU runs, so a changed generator cannot quietly drop the coverage."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests.helpers import lp_amd

lp = lp_amd()
pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
RC = {"optimal": lp.capi.MI_OPTIMAL, "unbounded": lp.capi.MI_UNBOUNDED, "max_pivots": lp.capi.MI_MAX_PIVOTS}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class XTab:
    """An exact device tableau made from an integer matrix (every denominator 1)."""

    def __init__(self, T, basis, min_bits=0):
        T = np.ascontiguousarray(T, dtype=np.int64)
        basis = np.ascontiguousarray(basis, dtype=np.int64)
        self.shape, self.h = T.shape, ctypes.c_void_p()
        rc = lp.capi.lib().mi355x_xtab_create(ctypes.byref(self.h), T.shape[0], T.shape[1], _p(T),
                                              _p(np.ones_like(T)), _p(basis), 0, min_bits)
        assert rc == lp.capi.MI_OK, lp.capi.lib().mi355x_last_error()

    def solve(self, is_max, max_pivots=0):
        n = ctypes.c_int64(-1)
        rc = lp.capi.lib().mi355x_xtab_solve(self.h, int(is_max), max_pivots, ctypes.byref(n))
        return rc, n.value

    def state(self):
        """(T, D, basis): T int64 where every entry fits, Python ints otherwise."""
        R, C = self.shape
        raw = np.empty((R * C, 2), dtype=np.int64)
        D = np.empty(2, dtype=np.int64)
        b = np.empty(R - 1, dtype=np.int64)
        assert lp.capi.lib().mi355x_xtab_download(self.h, _p(raw), _p(D), _p(b)) == lp.capi.MI_OK
        lo, hi = raw[:, 0], raw[:, 1]
        if (hi == (lo >> 63)).all():
            T = lo.reshape(R, C)
        else:
            T = ((hi.astype(object) << 64) | (lo.astype(object) & M64)).reshape(R, C)
        return T, (int(D[1]) << 64) | (int(D[0]) & M64), b.tolist()

    def trace(self, cap=1 << 18):
        n = ctypes.c_int64(-1)
        e, r = np.full(cap, -1, dtype=np.int64), np.full(cap, -1, dtype=np.int64)
        assert lp.capi.lib().mi355x_xtab_trace(self.h, _p(e), _p(r), cap, ctypes.byref(n)) == lp.capi.MI_OK
        return list(zip(e[:n.value].tolist(), r[:n.value].tolist()))

    @property
    def bits(self):
        b = ctypes.c_int(0)
        assert lp.capi.lib().mi355x_xtab_bits(self.h, ctypes.byref(b)) == lp.capi.MI_OK
        return b.value

    def close(self):
        if self.h:
            lp.capi.lib().mi355x_xtab_destroy(self.h)
            self.h = None

    __del__ = close


def _same_state(x, model):
    T, D, basis = x.state()
    assert D == model.D and basis == model.basis
    if T.dtype == object or model.T.dtype == object:
        assert (T.astype(object) == model.T.astype(object)).all()
    else:
        assert np.array_equal(T, model.T)


def _model(T, basis, nv, is_max, max_pivots=0, at_least=3):
    m = ec.VecModel.from_state(T, 1, basis, nv)
    trace = []
    st = m.solve(is_max, trace, max_pivots)
    assert len(trace) >= at_least and m.stats["inexact"] == 0
    return m, st, trace


def _run(T, basis, is_max, model, st, trace, max_pivots=0, min_bits=0, bits=64):
    """The device against a solved model: status, pivot count, trace, width, basis, D and T."""
    assert model.stats["max_bits"] <= bits
    x = XTab(T, basis, min_bits)
    try:
        rc, n = x.solve(is_max, max_pivots)
        assert (rc, n) == (RC[st], len(trace)), lp.capi.lib().mi355x_last_error()
        assert x.trace() == trace
        assert x.bits == bits
        _same_state(x, model)
    finally:
        x.close()


def _case(T, basis, is_max=True, max_pivots=0, status=None, at_least=3):
    nv = T.shape[1] - 1
    model, st, trace = _model(T, basis, nv, is_max, max_pivots, at_least)
    assert status is None or st == status
    _run(T, basis, is_max, model, st, trace, max_pivots)
    return model, trace


# ---- wide: pricing strides (79 per thread), k_x_update's x-stride past 64 * 256 columns, long pivot rows
def test_wide_tableau_ends_unbounded():
    T, basis = ec.slack_tableau(6, 20000, 2)
    assert T.shape == (7, 20007) and (T[:6, :20000].max(axis=0) == 0).any()       # (an all-zero column)
    model, trace = _case(T, basis, max_pivots=100, status="unbounded", at_least=10)
    assert max(e for e, _ in trace) >= 64 * 256                                # an entering column of the second x-stride


def test_wide_tableau_bounded():
    T, basis = ec.slack_tableau(6, 20000, 2, entries=(1, 3))
    _case(T, basis, max_pivots=100, status="optimal")


# ---- planted ties: equal objective entries / equal ratios at i, i + 1, i + 256, i + 257 and last
def plant_price_tie(T, cols, is_max):
    """The objective row's best value, duplicated on `cols` and nowhere else."""
    nv = T.shape[1] - 1
    T[-1, cols] = T[-1, :nv].min() - 1 if is_max else T[-1, :nv].max() + 1


def plant_ratio_tie(T, e, rows):
    """The minimum ratio of column e, 1/3, on `rows` (as 1/3 and 2/6 in turn) and nowhere else: needs
    right-hand sides >= 2 and entries <= 3 elsewhere."""
    m = T.shape[0] - 1
    assert T[:m, -1].min() >= 2 and T[:m, e].max() <= 3
    for k, r in enumerate(rows):
        T[r, e], T[r, -1] = (3, 1) if k % 2 == 0 else (6, 2)


def _assert_ties(T, nv, is_max, cols, rows):
    """From the start state itself: `cols` tie for the pricing, `rows` for the ratio test of cols[0], every
    other candidate is strictly worse, and the model takes the first of each."""
    obj = T[-1, :nv]
    best = obj.min() if is_max else obj.max()
    assert np.nonzero(obj == best)[0].tolist() == sorted(cols) and len(cols) >= 3
    e, m = cols[0], T.shape[0] - 1
    a, b = T[:m, e], T[:m, -1]
    tied = [i for i in range(m) if a[i] > 0 and 3 * int(b[i]) == int(a[i])]
    assert tied == sorted(rows) and len(rows) >= 3
    assert all(3 * int(b[i]) > int(a[i]) for i in range(m) if a[i] > 0 and i not in rows)
    assert len({(int(a[i]), int(b[i])) for i in rows}) == 2                     # equal only after cross-multiplication


def _later_duplicates_differ(T, basis, nv, is_max, cols, rows, model, trace, k):
    """Taking a later duplicate instead (in pricing, in the ratio test) leads somewhere else."""
    for e, r in ((cols[0], rows[1]), (cols[1], None)):
        alt = ec.VecModel.from_state(T, 1, basis, nv)
        r = alt.ratio(e) if r is None else r
        alt_trace = [(e, r)]
        alt.pivot(e, r)
        alt.solve(is_max, alt_trace, k - 1)
        assert alt_trace != trace and alt_trace[0] != trace[0]
        assert alt.basis != model.basis or not np.array_equal(alt.T, model.T)


def _assert_tie_clause_decides(T, nv, is_max, cols, rows):
    """From a thread-for-thread model of k_x_select's two reductions (exact_cases.select_price /
    select_ratio): with the "equal and lower index" clause they pick the first duplicate, without it (the
    element at the lower thread position survives a tie) they pick a later one -- so a kernel that lost
    either clause fails this case."""
    m = T.shape[0] - 1
    assert ec.select_price(T[-1, :nv], is_max) == cols[0]
    assert ec.select_price(T[-1, :nv], is_max, tie_clause=False) in cols[1:]
    assert ec.select_ratio(T[:m, cols[0]], T[:m, -1]) == rows[0]
    assert ec.select_ratio(T[:m, cols[0]], T[:m, -1], tie_clause=False) in rows[1:]


# "spread": the issue's placement i, i + 1, i + 256, i + 257, last (and without its first two: the winner is
# then met in a thread's second stride).  There the lowest index always sits at the lowest thread position,
# so the tree's tie clause is not what decides.  "odd": an odd i and i + 1 -- the even thread i + 1 reaches
# position 0, the odd one position 1.  "stride": an index below 256 against one a lower thread keeps from
# its second stride.  In both the clause decides, which _assert_tie_clause_decides shows from the model.
TIE_PLACES = {"spread": ([70, 71, 326, 327, 399], [20, 21, 276, 277, 299], False),
              "spread-late": ([326, 327, 399], [276, 277, 299], False),
              "odd": ([71, 72, 399], [21, 22, 299], True),
              "stride": ([101, 300, 399], [5, 270, 299], True)}


@pytest.mark.parametrize("is_max", [True, False], ids=["max", "min"])
@pytest.mark.parametrize("place", sorted(TIE_PLACES))
def test_planted_ties_lowest_index_wins(is_max, place):
    m, n, k = 300, 400, 8
    cols, rows, clause_decides = TIE_PLACES[place]
    T, basis = ec.slack_tableau(m, n, 11, rhs=(2, 9))
    if not is_max:
        T[-1] = -T[-1]
    nv = n + m
    plant_price_tie(T, cols, is_max)
    plant_ratio_tie(T, cols[0], rows)
    _assert_ties(T, nv, is_max, cols, rows)
    if clause_decides:
        _assert_tie_clause_decides(T, nv, is_max, cols, rows)
    model, st, trace = _model(T, basis, nv, is_max, k, at_least=k)
    assert trace[0] == (cols[0], rows[0])
    _later_duplicates_differ(T, basis, nv, is_max, cols, rows, model, trace, k)
    _run(T, basis, is_max, model, st, trace, max_pivots=k)


def test_planted_ties_in_a_tableau_below_half_a_workgroup():
    """90 variables, 40 constraints: both reduction trees of k_x_select start below the workgroup size (at
    128 and at 64), and the tie clause decides ("odd": see TIE_PLACES).  Trace and entries against the
    Fraction oracle, at 64 bits and at 128."""
    m, n, k = 40, 50, 8
    cols, rows = [21, 22, 49], [11, 12, 39]
    T, basis = ec.slack_tableau(m, n, 11, rhs=(2, 9))
    nv = n + m
    plant_price_tie(T, cols, True)
    plant_ratio_tie(T, cols[0], rows)
    _assert_ties(T, nv, True, cols, rows)
    _assert_tie_clause_decides(T, nv, True, cols, rows)
    t = rr.Tableau([[Fraction(int(x)) for x in row] for row in T], basis.tolist(), nv, m, {}, True)
    trace = []
    for _ in range(k):
        e = rr.price(t)
        trace.append((e, rr.ratio(t, e)))
        rr.pivot(t, *trace[-1])
    assert trace[0] == (cols[0], rows[0])
    for min_bits, bits in ((0, 64), (128, 128)):
        x = XTab(T, basis, min_bits)
        try:
            assert x.solve(True, k) == (lp.capi.MI_MAX_PIVOTS, k), lp.capi.lib().mi355x_last_error()
            assert x.trace() == trace and x.bits == bits
            Tx, D, b = x.state()
            assert b == t.basis
            assert [[Fraction(int(v), D) for v in row] for row in Tx.tolist()] == t.matrix
        finally:
            x.close()


# ---- tall: ratio-test strides, gridDim.y capped at 4 096 with a y-stride
@pytest.mark.parametrize("rows,clause_decides", [([1000, 1001, 1256, 1257, 4199], False),
                                                 ([1001, 1002, 1258, 4199], True)], ids=["spread", "odd"])
def test_tall_tableau(rows, clause_decides):
    """Planted ratio ties: neighbours, rows 256 apart, the last row ("odd": see TIE_PLACES)."""
    m, n = 4200, 4
    T, basis = ec.slack_tableau(m, n, 1, rhs=(2, 9), density=0.3)
    assert T.shape == (4201, 4205)
    e = int(np.argmin(T[-1, :n]))
    plant_ratio_tie(T, e, rows)
    a, b = T[:m, e], T[:m, -1]
    assert [i for i in range(m) if a[i] > 0 and 3 * int(b[i]) == int(a[i])] == rows
    assert all(3 * int(b[i]) > int(a[i]) for i in range(m) if a[i] > 0 and i not in rows)
    if clause_decides:
        assert ec.select_ratio(a, b) == rows[0] and ec.select_ratio(a, b, tie_clause=False) in rows[1:]
    model, trace = _case(T, basis, max_pivots=100, status="optimal")      # (capped: a wrong update must fail, not cycle)
    assert trace[0] == (e, rows[0])
    assert (model.T[4096:m, :n] != T[4096:m, :n]).any()                        # the y-stride's rows change
    assert max(r for _, r in trace) >= 2 * 256                                 # a pivot row of a later stride


# ---- middle: 300 rows x 400 variables, both strides at once, tens of pivots, width escalation
def test_middle_tableau_20_pivots_at_64_bits_and_at_128():
    T, basis = ec.slack_tableau(300, 400, 1)
    assert T.shape == (301, 701)
    model, st, trace = _model(T, basis, 700, True, 20, at_least=20)
    assert st == "max_pivots" and model.stats["max_bits"] <= 64
    _run(T, basis, True, model, st, trace, max_pivots=20, bits=64)
    _run(T, basis, True, model, st, trace, max_pivots=20, min_bits=128, bits=128)


def test_middle_tableau_60_pivots_escalate_on_the_way():
    T, basis = ec.slack_tableau(300, 400, 1)
    model, st, trace = _model(T, basis, 700, True, 60, at_least=60)
    assert st == "max_pivots" and 64 < model.stats["max_bits"] <= 128
    stage, at = model.stats["over64"]
    assert 20 < at < 60                                          # 64 bits hold for the first 20, not for all 60
    x = XTab(T, basis)
    try:
        assert x.solve(True, 20) == (lp.capi.MI_MAX_PIVOTS, 20) and x.bits == 64
        assert x.trace() == trace[:20]
        assert x.solve(True, 40) == (lp.capi.MI_MAX_PIVOTS, 40) and x.bits == 128    # restarted wider, the same pivots
        assert x.trace() == trace
        _same_state(x, model)
    finally:
        x.close()
    _run(T, basis, True, model, st, trace, max_pivots=60, bits=128)           # and in one call


# ---- edges: rows and var_count around the block sizes
@pytest.mark.parametrize("rows,var_count,seed", [(255, 257, 2), (256, 511, 1), (256, 512, 1), (257, 511, 1),
                                                 (257, 513, 1), (511, 513, 1), (512, 513, 2), (513, 515, 2),
                                                 (101, 255, 1), (101, 256, 1), (101, 257, 1)])
def test_block_boundary_shapes(rows, var_count, seed):
    """rows and var_count around 256 and 512.  Every start needs rows - 1 unit basis columns among its
    var_count columns, so var_count 255 or 256 (255 / 256 priced columns, 256 / 257 stored ones: one column
    per thread, one block of k_x_update exactly) cannot go with 255 and more rows and 3 pivots: those
    widths are run with 101 rows, and 513 rows with 515 columns."""
    m = rows - 1
    T, basis = ec.slack_tableau(m, var_count - m, seed)
    assert T.shape == (rows, var_count + 1)
    _case(T, basis, max_pivots=12)


# ---- two-phase: k_x_handover with several blocks, k_x_force on a long row, src = nav for the last column
def _int_matrix(t):
    assert all(x.denominator == 1 for row in t.matrix for x in row)
    return np.array([[int(x) for x in row] for row in t.matrix], dtype=np.int64)


@pytest.mark.parametrize("seed,bits", [(5, 64), (1, 128)])
def test_two_phase_hand_over_wider_than_one_block(seed, bits):
    """(seed 1 outgrows 64 bits on the way: both tableaux start again at 128.)"""
    p = ec.mixed_problem(lp, 300, 40, 6, 4, seed)
    art_t, main_t = rr.build_tableau(ec.to_dict(p))
    assert main_t.var_count + 1 > 256 and art_t.var_count > main_t.var_count
    keep, extra = {}, 6
    st, trace, mm, stats = ec.model_solve((art_t, main_t), cls=ec.VecModel, keep=keep, phase2_pivots=extra)
    assert st == "max_pivots" and stats["driveouts"] >= 1 and stats["inexact"] == 0 and keep["n1"] >= 3
    assert len(trace) == keep["n1"] + extra and stats["max_bits"] <= 128
    assert bits == (64 if stats["max_bits"] <= 64 else 128)
    a = XTab(_int_matrix(art_t), art_t.basis)
    b = XTab(_int_matrix(main_t), main_t.basis)
    try:
        npv = (ctypes.c_int64 * 2)(-1, -1)
        cap = keep["n1"] + stats["driveouts"] + extra
        rc = lp.capi.lib().mi355x_xtab_solve_two_phase(a.h, b.h, 1, cap, npv)
        assert rc == lp.capi.MI_MAX_PIVOTS, lp.capi.lib().mi355x_last_error()
        assert list(npv) == [keep["n1"] + stats["driveouts"], extra]
        assert a.trace() + b.trace() == trace
        assert a.bits == bits and b.bits == bits
        _same_state(a, keep["art"])
        _same_state(b, mm)
    finally:
        a.close()
        b.close()
