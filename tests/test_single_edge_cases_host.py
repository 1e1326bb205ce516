"""Conditions on the inputs of tests/test_gpu_single_edges.py, asserted on the float32 model alone (no GPU, no
library): every directed case has the winner and the geometry its docstring claims relative to 64, 256, 1024 and 4096;
every seeded member is as extreme as claimed; the hand-over cases end as claimed.  These are conditions on the
inputs, not measurements: a later edit of the generators that quietly turns the GPU tests into easy ones fails here.

The last section shows that the cases tell a wrong kernel from a right one: against a model whose ratio test lets a
thread's first NaN quotient stick, and against one whose pivot flushes subnormals to zero, the answers differ."""
import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_edge_cases as E

F32 = np.float32
WAVE, QUAD = 64, 4


def subnormal(x):
    return (np.abs(x) > 0) & (np.abs(x) < E.TINY)


def test_the_model_keeps_subnormals():
    with np.errstate(all="ignore"):
        assert F32(1e-30) * F32(1e-10) != 0 and subnormal(F32(1e-30) * F32(1e-10))
        assert subnormal(F32(1e-38) / F32(7))
    M = np.array([[F32(2), F32(1e-38)], [F32(-1), F32(0)]], dtype=F32)
    sc.pivot(M, np.zeros(1, dtype=np.int64), 0, 0)
    assert subnormal(M[0, 1]) and subnormal(M[1, 1])


# ------------------------------------------------------------------ a. pricing
@pytest.mark.parametrize("n", [4200, 8300])
@pytest.mark.parametrize("is_max", [True, False])
def test_pricing_cases(n, is_max):
    sgn = F32(1 if is_max else -1)
    for name in E.PRICING:
        M0 = E.pricing_case(name, n, is_max)[0]
        special = {"P1": E.P1_TIED + E.P1_NANS, "P2": (0, E.P2_INF), "P3": (0, E.P3_INF) + E.P3_NANS}[name]
        rest = np.delete(M0, special, axis=1)
        assert np.array_equal(rest, np.round(rest)) and np.isfinite(rest).all()       # integer-valued elsewhere
        assert np.isfinite(M0[:-1]).all() and M0.shape == (4, n + 4)
    # the pair's 1024-thread select beyond a leading dimension of 8192 floats; a second trip of 1024 threads beyond 4096
    assert (n + 4 > 8192) == (n == 8300) and (n + 4) // QUAD > 1024
    M0, _, _, cap, (st, tr, M, b) = E.pricing_case("P1", n, is_max)
    key = M0[-1] * sgn
    assert (key[list(E.P1_TIED)] == -7).all() and np.isnan(key[list(E.P1_NANS)]).all()
    assert np.nanmin(key[:n]) == -7 and sorted(np.where(key == -7)[0]) == list(E.P1_TIED)
    c = E.P1_TIED
    assert c[0] // QUAD == WAVE - 1 and c[1] // QUAD == WAVE                   # lanes 63 | 64
    assert c[2] // QUAD == 256 and c[3] // QUAD == 1024                        # the second trip at 256 / 1024 threads
    assert 252 in E.P1_NANS and 252 // QUAD == c[0] // QUAD                    # a NaN in the winner's own quad
    assert all(any(abs(x - t) <= 2 for t in c) or x == 252 for x in E.P1_NANS)
    assert sc.price(M0, is_max) == 255 and tr[0][0] == 255 and len(tr) == cap and st == sc.MAX_PIVOTS
    M0, _, _, cap, (st, tr, M, b) = E.pricing_case("P2", n, is_max)
    assert np.isnan(M0[-1, 0]) and M0[-1, E.P2_INF] * sgn == -np.inf
    assert E.P2_INF // QUAD > 1024 and E.P2_INF < n                             # another trip than column 0, at both sizes
    assert (np.delete(M0[-1, :n] * sgn, [0, E.P2_INF]) < 0).all()
    assert sc.price(M0, is_max) is None and (st, tr) == (sc.OPTIMAL, []) and sc.same_bits(M, M0)
    M0, _, _, cap, (st, tr, M, b) = E.pricing_case("P3", n, is_max)
    assert M0[-1, 0] * sgn == -3 and np.isnan(M0[-1, 1:4]).all() and M0[-1, E.P3_INF] * sgn == -np.inf
    assert max(E.P3_NANS) // QUAD == 0 and E.P3_INF // QUAD == 1024
    assert sc.price(M0, is_max) == E.P3_INF and tr[0][0] == E.P3_INF and 1 <= len(tr) <= cap
    s, i, nn = E.census(M)
    assert i > n // 2 and nn >= 5                            # infinities and NaNs went through a whole update


# ------------------------------------------------------------------ b. ratio
@pytest.mark.parametrize("rows,slack", [(1100, False), (1100, True), (300, False), (300, True)])
def test_ratio_cases(rows, slack):
    for name in E.RATIO:
        M0, b0, is_max, cap, (st, tr, M, b) = E.ratio_case(name, rows, slack)
        winner, placed, first = E.ratio_geometry(name, rows)
        assert M0.shape == (rows + 1, 7 + (rows if slack else 0)) and is_max and cap == 3
        assert sc.price(M0, True) == 2 and (M0[-1] < 0).sum() == 1               # only column 2 is priced in
        thr = sc.thresholds()[1]
        elig = np.where(M0[:rows, 2] > thr)[0]
        assert elig[0] == first and (M0[:first, 2] == -1).all() and len(elig) > len(placed) + 10
        assert sc.ratio(M0, 2) == winner and tr[0] == (2, winner) and 1 <= len(tr) <= cap
        with np.errstate(all="ignore"):
            q = M0[:rows, -1] / M0[:rows, 2]
        others = [r for r in elig if r not in placed]
        assert (q[others] == 64).all()
        special = np.zeros(M0.shape, dtype=bool)
        special[list(placed), 2] = special[list(placed), -1] = True
        assert np.array_equal(M0[~special], np.round(M0[~special]))              # integer-valued elsewhere
        assert np.isnan(M).any()                                                 # the NaN went through an update
    g = {name: E.ratio_geometry(name, rows) for name in E.RATIO}
    if rows == 1100:
        assert rows + 1 > 1024                               # the pair's 1024-thread select; two trips at 256 threads
        assert g["R1"][0] == 700 and set(g["R1"][1]) == {700, 1090} and 700 // WAVE != 1090 // WAVE
        w, p, f = g["R2"]
        assert (w, f) == (1035, 10) and sorted(p) == [10, 11, 267, 1035]
        assert 267 % 256 == 11 and 1035 % 256 == 11 and 1035 % 1024 == 11       # thread 11 owns the NaN and the winner
        assert g["R2b"][0] == 267 and sorted(g["R2b"][1]) == [10, 11, 267]
        assert g["R3"][0] == 900 and sorted(g["R3"][1]) == [700, 701, 900, 1099]
        assert sorted(g["R4"][1]) == [64, 63 + 256] and g["R4"][0] == 64 and 64 // WAVE == 1
    else:
        assert 256 < rows + 1 <= 1024                        # the pair's 256-thread select, with a second trip
        assert g["R2"][0] == 267 and 267 % 256 == 11 and g["R2b"][0] == 139 and 139 // WAVE != 11 // WAVE
    for name in ("R2", "R2b", "R3"):                         # quotients: the first eligible row finite, NaNs later
        M0 = E.ratio_case(name, rows, slack)[0]
        w, p, f = g[name]
        with np.errstate(all="ignore"):
            q = {r: F32(M0[r, -1] / M0[r, 2]) for r in p}
        assert np.isfinite(q[f]) and sum(np.isnan(v) for v in q.values()) >= 1
        assert q[w] == min(v for v in q.values() if not np.isnan(v)) and q[w] < 5
        assert sum(v == q[w] for v in q.values()) == 1                           # a strict minimum
    for name in ("R1", "R4"):                                # the first eligible row's quotient is a NaN
        M0 = E.ratio_case(name, rows, slack)[0]
        w, p, f = g[name]
        with np.errstate(all="ignore"):
            assert w == f and all(np.isnan(F32(M0[r, -1] / M0[r, 2])) for r in p)
    M0 = E.ratio_case("R4", rows, slack)[0]
    assert all(M0[r, 2] == np.inf and M0[r, -1] == np.inf for r in g["R4"][1])


# ------------------------------------------------------------------ c. extreme magnitudes
@pytest.mark.parametrize("shape", sorted(E.EXTREME))
def test_extreme_members_are_extreme(shape):
    m, n = shape
    members = E.EXTREME[shape]
    assert len(members) == 8 and len({(lo, hi) for lo, hi, _ in members}) == 8
    outcomes = set()
    for k in range(8):
        M0, b0, is_max, cap, (st, tr, M, b) = E.extreme_case(m, n, k)
        assert cap == 60 and M0.shape == (m + 1, n + m + 1) and np.isfinite(M0).all()
        assert len(tr) >= 8, (k, len(tr))
        assert min(E.census(M)) >= 1, (k, E.census(M))       # a subnormal, an infinity and a NaN at the end
        st1, tr1, M1, _ = sc.solve(M0, b0, True, cap=len(tr) - 1)
        assert tr1 == tr[:-1] and sum(E.census(M1)) >= 1, k  # ... and one of them before the last pivot
        outcomes.add((st, len(tr)))
    assert len(outcomes) >= 3
    if shape == (24, 40):                                    # the generator is the one the seeds were found with
        assert len(E.extreme_case(24, 40, 0)[4][1]) == 20 and E.census(E.extreme_case(24, 40, 0)[4][2]) == (20, 34, 183)
    if shape == (61, 97):
        assert len(E.extreme_case(61, 97, 0)[4][1]) == 12 and E.census(E.extreme_case(61, 97, 0)[4][2]) == (32, 5, 154)


# ------------------------------------------------------------------ d. subnormal right-hand sides
def _flushed(M):
    M = np.array(M)
    M[subnormal(M)] = 0
    return M


@pytest.mark.parametrize("m,n,n_sub,pivots_147", [(61, 97, 36, 28), (130, 203, 34, 42)])
def test_subnormal_right_hand_sides(m, n, n_sub, pivots_147):
    base0, _, bst, btr, bM, _ = sc.solved_synthetic(n, m)
    btr = [tuple(int(v) for v in x) for x in btr]
    assert bst == sc.OPTIMAL and len(btr) == {61: 26, 130: 44}[m] and len(btr) < E.EXTREME_CAP
    for e in E.SUBNORMAL_EXPONENTS:
        M0, b0, is_max, cap, (st, tr, M, b) = E.subnormal_case(m, n, e)
        assert st == sc.OPTIMAL and not np.isnan(M).any() and not np.isinf(M).any()
        assert np.array_equal(M0[:, :-1], base0[:, :-1])
        assert not (M[:, -1] == 0).any() and not (bM[:, -1] == 0).any()          # no zero where the unscaled solve has none
        n_in, n_out = int(subnormal(M0).sum()), int(subnormal(M[:, -1]).sum())
        if e == -130:                                        # normal inputs, subnormal outputs, the unscaled trace
            assert n_in == 0 and n_out == n_sub and tr == btr
        elif e == -140:                                      # every right-hand side entry subnormal
            assert n_in == m and n_out == m + 1 and tr == btr
        else:                                                # rounding inside the subnormal range changes the trace
            assert n_in == m and n_out == m + 1 and len(tr) == pivots_147 and tr != btr
        if e <= -140:                                        # a kernel that flushes its subnormal inputs cannot pass
            fst, ftr, fM, fb = sc.solve(_flushed(M0), b0, True, cap=cap)
            assert not sc.same_bits(fM, M)


# ------------------------------------------------------------------ e. hand-over
@pytest.mark.parametrize("k", [0, 1])
def test_h1_wide_drive_out(k):
    (A, ab, M, mb), w = E.handover_h1(k)
    nv = M.shape[1] - 1
    assert nv > 2 * 256 and A.shape[1] - 1 > nv and A.shape[0] == M.shape[0] == 7
    assert np.array_equal(np.nonzero(A[1, :nv])[0], E.H1_ROW1) and A[1, -1] == 0
    assert np.array_equal(np.nonzero(A[2, :nv])[0], E.H1_ROW2) and A[2, -1] == 0
    assert E.H1_ROW2 == (255, 256) and 256 < E.H1_ROW1[1] < E.H1_ROW1[2] < 512 < E.H1_ROW1[3]
    st, t1, A1, ab1 = sc.solve(A, ab, False)
    assert st == sc.OPTIMAL and len(t1) >= 2
    assert E.H1_BASIC in ab1 and ab1[1] >= nv and ab1[2] >= nv                   # column 40 basic, both artificials left
    assert A1[1, E.H1_BASIC] == 0 and 290 not in ab1 and 255 not in ab1
    assert w["art_trace"][:len(t1)] == [tuple(int(v) for v in x) for x in t1]
    assert w["art_trace"][len(t1):] == [(290, 1), (255, 2)]                      # exactly the two drive-outs
    assert w["status"] == sc.OPTIMAL and w["n1"] == len(t1) + 2 and w["n2"] >= 2
    assert not sc.same_bits(E.handover_h1(0)[1]["M"], E.handover_h1(1)[1]["M"])


def test_h2_h3_h4_small_hand_overs():
    shapes = {(E.handover_small(nm)[0][0].shape, E.handover_small(nm)[0][2].shape) for nm in E.HANDOVER_SMALL}
    assert shapes == {((3, 6), (3, 5))}                      # one batch holds them all
    (A, ab, M, mb), w = E.handover_small("H2")
    assert np.isnan(A[-1, -1]) and sc.solve(A, ab, False)[:2] == (sc.OPTIMAL, [])
    assert w["status"] == sc.INFEASIBLE and (w["n1"], w["n2"]) == (0, 0) and sc.same_bits(w["M"], M)
    (A, ab, M, mb), w = E.handover_small("H3")
    row = int(np.where(ab >= M.shape[1] - 1)[0][0])
    assert A[-1, -1] == 0 and np.isnan(A[row, -1]) and sc.solve(A, ab, False)[:2] == (sc.OPTIMAL, [])
    assert w["status"] == sc.ART_NONZERO and (w["n1"], w["n2"]) == (0, 0) and sc.same_bits(w["M"], M)
    (A, ab, M, mb), w = E.handover_small("H4")
    assert np.isinf(M[-1]).sum() == 1 and int(np.argmax(np.isinf(M[-1]))) in w["abasis"]
    assert w["art_trace"] == [(1, 1)] and M[-1, 1] == np.inf and w["abasis"][1] == 1
    assert w["main_trace"] == [(0, 1)] and w["n2"] == 1                          # -inf in column 0 enters
    assert w["status"] == sc.OPTIMAL and np.isnan(w["M"][-1]).all()              # inf - inf, inf * 0, then a NaN in column 0
    assert np.isfinite(w["M"][:-1]).all()
    (A, ab, M, mb), w = E.handover_small("H0")
    assert w["status"] == sc.OPTIMAL and w["n1"] == 1 and w["n2"] == 1 and np.isfinite(w["M"]).all()


# ------------------------------------------------------------------ the cases tell a wrong kernel from a right one
def _solve_with(M0, basis0, is_max, cap, ratio=sc.ratio, pivot=sc.pivot):
    """sc.solve with the ratio test or the pivot swapped for a deliberately wrong one."""
    M, basis = np.array(M0, dtype=F32, copy=True), np.array(basis0, dtype=np.int64, copy=True)
    trace = []
    while True:
        ec = sc.price(M, is_max)
        if ec is None:
            return sc.OPTIMAL, trace, M, basis
        if len(trace) >= cap:
            return sc.MAX_PIVOTS, trace, M, basis
        cr = ratio(M, ec)
        if cr is None:
            return sc.UNBOUNDED, trace, M, basis
        pivot(M, basis, ec, cr)
        trace.append((int(ec), int(cr)))


def _sticky_nan_ratio(threads):
    """WRONG on purpose: every thread scans its own rows (r = t mod threads) in the reference's way, so a NaN quotient
    in a THREAD's first eligible row sticks there; the block then takes the lowest-index NaN if there is one."""
    def ratio(M, ec):
        thr, vc, m = sc.thresholds()[1], M.shape[1] - 1, M.shape[0] - 1
        per_thread = []
        with np.errstate(all="ignore"):
            for t in range(min(threads, m)):
                best, bq = None, None
                for i in range(t, m, threads):
                    if thr < M[i, ec]:
                        q = F32(M[i, vc] / M[i, ec])
                        if best is None or q < bq:
                            best, bq = i, q
                if best is not None:
                    per_thread.append((best, bq))
        nans = [i for i, q in per_thread if np.isnan(q)]
        if nans:
            return min(nans)
        return min(per_thread, key=lambda x: (x[1], x[0]))[0] if per_thread else None
    return ratio


def _flushing_pivot(M, basis, ec, cr):
    """WRONG on purpose: n-pivot-row on hardware that flushes subnormal results to zero."""
    sc.pivot(M, basis, ec, cr)
    M[subnormal(M)] = 0


def test_the_self_check_reproduces_the_model():
    M0, b0, is_max, cap, (st, tr, M, b) = E.ratio_case("R2", 300)
    got = _solve_with(M0, b0, is_max, cap)
    assert got[:2] == (st, tr) and sc.same_bits(got[2], M)


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["R2", "R2b", "R3"])
def test_a_ratio_test_whose_thread_first_nan_sticks_fails_the_case(name, threads):
    for rows in (1100, 300):
        M0, b0, is_max, cap, (st, tr, M, b) = E.ratio_case(name, rows)
        wrong = _solve_with(M0, b0, is_max, cap, ratio=_sticky_nan_ratio(threads))
        assert wrong[1][0] != tr[0] and not sc.same_bits(wrong[2], M)
        assert np.isnan(M0[wrong[1][0][1], -1])              # it took a NaN row


@pytest.mark.parametrize("m,n", [(61, 97), (130, 203)])
def test_a_pivot_that_flushes_subnormals_fails_the_cases(m, n):
    for e in E.SUBNORMAL_EXPONENTS:
        M0, b0, is_max, cap, (st, tr, M, b) = E.subnormal_case(m, n, e)
        wrong = _solve_with(M0, b0, is_max, cap, pivot=_flushing_pivot)
        assert not sc.same_bits(wrong[2], M), e
    M0, b0, is_max, cap, (st, tr, M, b) = E.extreme_case(m, n, 0)
    wrong = _solve_with(M0, b0, is_max, cap, pivot=_flushing_pivot)
    assert not sc.same_bits(wrong[2], M)
