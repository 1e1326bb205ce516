"""tests/single_threshold_cases.py checked on the float32 model alone (no GPU): every case
tests/test_gpu_single_thresholds.py uses is what it claims.  These are conditions on the INPUTS, not measurements:
a later edit of the builders that quietly moves an entry off its threshold fails here.

Bits: the planted entry has exactly the bits of sc.thresholds(f)[k] or of the next float beyond it, and those are the
values lp.single.thresholds(f) returns.
T: before step j the trace is the base's; after j pivots M[R, X] still has the planted bits, R is not the row the
base picks, lies in the later trip or wave its shape names, and its quotient 2^-10 is the strict minimum.
P: Y's key is bit-unchanged at the end, the `at` and `beyond` traces are equal, the statuses differ, k_end >= 3.
F: phase 1 makes 0 pivots; `beyond` ends INFEASIBLE with n2 = 0; `at` hands over.

The last section runs seven wrong models over every list of single_threshold_cases.ROWS (one list per kernel path or
route): each must differ from the right model, in status or trace, on at least one case of every event it touches in
EVERY list.  A mutant that survives a list means a case is missing there."""
import contextlib
from unittest import mock

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_threshold_cases as C
from tests.helpers import lp_amd

lp = lp_amd()
F32 = np.float32
SPECS = sorted({s for items in C.ROWS.values() for s in items if isinstance(s, C.Spec) and s.ev}, key=C.spec_id)
T_SPECS, P_SPECS = [s for s in SPECS if s.ev == "T"], [s for s in SPECS if s.ev == "P"]


def bits(x):
    assert isinstance(x, np.float32)
    return int(x.view(np.uint32))


def up(x):
    return np.nextafter(x, F32(np.inf))


def after(spec, pivots):
    M0, b0, is_max, _, _ = C.planted(spec).case
    return sc.solve(M0, b0, is_max, spec.f, pivots)[2] if pivots else M0


# ------------------------------------------------------------------ the thresholds themselves
def test_thresholds_are_the_librarys_and_round_where_claimed():
    eps = sc.EPS_S
    assert float(eps) == 2.0 ** -24 * (1 + 2.0 ** -23)
    for f in C.FACTORS:
        got = lp.single.thresholds(f)
        assert [bits(x) for x in got] == [bits(x) for x in sc.thresholds(f)]
        assert all(0 < x < 1 for x in got)
    assert float(sc.thresholds(1000)[0]).hex() == "0x1.f400040000000p-18"
    assert float(F32(F32(125) * F32(2.0 ** -24))).hex() == "0x1.f400000000000p-18"     # eps = 2^-24: two floats below
    assert float(F32(C.F_NO_FLOAT)) != C.F_NO_FLOAT and float(F32(C.F_NO_FLOAT)).hex() == "0x1.f426660000000p+9"
    assert sc.thresholds(C.F_NO_FLOAT) == sc.thresholds(F32(C.F_NO_FLOAT)) != sc.thresholds(1000)
    # 1000: all three products round in float; the powers of two: none does
    for f, exact in ((1024, True), (16, True), (2.0 ** 20, True), (1000, False)):
        for k, d in enumerate((8, 2, 1)):
            assert (float(sc.thresholds(f)[k]) == (f / d) * float(eps)) == exact, (f, d)


# ------------------------------------------------------------------ T
@pytest.mark.parametrize("spec", T_SPECS, ids=C.spec_id)
def test_t_case_is_what_it_claims(spec):
    p = C.planted(spec)
    M0, b0, is_max, cap, (st, tr, M, b) = p.case
    m, n, f, R, X, j, w = spec.m, spec.n, spec.f, p.R, p.X, p.j, p.w
    thr = sc.thresholds(f)[1]
    want = thr if spec.var == "at" else up(thr)
    assert bits(M0[R, X]) == bits(want) and bits(M0[R, -1]) == bits(F32(want * F32(2.0 ** -10)))
    assert not M0[R, :n][np.arange(n) != X].any()            # structural entries 0
    # X is structural and enters at step j >= 1 for the first time; before step j the trace is the base's
    assert 1 <= j < len(tr) and X < n and p.base_trace[j] == (X, w) and all(c != X for c, _ in p.base_trace[:j])
    assert tr[:j] == p.base_trace[:j] and st == sc.OPTIMAL and cap == C.CAP
    assert j % spec.mult == 0
    # after j pivots the planted entry has its bits, and R's quotient is the strict minimum
    Mj = after(spec, j)
    assert bits(Mj[R, X]) == bits(want) and sc.price(Mj, is_max, f) == X
    q = {i: F32(Mj[i, -1] / Mj[i, X]) for i in range(m) if thr < Mj[i, X] or i == R}
    assert q[R] == F32(2.0 ** -10) and all(q[R] < v for i, v in q.items() if i != R)
    # R is not the ordinary winner's row and lies where the shape says
    assert w != R and thr < Mj[w, X]
    assert R == C.t_row(m, spec.row) and (R == 0) == (spec.row == "first")
    unit = C.t_unit(m)
    if spec.row != "first":
        assert R == m - 1 or (m, R) in ((1100, 1090), (300, 290))
        if unit:
            assert R >= unit and w // unit < R // unit       # a LATER trip (1100, 300 rows) or wave than the winner's
    if spec.var == "at":                                     # `<` leaves R out, `<=` lets it in -- and it would win
        assert not thr < Mj[R, X] and thr <= Mj[R, X]
        assert tr[j] == (X, w) and sc.ratio(Mj, X, f) == w
    else:                                                    # eligible by one float: a threshold one float higher misses it
        assert thr < Mj[R, X] and not up(thr) < Mj[R, X]
        assert tr[j] == (X, R) and sc.ratio(Mj, X, f) == R
    assert np.isfinite(M).all()


# ------------------------------------------------------------------ P
@pytest.mark.parametrize("spec", P_SPECS, ids=C.spec_id)
def test_p_case_is_what_it_claims(spec):
    p = C.planted(spec)
    M0, b0, is_max, cap, (st, tr, M, b) = p.case
    m, n, f, Y = spec.m, spec.n, spec.f, p.Y
    ptol = sc.thresholds(f)[0]
    sgn = F32(1 if is_max else -1)
    edge = F32(F32(0) - ptol)
    want = edge if spec.var == "at" else np.nextafter(edge, F32(-np.inf))
    assert bits(F32(M0[m, Y] * sgn)) == bits(want) and not M0[:m, Y].any()
    assert bits(M[m, Y]) == bits(M0[m, Y]) and not M[:m, Y].any()               # bit-unchanged at the end
    key = M[m, :-1] * sgn
    assert key[Y] < np.delete(key, Y).min()                  # the strict minimum: the decision rests on it alone
    assert len(tr) == p.j >= 3 and all(c != Y for c, _ in tr) and np.isfinite(M).all()
    if spec.var == "at":
        assert not want < edge and want <= edge and st == sc.OPTIMAL
    else:
        assert want < edge and not want < np.nextafter(edge, F32(-np.inf)) and st == sc.UNBOUNDED
        assert sc.price(M, is_max, f) == Y and sc.ratio(M, Y, f) is None
    twin = C.planted(spec._replace(var="beyond" if spec.var == "at" else "at")).case[4]
    assert twin[1] == tr and {twin[0], st} == {sc.OPTIMAL, sc.UNBOUNDED}
    # a later trip than column 0's: quads beyond 1023 (1024 threads; 4100: beyond 255 too), or a later wave
    assert Y == C.p_column(n) and 0 < Y < n
    if n >= 4200:
        assert Y // 4 >= 1024
    elif n >= 300:
        assert Y // 4 >= 64


def test_the_lists_cover_what_they_name():
    for name, specs in (("256", C.PAIR_256), ("1024", C.PAIR_1024), ("lds", [s for s, _ in C.LDS_CASES]), ("steps", C.STEPWISE)):
        assert {(s.ev, s.var) for s in specs} == {(e, v) for e in "TP" for v in ("at", "beyond")}, name
        assert {s.is_max for s in specs} == {True, False} and len({s.f for s in specs}) >= 2, name
    single = C.PAIR_256 + C.PAIR_1024 + [s for s, _ in C.LDS_CASES]
    assert {s.f for s in single if s.ev == "T"} == set(C.FACTORS) == {s.f for s in single if s.ev == "P"}
    assert {(s.m, s.n) for s in C.PAIR_256} == {(300, 6), (61, 97), (96, 300)} and all(s.slack for s in C.PAIR_256)
    assert {(s.m, s.n, s.ev) for s in C.PAIR_1024} == {(1100, 6, "T"), (3, 8300, "P")} and all(s.slack for s in C.PAIR_1024)
    assert {(s.m, s.n, s.slack) for s, _ in C.LDS_CASES} == {(1100, 6, False), (3, 4200, True), (96, 300, True), (61, 97, True)}
    chunked = [s for s, chunk in C.LDS_CASES if chunk]
    assert {s.ev for s in chunked} == {"T", "P"} and all(chunk in (None, 5) for _, chunk in C.LDS_CASES)
    for s in chunked:                                        # the event step is the first of a foreign call
        assert C.planted(s).j % 5 == 0 and C.planted(s).j >= 5, C.spec_id(s)


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("shape", sorted(C.BATCHES), ids=lambda s: "%dx%d" % s[:2])
def test_batch_members_are_what_they_claim(shape):
    is_max, f, events = C.BATCHES[shape]
    specs = C.batch_specs(*shape)
    cases = C.batch_cases(*shape)
    want = [mb if mb is None else mb[:3] for mb in C.BATCH_MEMBERS if mb is None or mb[0] in events]
    assert [None if s.ev is None else (s.ev, s.var, s.row if s.ev == "T" else None) for s in specs] == want
    assert all(s.f == f and s.is_max == is_max for s in specs)                  # one factor and one sense per call
    assert len({c[0].shape for c in cases}) == 1 and all(c[3] == C.CAP and c[4][0] != sc.MAX_PIVOTS for c in cases)
    plain = [c for s, c in zip(specs, cases) if s.ev is None]
    assert len(plain) == 2 and all(c[4][0] == sc.OPTIMAL for c in plain) and not sc.same_bits(plain[0][0], plain[1][0])
    steps = [C.planted(s).j for s in specs if s.ev == "T"]
    assert len(set(steps)) >= (2 if shape[0] > 1024 else len(steps))            # the events fall at different steps
    assert len({len(c[4][1]) for c in cases}) >= 3 or events == "P"             # the members end at different times
    factors = [C.BATCHES[s][1] for s in C.BATCHES]
    assert len(set(factors)) == len(factors) and C.BATCHES[(24, 40, True)][:2] == (True, 1024)
    assert C.BATCHES[(96, 300, True)][:2] == (False, 1000)


# ------------------------------------------------------------------ F, Q
@pytest.mark.parametrize("f", C.PAIR_FACTORS)
def test_pairs_are_what_they_claim(f):
    ptol, _, feas = sc.thresholds(f)
    shapes = set()
    for name in C.BETWEEN_MEMBERS:
        (A, ab, M, mb), w = C.pair_case(name, f)
        shapes.add((A.shape, M.shape))
        phase1 = sc.solve(A, ab, False, f)
        if name in C.F_NAMES:
            obj = A[-1, -1]
            want = feas if name.endswith("at") else up(feas)
            assert bits(abs(obj)) == bits(want) and (obj > 0) == (name[1] == "+")
            assert phase1[0] == sc.OPTIMAL and phase1[1] == [] and (A[-1, :-1] <= 0).all()     # nothing to price in
            assert (ab < M.shape[1] - 1).all() and w["n1"] == 0 and w["art_trace"] == []
            if name.endswith("at"):
                assert abs(F32(F32(0) - obj)) <= feas and not abs(F32(F32(0) - obj)) < feas
                assert w["status"] == sc.OPTIMAL and w["n2"] >= 1 and not sc.same_bits(w["M"], M)   # handed over, solved
            else:
                assert not abs(F32(F32(0) - obj)) <= feas and abs(F32(F32(0) - obj)) <= up(feas)
                assert w["status"] == sc.INFEASIBLE and w["n2"] == 0 and sc.same_bits(w["M"], M)    # no hand-over
        elif name[0] == "Q":
            assert bits(A[-1, 1]) == bits(ptol if name == "Q-at" else up(ptol)) and not A[:-1, 1].any()
            assert w["art_trace"][0] == (0, 1) and bits(w["A"][-1, 1]) == bits(A[-1, 1])        # phase 1 really pivots
            if name == "Q-at":
                assert phase1[0] == sc.OPTIMAL and len(phase1[1]) == 1
                assert w["status"] == sc.OPTIMAL and (w["n1"], w["n2"]) == (1, 1)
            else:
                assert phase1[0] == sc.UNBOUNDED and len(phase1[1]) == 1 and sc.price(phase1[2], False, f) == 1
                assert w["status"] == sc.UNBOUNDED and (w["n1"], w["n2"]) == (1, 0) and sc.same_bits(w["M"], M)
        else:
            assert w["status"] == sc.OPTIMAL and (w["n1"], w["n2"]) == (1, 1)
    assert shapes == {((3, 6), (3, 5))}                      # one pair of batches holds them all


def test_public_problems_sit_on_the_edge():
    assert [r for r, _ in C.PUBLIC] == ["solve_problem", "solve_problems", "solve_lps_single"]
    assert dict(C.PUBLIC)["solve_problem"] == 16 and dict(C.PUBLIC)["solve_lps_single"] == 1000
    for _, f in C.PUBLIC:
        ptol = sc.thresholds(f)[0]
        at, beyond = (sc.solve_problem(C.edge_problem(f, var), f) for var in ("at", "beyond"))
        assert bits(C.edge_problem(f, "at")["objective"][0][1]) == bits(ptol)
        assert bits(C.edge_problem(f, "beyond")["objective"][0][1]) == bits(up(ptol))
        assert (at["status"], at["pivots"], sc.objective(at["M"])) == (sc.OPTIMAL, 0, 0)
        assert (beyond["status"], beyond["pivots"]) == (sc.OPTIMAL, 1) and bits(sc.objective(beyond["M"])) == bits(up(ptol))
        # under the default factor both would read otherwise on at least one side
        assert [sc.solve_problem(C.edge_problem(f, var))["pivots"] for var in ("at", "beyond")] != [0, 1]


# ------------------------------------------------------------------ the cases tell seven wrong models from the right one
def _price(strict):
    def price(M, is_max, factor=1024):
        ptol = sc.thresholds(factor)[0]
        obj, vc = M[-1], M.shape[1] - 1
        if vc < 1:
            return None
        col = 0
        for i in range(1, vc):
            if (obj[i] < obj[col]) if is_max else (obj[i] > obj[col]):
                col = i
        lo, hi = F32(F32(0) - ptol), F32(F32(0) + ptol)
        if strict:
            return col if ((obj[col] < lo) if is_max else (obj[col] > hi)) else None
        return col if ((obj[col] <= lo) if is_max else (obj[col] >= hi)) else None
    return price


def _ratio(strict):
    def ratio(M, ec, factor=1024):
        thr, vc = sc.thresholds(factor)[1], M.shape[1] - 1
        best, bq = None, None
        with np.errstate(all="ignore"):
            for i in range(M.shape[0] - 1):
                a = M[i, ec]
                if (thr < a) if strict else (thr <= a):
                    q = F32(M[i, vc] / a)
                    if best is None or q < bq:
                        best, bq = i, q
        return best
    return ratio


def _thresholds_with(eps):
    def thresholds(factor=1024):
        f = F32(factor)
        return (F32(F32(f / F32(8)) * eps), F32(F32(0) + F32(F32(f / F32(2)) * eps)), F32(f * eps))
    return thresholds


_RIGHT = sc.thresholds


def _double_thresholds(factor=1024):
    eps = 2.0 ** -53 * (1 + 2.0 ** -52)                      # double-float-epsilon
    f = float(factor)
    return F32((f / 8.0) * eps), F32(0.0 + (f / 2.0) * eps), F32(f * eps)


# name: (what is patched in the model, the events it can change)
MUTANTS = {
    "a: <= in pricing": (dict(price=_price(False)), "P"),
    "b: <= in the ratio test": (dict(ratio=_ratio(False)), "T"),
    "c: < in the feasibility test": (None, "F"),
    "d: eps = 2^-24": (dict(thresholds=_thresholds_with(F32(2.0 ** -24))), "TPF"),
    "e: eps = FLT_EPSILON": (dict(thresholds=_thresholds_with(np.finfo(F32).eps)), "TPF"),
    "f: the factor fixed at 1024": (dict(thresholds=lambda factor=1024: _RIGHT(1024)), "TPF"),
    "g: thresholds from the double formula": (dict(thresholds=_double_thresholds), "TPF"),
}


def _strict_feasibility_answer(item):
    """Mutant c, `<` for `<=` in (fp= 0 objective): where phase 1 ends OPTIMAL with |0 - objective| EQUAL to the
    threshold it says INFEASIBLE without a hand-over; everywhere else `<` and `<=` agree."""
    right = C.answer(item)
    if isinstance(item, C.Spec) or item[0] in ("at", "beyond"):
        return right
    (A, ab, M, mb), _ = C.pair_case(*item)
    st, t1, A1, _ = sc.solve(A, ab, False, item[1])
    if st == sc.OPTIMAL and abs(F32(F32(0) - A1[-1, -1])) == sc.thresholds(item[1])[2]:
        return sc.INFEASIBLE, C._pairs(t1), []
    return right


def _mutant_answer(name, item):
    patches, _ = MUTANTS[name]
    if patches is None:
        return _strict_feasibility_answer(item)
    with contextlib.ExitStack() as stack:
        for attr, fn in patches.items():
            stack.enter_context(mock.patch.object(sc, attr, fn))
        return C.answer(item)


def test_the_copies_of_the_scans_reproduce_the_model():
    items = [C.PAIR_256[4], C.PAIR_256[7], ("Q-beyond", 1000), ("F+at", 1024)]
    for item in items:
        right = C.answer(item)                               # (builds and caches the case under the right model)
        with mock.patch.object(sc, "price", _price(True)), mock.patch.object(sc, "ratio", _ratio(True)), \
                mock.patch.object(sc, "thresholds", _thresholds_with(sc.EPS_S)):
            assert C.answer(item) == right
    assert sc.thresholds is _RIGHT


@pytest.mark.parametrize("row", sorted(C.ROWS))
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_wrong_model_differs_on_every_list(mutant, row):
    items = C.ROWS[row]
    right = [C.answer(item) for item in items]               # first: the cases are built and cached under the right model
    events = {C.event_of(item) for item in items} - {None}
    assert events
    for ev in MUTANTS[mutant][1]:
        if ev not in events:
            continue
        killed = [item for item, r in zip(items, right) if C.event_of(item) == ev and _mutant_answer(mutant, item) != r]
        assert killed, "%s survives the %s cases of %s" % (mutant, ev, row)
    assert sc.thresholds is _RIGHT
