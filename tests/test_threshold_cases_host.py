"""tests/threshold_cases.py checked on the oracle alone (no GPU): every case tests/test_gpu_thresholds.py uses is what
it claims, and a kernel that followed another rule -- `<=` for `<` in the ratio test or in the pricing test, a
threshold one ulp off -- would give another trace or another end on it.  These are conditions on the INPUTS: a
seed that fails one is replaced in threshold_cases.TSEEDS / PSEEDS, never excused.

T: after j pivots of the oracle M[R, X] is still bitwise the planted value and b[R] / M[R, X] is exactly 2**-10,
strictly below the quotient of the row the oracle picks; `at`: thr < M[R, X] fails and thr <= M[R, X] holds, so a
`<=` kernel pivots on R where the oracle keeps the base's row; `beyond`: thr < M[R, X] holds and fails for the next
double above thr, so a kernel whose threshold is one ulp higher misses R where the oracle pivots on it.
P: after k_end pivots Y's key is bitwise -ptol (`at`) or its predecessor (`beyond`) and the STRICT minimum of all
keys: the decision rests on it alone; OPTIMAL against UNBOUNDED after the same pivots."""
import numpy as np
import pytest

import oracle
from tests import threshold_cases as tc
from tests.test_nonfinite_cases_host import _last_place

ALL = tc.SINGLE + sorted(set(c for _, c in tc.COLPART) - set(tc.SINGLE), key=tc.case_id)
T_STEPS = {5, 15, 16, 19, 23, 24, 27}


def _bits(x):
    return np.float64(x).view(np.int64)


def _after(case, pivots):
    p = tc.planted(case)
    return tc.solve(p.M, p.basis, case.kind, pivots, case.f).M if pivots else p.M


def _check_t(case):
    n, m, j, f = case.n, case.m, case.j, case.f
    p, ref = tc.planted(case), tc.reference(case)
    thr, _ = tc.thresholds(f)
    R, X, bt = p.R, p.X, p.base_trace
    is_max = case.kind == "max"
    # X enters at step j for the first time, R is isolated; before step j the trace is the base's
    assert X not in bt[:j, 0] and bt[j, 0] == X and R not in bt[:, 1] and not p.M[R, :n][np.arange(n) != X].any()
    assert ref.pivots > j and np.array_equal(ref.trace[:j], bt[:j])
    # the planted entry has not moved, the quotient is exactly 2**-10
    M = _after(case, j)
    a = M[R, X]
    assert _bits(a) == _bits(thr if case.var == "at" else np.nextafter(thr, np.inf)) and _bits(a) == _bits(p.M[R, X])
    assert M[R, -1] / a == 2.0 ** -10
    w = int(bt[j, 1])                                      # the row that wins without R
    assert thr < M[w, X] and 2.0 ** -10 < M[w, -1] / M[w, X]
    assert oracle.price(np.ascontiguousarray(M), is_max, f) == X
    if case.var == "at":                                   # `<` leaves R out, `<=` lets it in -- and it would win
        assert not thr < a and thr <= a
        assert tuple(ref.trace[j]) == (X, w) == tuple(bt[j]) and oracle.ratio(np.ascontiguousarray(M), X, f) == w
    else:                                                  # eligible by one ulp: a threshold one ulp higher misses it
        assert thr < a and not np.nextafter(thr, np.inf) < a
        assert tuple(ref.trace[j]) == (X, R) and oracle.ratio(np.ascontiguousarray(M), X, f) == R
    # finite to the end: no hand-over to the dense path
    assert np.isfinite(ref.M).all()
    # geometry
    assert _last_place(X, n, 2)
    if case.row == "target":
        assert _last_place(R, m, 1) and R < m - 1
    else:
        assert R == (0 if case.row == "first" else m - 1)
    if m > 256:
        assert w // 256 != R // 256


def _check_p(case):
    n, m, j, f = case.n, case.m, case.j, case.f
    p, ref = tc.planted(case), tc.reference(case)
    _, ptol = tc.thresholds(f)
    Y = p.Y
    sgn = 1.0 if case.kind == "max" else -1.0
    assert j >= 3
    M = _after(case, j)
    key = sgn * M[m, :-1]
    assert _bits(key[Y]) == _bits((0.0 - ptol) if case.var == "at" else np.nextafter(0.0 - ptol, -np.inf))
    assert key[Y] < np.delete(key, Y).min()                # the strict minimum: the decision rests on it alone
    assert not M[:m, Y].any()
    if case.var == "at":
        assert not key[Y] < 0.0 - ptol and key[Y] <= 0.0 - ptol
        assert (ref.status, ref.pivots) == (oracle.OPTIMAL, j)
    else:
        assert key[Y] < 0.0 - ptol and not key[Y] < np.nextafter(0.0 - ptol, -np.inf)
        assert (ref.status, ref.pivots) == (oracle.UNBOUNDED, j)
    twin = tc.reference(case._replace(var="beyond" if case.var == "at" else "at"))
    assert twin.pivots == j and twin.status != ref.status and twin.status in (oracle.OPTIMAL, oracle.UNBOUNDED)
    assert np.array_equal(twin.trace, ref.trace)
    assert np.isfinite(ref.M).all()
    if case.shard:                                         # the first column of a later shard
        assert case.shard[1] > 0 and Y == tc.r_start(n + m if case.dense else n, *case.shard)
    else:
        assert _last_place(Y, n, 2)


def _check(case):
    (_check_t if case.ev == "T" else _check_p)(case)


@pytest.mark.parametrize("case", ALL, ids=tc.case_id)
def test_case_is_what_it_claims(case):
    _check(case)


def test_the_lists_cover_what_they_name():
    blocked = [(c, b) for c, b, _ in tc.TWO_LAUNCH] + [(c, b) for c, _, b, _ in tc.PERSISTENT]
    for case, block in blocked:
        assert block in (16, 24)
        if case.ev == "P":                                 # k_end where the case says, in the block of its path
            assert case.pos == tc.position(case.j, block), (tc.case_id(case), block)
    for block in (16, 24):
        assert {c.pos for c, b in blocked if c.ev == "P" and b == block} >= {"first", "last"}
    assert "mid" in {c.pos for c, _ in blocked}
    families = {"per-pivot": tc.PER_PIVOT, "two-launch": [c for c, _, _ in tc.TWO_LAUNCH], "persistent": [c for c, _, _, _ in tc.PERSISTENT],
                "wide": tc.WIDE, "resident": [c for c, _ in tc.RESIDENT], "column partitions": [c for _, c in tc.COLPART]}
    for name, cases in families.items():
        assert {(c.ev, c.var) for c in cases} >= {("T", "at"), ("P", "at")}, name
        assert tc.F_ROUNDS in {c.f for c in cases} and tc.F in {c.f for c in cases}, name
        if name != "wide":
            assert {(c.ev, c.var) for c in cases} >= {("T", "beyond"), ("P", "beyond")}, name
    every = [c for cases in families.values() for c in cases]
    assert {c.f for c in every} == {tc.F, tc.F_SMALL, tc.F_LARGE, tc.F_ROUNDS}
    assert {c.j for c in every if c.ev == "T"} >= T_STEPS
    assert {c.row for c in every if c.ev == "T"} == {"target", "first", "last"}
    assert 0 in {c.j for c, _, _, _ in tc.PERSISTENT if c.ev == "T"}
    # the products that round, and the ones that do not
    eps = np.float64(oracle.EPSILON)
    for f, exact in ((tc.F, True), (tc.F_SMALL, True), (tc.F_LARGE, True), (tc.F_ROUNDS, False)):
        for d in (2, 8):
            num, den = (int(f) // d) * int(eps.as_integer_ratio()[0]), int(eps.as_integer_ratio()[1])
            got = np.float64(f / d * eps).as_integer_ratio()
            assert (got[0] * den == num * got[1]) == exact, (f, d)
    for case, wg, block, _ in tc.PERSISTENT:
        assert (max(case.m, (case.n + 1) // 2) + 255) // 256 == wg
    assert {(wg, c.ev) for c, wg, _, _ in tc.PERSISTENT} == {(wg, ev) for wg in (3, 17, 33) for ev in "TP"}
    big = [c for c, _, _, _ in tc.PERSISTENT if (c.n, c.m) == (64, 8300)]
    assert sorted(c.ev for c in big) == ["P", "T"] and all(tc.cap_of(c) == 40 for c in big)


@pytest.mark.parametrize("shards,case", tc.COLPART, ids=["s%d-%s" % (s, tc.case_id(c)) for s, c in tc.COLPART])
def test_column_partition_placement(shards, case):
    count = case.n + case.m if case.dense else case.n      # compact shards deal out the slots, dense ones all columns
    p = tc.planted(case)
    if case.ev == "T":                                     # X is owned by the last shard
        assert tc.r_start(count, shards, shards - 1) <= p.X < count
    else:                                                  # Y is the FIRST column of shard r > 0
        assert case.shard[0] == shards and 0 < case.shard[1] < shards
        assert p.Y == tc.r_start(count, shards, case.shard[1]) and p.Y < case.n


# ------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("shape", tc.BATCH_SHAPES, ids=["%dx%d" % s for s in tc.BATCH_SHAPES])
def test_batch_members_are_what_they_claim(shape):
    kind, f = tc.BATCH_KIND_FACTOR[shape]
    Ms, Bs, cases = tc.batch(*shape, kind)
    refs = tc.batch_reference(*shape, kind, tc.BATCH_CAP)
    assert len(cases) == 8 and [c is None for c in cases].count(True) == 2
    assert len({c.j for c in cases if c}) == 6             # the events fall at different steps
    assert [(c.ev, c.var, c.row) for c in cases if c] == [("T", "at", "target"), ("T", "beyond", "first"), ("T", "beyond", "last"),
                                                          ("P", "at", "target"), ("P", "beyond", "target"), ("T", "at", "first")]
    for k, (case, ref) in enumerate(zip(cases, refs)):
        assert np.isfinite(ref.M).all() and ref.status != oracle.MAX_PIVOTS, k
        if case is None:
            assert ref.status == oracle.OPTIMAL and np.isfinite(Ms[k]).all()
            continue
        assert case.f == f and case.kind == kind           # one factor per call
        _check(case)
        short = tc.reference(case)
        assert np.array_equal(ref.trace[:short.pivots], short.trace) and ref.pivots >= short.pivots, k
    assert len({r.pivots for r in refs}) > 3               # the members end at different times
    factors = [tc.BATCH_KIND_FACTOR[s][1] for s in tc.BATCH_SHAPES]
    assert all(a != b for a, b in zip(factors, factors[1:])) and tc.F_ROUNDS in factors
