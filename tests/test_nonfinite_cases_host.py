"""tests/nonfinite_cases.py checked on the oracle alone (no GPU): every case tests/test_gpu_nonfinite.py uses is what
it claims -- the trace before step j is the base's, nothing non-finite has spread before step j, the named row
wins at step j, the solve ends where the case says, and the row, slot or column that carries the event sits
where the case says (workgroup, wave, lane, strip, shard).  These are conditions on the INPUTS: a seed that
fails one is replaced in nonfinite_cases.SEEDS, never excused.

A NumPy restatement of the two scans replays every case with the reference's rules (it must give the oracle's
trace) and with the rules a wrong kernel could follow -- a ratio test that lets ANY NaN quotient win, a pricing
step that stops at a NaN in ANY column, one that ignores the NaN in column 0, one that looks at SLOT 0 instead
of logical column 0: each must give another trace or another end on the cases meant for it, so a kernel that
followed it could not pass the GPU tests."""
import functools

import numpy as np
import pytest

import oracle
from tests import nonfinite_cases as nc

ALL = nc.SINGLE + sorted(set(c for _, c in nc.COLPART) - set(nc.SINGLE), key=nc.case_id)
RESIDENT_SHAPES = {(1024, 512), (2048, 200)}


def _last_place(index, size, per):
    """In the last look-ahead workgroup, not in lane 0, and not in its first wave if it has a usable later one."""
    wg, wave, lane = nc.place(index, per)
    last = nc.place(size - 1, per)[0]
    later = [i for i in range(size - 1) if nc.place(i, per)[0] == last and nc.place(i, per)[1] != 0 and nc.place(i, per)[2] != 0]
    return wg == last and lane != 0 and (wave != 0 or not later)


def _slot(case, col):
    """Slot of a structural column that has not moved: the non-basic columns in logical order."""
    return col - (1 if (case.basic0 or (case.ev, case.var) == ("S0", "col0")) else 0)


@functools.lru_cache(maxsize=None)
def _non_finite_at(case, cap):
    """Positions of the non-finite entries after `cap` pivots of the oracle."""
    p = nc.planted(case)
    M = nc.solve(p.M, p.basis, case.kind, cap).M if cap else p.M
    return tuple(map(tuple, np.argwhere(~np.isfinite(M))))


# ------------------------------------------------------------------------------------------ the scans, restated
def _price(obj, sgn, tol, slots, rule):
    """-> entering column or -1.  rule: "reference" | "any-nan-stops" | "ignore-nan0" | "slot0"."""
    key = obj * sgn                                        # key space: the most negative key enters
    nan = np.isnan(key)
    if rule == "reference" and nan[0]:
        return -1                                          # nothing replaces a NaN incumbent, (fp< NaN 0) fails
    if rule == "any-nan-stops" and nan.any():
        return -1
    if rule == "slot0" and nan.any() and (slots[nan] == 0).any():
        return -1
    if nan.all():
        return -1
    best = int(np.flatnonzero(~nan)[np.argmin(key[~nan])])  # first index of the strict minimum among the numbers
    return best if key[best] < 0.0 - tol else -1


def _ratio(a, rhs, thr, rule):
    """-> pivot row or -1.  rule: "reference" | "any-nan-wins"."""
    with np.errstate(all="ignore"):
        el = np.flatnonzero(thr < a)
        if not len(el):
            return -1
        q = rhs[el] / a[el]
    nan = np.isnan(q)
    if rule == "reference" and nan[0]:
        return int(el[0])                                  # the first eligible row: nothing is smaller than a NaN
    if rule == "any-nan-wins" and nan.any():
        return int(el[np.flatnonzero(nan)[0]])
    el, q = el[~nan], q[~nan]                              # a NaN quotient never replaces the incumbent
    return int(el[np.argmin(q)])


def _replay(case, cap, price_rule="reference", ratio_rule="reference", factor=1024.0):
    p = nc.planted(case)
    M, b = p.M.copy(), p.basis.copy()
    m, vc = M.shape[0] - 1, M.shape[1] - 1
    sgn = 1.0 if case.kind == "max" else -1.0
    tol, thr = (factor / 8.0) * oracle.EPSILON, 0.0 + (factor / 2.0) * oracle.EPSILON
    slots = np.full(vc, -1, dtype=np.int64)
    nonbasic = np.setdiff1d(np.arange(vc), b)
    slots[nonbasic] = np.arange(len(nonbasic))
    trace, status = [], oracle.MAX_PIVOTS
    while True:
        ec = _price(M[m, :vc], sgn, tol, slots, price_rule)
        if ec < 0:
            status = oracle.OPTIMAL
            break
        if len(trace) >= cap:
            break
        cr = _ratio(M[:m, ec], M[:m, vc], thr, ratio_rule)
        if cr < 0:
            status = oracle.UNBOUNDED
            break
        slots[b[cr]], slots[ec] = slots[ec], -1
        with np.errstate(all="ignore"):
            oracle.pivot(M, b, ec, cr, omp=M.size > 4_000_000)
        trace.append((ec, cr))
    return status, np.array(trace, dtype=np.int64).reshape(-1, 2), slots


def _differs(case, cap, **rules):
    ref = nc.reference(case, cap)
    st, tr, _ = _replay(case, cap, **rules)
    return st != ref.status or not np.array_equal(tr, ref.trace)


# ------------------------------------------------------------------------------------------ single tableaux
@pytest.mark.parametrize("case", ALL, ids=nc.case_id)
def test_case_is_what_it_claims(case):
    n, m, ev, var, j = case[:5]
    p = nc.planted(case)
    cap = nc.cap_of(case)
    ref = nc.reference(case)
    bt = p.base_trace
    short = j + 2                                          # the replays: two steps past the event show every rule
    # the restated scans ARE the oracle's
    st, tr, slots = _replay(case, short)
    rs = nc.reference(case, short)
    assert st == rs.status and np.array_equal(tr, rs.trace) and np.array_equal(rs.trace, ref.trace[:short])
    if ev == "S0":
        return _s0(case, p, ref, slots)
    # before step j: the base's trace, and nothing non-finite has spread
    assert np.array_equal(ref.trace[:j], bt[:j])
    assert _non_finite_at(case, j) == _non_finite_at(case, 0)
    if ev != "Q" or var[1] == "first":                     # ... and pivot j spreads it (an ignored NaN quotient stays where it is)
        assert len(_non_finite_at(case, j + 1)) > len(_non_finite_at(case, 0))
    if ev in ("C", "Q"):
        R, X = p.R, p.X
        assert X not in bt[:j, 0] and bt[j, 0] == X and R not in bt[:, 1]      # X enters at j for the first time; R is isolated
        nan_quotient_first = ev == "Q" and var[1] == "first"
        wins = R if (nan_quotient_first or (ev, var) == ("C", "+inf")) else int(bt[j, 1])
        assert tuple(ref.trace[j]) == (X, wins)
        assert (ref.status, ref.pivots) == (oracle.MAX_PIVOTS, cap)
        assert np.isnan(ref.M).any()
        # geometry: X's slot, and R unless the case pins it to row 0 / m - 1
        assert _last_place(_slot(case, X), n, 2)
        if ev == "C" or var[1] == "mid":
            assert _last_place(R, m, 1) and R < m - 1
        if m > 256 and not nan_quotient_first:             # the step's winner in another workgroup than the event's row
            assert wins // 256 != R // 256 or wins == R
        if ev == "Q":
            planted_at_j = nc.solve(p.M, p.basis, case.kind, j).M
            el = np.flatnonzero(planted_at_j[:m, X] > 512 * oracle.EPSILON)
            assert R in el and len(el) > 2
            if var[1] == "first":
                assert el[0] == R == 0
                if m > 256:
                    assert int(bt[j, 1]) // 256 != 0       # the row that would win without the NaN: another workgroup
            else:
                assert el[0] < R and (var[1] == "last" or el[-1] > R)
                if m > 256:
                    assert el[0] // 256 != R // 256        # the first eligible row and the NaN row: different workgroups
                assert _differs(case, short, ratio_rule="any-nan-wins")
    else:
        Y, Rj = p.Y, p.Rj
        assert Rj not in bt[:j, 1] and bt[j, 1] == Rj and Y not in bt[:, 0]
        assert tuple(ref.trace[j]) == tuple(bt[j])
        assert _last_place(Rj, m, 1)
        after = nc.solve(p.M, p.basis, case.kind, j + 1).M
        assert np.isnan(after[m, Y])                       # inf - inf in the objective entry
        if ev == "Z0":
            assert Y == 0 and (ref.status, ref.pivots) == (oracle.OPTIMAL, j + 1)
            assert _differs(case, short, price_rule="ignore-nan0")
        else:
            assert Y != 0 and (ref.status, ref.pivots) == (oracle.MAX_PIVOTS, cap) and np.array_equal(ref.trace, bt[:cap])
            assert np.isinf(after[:, Y]).any() and np.isnan(after[:, Y]).any() and np.isnan(ref.M[:, Y]).any()
            assert _differs(case, short, price_rule="any-nan-stops")
            if case.basic0:                                # the NaN arises in SLOT 0, which holds logical column 1
                assert (Y, slots[Y]) == (1, 0) and _differs(case, short, price_rule="slot0")
            elif var is not None:                          # the first column of a later shard
                count = n + m if case.dense else n
                assert var[2] > 0 and Y == nc.r_start(count, var[1], var[2])
            else:
                assert _last_place(Y, n, 2)
            if (n, m) in RESIDENT_SHAPES and not case.basic0:
                Xj = int(bt[j, 0])                         # strips of 64 slots: the step's entering column in another one,
                assert Xj < n and Xj not in bt[:j, 0] and Xj // 64 != Y // 64 and Y % 64 >= 40   # Y among a strip's last 24 (LDS with lds 1)


def _s0(case, p, ref, slots):
    n, m = case.n, case.m
    r1, r3, d1, u = p.R, p.Rj, p.X, p.Y
    assert [tuple(t) for t in ref.trace[:3]] == [(d1, r1), (d1 - 1, r1 + 1), (d1 - 2, r3)]
    assert _slot(case, d1) == n - 1 and slots[u] == n - 1  # u left into the LAST slot and stayed there
    assert nc.place(n - 1, 2)[2] != 0 and _last_place(r3, m, 1)
    two = nc.solve(p.M, p.basis, case.kind, 2).M
    assert np.isinf(two[m, u]) and np.isfinite(np.delete(two[m], [u, two.shape[1] - 1])).all()
    assert np.isnan(ref.M[m, u])
    if case.var == "col0":
        assert u == 0 and (ref.status, ref.pivots) == (oracle.OPTIMAL, nc.S0_PIVOTS)
        assert _differs(case, 5, price_rule="slot0") and _differs(case, 5, price_rule="ignore-nan0")
    else:
        assert u != 0 and (ref.status, ref.pivots) == (oracle.MAX_PIVOTS, nc.cap_of(case))
        assert _differs(case, 5, price_rule="any-nan-stops")


def test_every_event_meets_every_path_after_step_zero():
    for name, cases in (("per-pivot", nc.PER_PIVOT), ("two-launch", [c for c, _ in nc.TWO_LAUNCH]),
                        ("persistent", [c for c, _, _ in nc.PERSISTENT]), ("resident", [c for c, _ in nc.RESIDENT]),
                        ("column partitions", [c for _, c in nc.COLPART])):
        assert {c.ev for c in cases if c.j > 0} >= {"C", "Q", "Z0", "ZY"}, name
    assert {c.ev for c in nc.WIDE if c.j > 0} == {"C", "ZY"}
    for wg in (3, 17, 33):
        assert {c.ev for c, w, _ in nc.PERSISTENT if w == wg and c.j > 0} >= {"C", "Q", "Z0", "ZY"} or wg == 33
    assert {c.ev for c, w, _ in nc.PERSISTENT if w == 33} >= {"C", "Q", "Z0", "ZY"}
    for c, wg, block in nc.PERSISTENT:
        assert (max(c.m, (c.n + 1) // 2) + 255) // 256 == wg


# ------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("kind", ["max", "min"])
@pytest.mark.parametrize("shape", nc.BATCH_SHAPES, ids=["%dx%d" % s for s in nc.BATCH_SHAPES])
def test_batch_members_are_what_they_claim(shape, kind):
    Ms, Bs, cases = nc.batch(*shape, kind)
    refs = nc.batch_reference(*shape, kind, nc.BATCH_CAP)
    assert len({c.j for c in cases if c}) == 4             # the events fall at different steps
    for k, (case, ref) in enumerate(zip(cases, refs)):
        if case is None:
            assert ref.status == oracle.OPTIMAL and np.isfinite(Ms[k]).all() and np.isfinite(ref.M).all()
            continue
        p, j = nc.planted(case), case.j
        assert np.array_equal(ref.trace[:j], p.base_trace[:j]) and ref.pivots > j, k
        assert _non_finite_at(case, j) == _non_finite_at(case, 0)
        if case.ev == "Z0":
            assert (ref.status, ref.pivots) == (oracle.OPTIMAL, j + 1) and tuple(ref.trace[j]) == tuple(p.base_trace[j])
        else:
            first = case.ev == "Q" and case.var[1] == "first"
            assert tuple(ref.trace[j]) == (p.X, p.R if first else int(p.base_trace[j, 1])), k
            assert np.isnan(ref.M).any()
            if case.ev == "Q" and not first:
                assert _differs(case, j + 2, ratio_rule="any-nan-wins")
    assert len({r.pivots for r in refs}) > 3               # the members end at different times
