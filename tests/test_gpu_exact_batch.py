"""Batches of exact rational LPs on the GPU (mi355x_xbatch_*, mi355x_solve_problems(exact=True)): one
workgroup per member (kernels_exact_batch.inc) against the Fraction oracle (oracle/rational_ref.py) and the
fraction-free model (tests/exact_cases.py) -- per member the status, the pivot sequence, the basis, every
final entry and the width -- never against the library's own one-tableau path, except where a test is
about the two agreeing."""
import ctypes
import functools
import threading
from fractions import Fraction

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi
pytestmark = pytest.mark.gpu
WG = capi.XBATCH_WORKGROUP
CODES = {"optimal": capi.MI_OPTIMAL, "unbounded": capi.MI_UNBOUNDED, "infeasible": capi.MI_INFEASIBLE,
         "art_nonzero": capi.MI_ART_NONZERO, "art_stuck": capi.MI_ART_STUCK, "max_pivots": capi.MI_MAX_PIVOTS}
_ERRORS = {"unbounded": lp.UnboundedProblemError, "infeasible": lp.InfeasibleProblemError,
           "art_nonzero": lp.SolverError, "art_stuck": lp.SolverError}
PERIOD = [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (5, 1)]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pairs(a):
    return [tuple(x) for x in a.tolist()]


def _trace(sol):
    return ([] if sol.phase1 is None else _pairs(sol.phase1.pivot_trace())) + _pairs(sol.pivot_trace())


@functools.lru_cache(maxsize=None)
def _reference(kind, *args):
    """(problem, oracle status, oracle trace, oracle final tableau, model stats, n1) of a generated problem,
    computed once per session."""
    p = getattr(ec, kind)(lp, *args)
    tabs = rr.build_tableau(ec.to_dict(p))
    st, trace, t = ec.oracle_outcome(tabs)
    keep = {}
    _, mtrace, _, stats = ec.model_solve(tabs, keep=keep)
    assert stats["max_bits"] > 128 or (mtrace == trace and not stats["inexact"])
    return p, st, trace, t, stats, keep.get("n1", 0)


def _check_member(ref, got):
    """A member of mi355x_solve_problems(exact=True, errorp=False) against its reference."""
    p, st, trace, t, stats, n1 = ref
    if stats["max_bits"] > 128:
        assert isinstance(got, lp.UnsupportedConstraintError)
        return
    if st != "optimal":
        assert isinstance(got, _ERRORS[st]) and not isinstance(got, lp.UnsupportedConstraintError), (st, got)
        return
    assert isinstance(got, lp.ExactTableau), got
    assert _trace(got) == trace
    assert got.basis_columns.tolist() == t.basis
    assert got.matrix.tolist() == t.matrix
    bits = 64 if stats["max_bits"] <= 64 else 128
    assert got.bits == bits and (got.phase1 is None or got.phase1.bits == bits)
    if got.phase1 is None:
        assert got.n_pivots == len(trace)
    else:
        assert tuple(got.n_pivots) == (n1 + stats["driveouts"], len(trace) - n1)
        assert _pairs(got.phase1.pivot_trace()) == trace[:n1]
    assert lp.solution_objective_value(got) == rr.objective_value(t)
    for v in p.vars:
        x = lp.solution_variable(got, v)
        assert isinstance(x, Fraction) and x == rr.tableau_variable(t, v)


def _batches(problems, min_bits=0):
    """(XBatch,) or (art XBatch, main XBatch) and the members' tableaux of problems of one shape."""
    tabs = [lp.build_tableau(p, exact=True) for p in problems]
    if isinstance(tabs[0], list):
        return (lp.exact.XBatch([t[0] for t in tabs], min_bits=min_bits),
                lp.exact.XBatch([t[1] for t in tabs], min_bits=min_bits)), tabs
    return (lp.exact.XBatch(tabs, min_bits=min_bits),), tabs


def _download(xb, q):
    """(T as Python ints, D, basis, bits, trace, trace count) of member q through the C ABI."""
    L = capi.lib()
    R, C = xb.rows, xb.cols
    T = np.empty(R * C * 2, dtype=np.int64)
    D = np.empty(2, dtype=np.int64)
    b = np.empty(R - 1, dtype=np.int64)
    assert L.mi355x_xbatch_download(xb.handle, q, _ptr(T), _ptr(D), _ptr(b)) == capi.MI_OK
    lo, hi = T[0::2].reshape(R, C), T[1::2].reshape(R, C)
    bits = ctypes.c_int(0)
    assert L.mi355x_xbatch_bits(xb.handle, q, ctypes.byref(bits)) == capi.MI_OK
    n = ctypes.c_int64(0)
    cap = capi.XBATCH_TRACE_CAP + 8
    e, r = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64)
    assert L.mi355x_xbatch_trace(xb.handle, q, _ptr(e), _ptr(r), cap, ctypes.byref(n)) == capi.MI_OK
    k = min(n.value, capi.XBATCH_TRACE_CAP)
    assert (e[k:] == -7).all() and (r[k:] == -7).all()
    return (lo, hi), lp.exact._int128(D[0], D[1]), b.tolist(), bits.value, list(zip(e[:k].tolist(), r[:k].tolist())), n.value


def _same_entries(lohi, model_T):
    lo, hi = lohi
    if isinstance(model_T, np.ndarray) and model_T.dtype == np.int64:
        return bool(np.array_equal(lo, model_T) and np.array_equal(hi, model_T >> 63))
    want = model_T.tolist() if isinstance(model_T, np.ndarray) else model_T
    got = [[lp.exact._int128(a, b) for a, b in zip(rl, rh)] for rl, rh in zip(lo.tolist(), hi.tolist())]
    return got == [[int(x) for x in row] for row in want]


# ---- 1. mixed widths in one single-phase group ----------------------------------------------------------
WIDE = [(s, e) for e in (10, 40, 60) for s in range(6)]


def test_mixed_widths_in_one_single_phase_group():
    refs = [_reference("wide_problem", s, e) for s, e in WIDE]
    for (s, e), ref in zip(WIDE, refs):
        mb = ref[4]["max_bits"]
        if e == 10:
            assert 21 <= mb <= 33
        elif e == 40:
            assert 82 <= mb <= 122
        else:
            assert mb == 182 if s == 2 else 122 <= mb <= 123
    ps = [r[0] for r in refs]
    (xb,), tabs = _batches(ps)
    assert tabs[0]._matrix.shape == (5, 9)
    rc, st, npv = xb.solve(True, 0)
    assert rc == capi.MI_OK
    want = [capi.MI_EXACT_OVERFLOW if r[4]["max_bits"] > 128 else CODES[r[1]] for r in refs]
    assert st.tolist() == want and want.count(capi.MI_EXACT_OVERFLOW) == 1
    widths = []
    for q, r in enumerate(refs):
        if want[q] != capi.MI_OPTIMAL:
            continue
        _, D, basis, bits, trace, n = _download(xb, q)
        assert trace == r[2] and n == len(trace) == npv[q] and basis == r[3].basis
        widths.append(bits)
    assert widths.count(64) == 6 and widths.count(128) == 11
    got = lp.solve_problems(ps, exact=True, errorp=False)
    for r, g in zip(refs, got):
        _check_member(r, g)
    assert sum(isinstance(g, lp.UnsupportedConstraintError) for g in got) == 1
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problems(ps, exact=True)


# ---- 2. / 7. a two-phase group with drive-outs and negative pivots, in one call and in bounded calls ---------
def _mixed_refs():
    refs = [_reference("mixed_problem", 6, 3, 2, 1, s) for s in range(24)]
    for r in refs:
        assert r[1] == "optimal" and r[4]["driveouts"] == 2 and r[4]["negative_pivots"] == 2
    return refs


def test_two_phase_group_with_driveouts_and_negative_pivots():
    refs = _mixed_refs()
    got = lp.solve_problems([r[0] for r in refs], exact=True)
    assert got[0].phase1._matrix.shape == (11, 19) and got[0]._matrix.shape == (11, 14)
    assert got[0]._batch[0] is got[23]._batch[0] and got[0].phase1._batch[0] is got[23].phase1._batch[0]
    for r, g in zip(refs, got):
        _check_member(r, g)


def _one_pivot_per_call(xa, xm, refs):
    """mi355x_xbatch_solve_two_phase with max_pivots = 1 until no member is left: per member the sums of
    the calls' counts; no call counts more than one pivot (or one between-phases step's drive-outs)."""
    total = np.zeros((len(refs), 2), dtype=np.int64)
    most = max(len(r[2]) + r[4]["driveouts"] for r in refs)
    for calls in range(most + 3):
        rc, st, npv = xa.solve_two_phase(xm, True, 1)
        assert rc == capi.MI_OK
        total += npv
        for q, r in enumerate(refs):
            assert npv[q].sum() <= max(1, r[4]["driveouts"])
        if not (st == capi.MI_MAX_PIVOTS).any():
            break
    assert (st == capi.MI_OPTIMAL).all()
    return total


def _check_two_phase_batch(xa, xm, refs, total, min_bits=0):
    for q, (p, st, trace, t, stats, n1) in enumerate(refs):
        assert tuple(total[q]) == (n1 + stats["driveouts"], len(trace) - n1)
        _, _, _, abits, atrace, an = _download(xa, q)
        lohi, D, basis, bits, mtrace, mn = _download(xm, q)
        assert atrace + mtrace == trace and an == n1
        assert abits == bits == (64 if stats["max_bits"] <= 64 and min_bits != 128 else 128)
        assert basis == t.basis
        lo, hi = lohi
        got = [[Fraction(lp.exact._int128(a, b), D) for a, b in zip(rl, rh)] for rl, rh in zip(lo.tolist(), hi.tolist())]
        assert got == t.matrix


def test_bounded_calls_reach_the_one_call_trace_and_entries():
    refs = _mixed_refs()
    (xa, xm), _ = _batches([r[0] for r in refs])
    total = _one_pivot_per_call(xa, xm, refs)
    _check_two_phase_batch(xa, xm, refs, total)


# ---- 3. escalation inside a two-phase batch --------------------------------------------------------------
WIDE_MIXED = [(s, e) for e in (10, 28) for s in range(8)]


def _wide_mixed_refs():
    refs = [_reference("wide_mixed_problem", s, e) for s, e in WIDE_MIXED]
    for (s, e), r in zip(WIDE_MIXED, refs):
        mb = r[4]["max_bits"]
        assert r[1] == "optimal"
        assert mb <= 34 if e == 10 else 61 <= mb <= 88
        assert (mb <= 64) == (e == 10 or s == 5)
    return refs


def test_escalation_inside_a_two_phase_batch():
    refs = _wide_mixed_refs()
    got = lp.solve_problems([r[0] for r in refs], exact=True)
    assert got[0].phase1._matrix.shape == (5, 10) and got[0]._matrix.shape == (5, 8)
    for r, g in zip(refs, got):
        _check_member(r, g)
    assert [g.bits for g in got].count(128) == 7
    # one pivot per call: a restarted member replays both phases and counts no pivot twice
    (xa, xm), tabs = _batches([r[0] for r in refs])
    assert all(t[0].bits == 64 and t[1].bits == 64 for t in tabs[8:9])       # (the start fits 64 bits)
    total = _one_pivot_per_call(xa, xm, refs)
    _check_two_phase_batch(xa, xm, refs, total)


# ---- 4. every outcome in a group --------------------------------------------------------------------------
def test_every_outcome_in_a_group_equals_the_one_by_one_result():
    groups = {}
    for seed in range(200):
        tabs = rr.build_tableau(ec.to_dict(ec.random_problem(lp, seed)))
        if isinstance(tabs, tuple):
            key = tuple((len(t.matrix), len(t.matrix[0])) for t in tabs) + (tabs[1].is_max,)
        else:
            key = ((len(tabs.matrix), len(tabs.matrix[0])), tabs.is_max)
        groups.setdefault(key, []).append(seed)
    groups = {k: v for k, v in groups.items() if len(v) >= 2}
    assert len(groups) == 26 and all(len(k) == 3 for k in groups)              # (all of them two-phase)
    seeds = sorted(s for v in groups.values() for s in v)
    refs = [_reference("random_problem", s) for s in seeds]
    count = {st: sum(r[1] == st for r in refs) for st in ("optimal", "infeasible", "unbounded", "art_stuck")}
    assert len(refs) == 60 and count == {"optimal": 13, "infeasible": 22, "unbounded": 12, "art_stuck": 13}
    assert sum(bool(r[4]["driveouts"]) for r in refs) == 7
    got = lp.solve_problems([r[0] for r in refs], exact=True, errorp=False)
    assert sum(isinstance(g, lp.ExactTableau) and g._batch is not None for g in got) == 13
    for r, g in zip(refs, got):
        _check_member(r, g)
        try:
            one = lp.solve_problem(r[0], exact=True)
        except lp.SolverError as e:
            assert type(g) is type(e) and g.args == e.args
            continue
        assert g.matrix.tolist() == one.matrix.tolist() and g.basis_columns.tolist() == one.basis_columns.tolist()
        assert _trace(g) == _trace(one) and tuple(g.n_pivots) == tuple(one.n_pivots) and g.bits == one.bits


# ---- 5. a cycling member does not hold the others ----------------------------------------------------------
def _bounded_problem(rows, rhs, obj):
    names = ["x1", "x2", "x3", "x4"]
    return lp.Problem(type="max", vars=names, objective_var="z", objective_func=list(zip(names, obj)),
                      constraints=[("<=", list(zip(names, a)), b) for a, b in zip(rows, rhs)])


def _beale_group():
    F = Fraction
    return [ec.beale(lp),
            _bounded_problem([[1, 2, 1, 1], [2, 1, 3, 1], [1, 1, 1, 2]], [10, 12, 9], [3, 2, 4, 1]),
            _bounded_problem([[F(1, 2), 1, 2, 1], [1, F(1, 3), 1, 3], [2, 2, 1, 1]], [7, 8, F(21, 2)], [1, 5, 2, F(3, 2)]),
            _bounded_problem([[3, 1, 1, 2], [1, 4, 1, 1], [1, 1, 5, 1]], [15, 16, 20], [2, 3, 4, 1])]


def _beale_state(k):
    ref = rr.build_tableau(ec.to_dict(ec.beale(lp)))
    for _ in range(k % 6):                                  # the cycle's state after k pivots
        e = rr.price(ref)
        rr.pivot(ref, e, rr.ratio(ref, e))
    return ref


def _member_matrix(xb, q):
    (lo, hi), D, basis, _, _, _ = _download(xb, q)
    return [[Fraction(lp.exact._int128(a, b), D) for a, b in zip(rl, rh)] for rl, rh in zip(lo.tolist(), hi.tolist())], basis


def test_a_cycling_member_does_not_hold_the_others():
    ps = _beale_group()
    others = []
    for p in ps[1:]:
        tabs = rr.build_tableau(ec.to_dict(p))
        st, trace, t = ec.oracle_outcome(tabs)
        assert st == "optimal" and not isinstance(tabs, tuple) and len(trace) >= 1
        others.append((trace, t))
    (xb,), tabs = _batches(ps)
    assert tabs[0]._matrix.shape == (4, 8)
    rc, st, npv = xb.solve(True, 60)
    assert rc == capi.MI_OK and st.tolist() == [capi.MI_MAX_PIVOTS] + [capi.MI_OPTIMAL] * 3
    assert npv[0] == 60 and npv[1:].tolist() == [len(tr) for tr, _ in others]
    assert _download(xb, 0)[4] == PERIOD * 10
    for q, (trace, t) in enumerate(others, 1):
        M, basis = _member_matrix(xb, q)
        assert _download(xb, q)[4] == trace and M == t.matrix and basis == t.basis
    got = lp.solve_problems(ps, exact=True, errorp=False, max_pivots=60)
    assert isinstance(got[0], lp.SolverError) and "cap" in str(got[0])
    for g, (trace, t) in zip(got[1:], others):
        assert _trace(g) == trace and g.matrix.tolist() == t.matrix
    # cancel from another thread during an uncapped call
    out = {}
    th = threading.Thread(target=lambda: out.update(r=xb.solve(True, 0)))
    th.start()
    xb.cancel()
    th.join(timeout=60)
    assert not th.is_alive()
    rc, st, npv = out["r"]
    assert rc == capi.MI_CANCELLED and st.tolist() == [capi.MI_RUNNING] + [capi.MI_OPTIMAL] * 3
    assert npv[0] > 0 and not npv[1:].any()
    k = _download(xb, 0)[5]
    assert k == 60 + npv[0]
    ref = _beale_state(k)
    assert _member_matrix(xb, 0) == (ref.matrix, ref.basis)
    for q, (trace, t) in enumerate(others, 1):
        assert _member_matrix(xb, q) == (t.matrix, t.basis)
    rc, st, npv = xb.solve(True, 7)                          # ... and a further capped call carries on
    assert rc == capi.MI_OK and st[0] == capi.MI_MAX_PIVOTS and npv.tolist() == [7, 0, 0, 0]
    ref = _beale_state(k + 7)
    assert _member_matrix(xb, 0) == (ref.matrix, ref.basis)


# ---- 6. strides and ties inside one workgroup ---------------------------------------------------------------
def _slack_batch(tabs, max_pivots=0, min_bits=0):
    """Integer slack-form starts straight through the C ABI against VecModel with the same cap."""
    L = capi.lib()
    num = np.ascontiguousarray(np.stack([T for T, _ in tabs]))
    den = np.ones_like(num)
    basis = np.ascontiguousarray(np.stack([b for _, b in tabs]))
    n, R, C = num.shape
    h = ctypes.c_void_p()
    assert L.mi355x_xbatch_create(ctypes.byref(h), n, R, C, _ptr(num), _ptr(den), _ptr(basis), 0, min_bits) == capi.MI_OK
    xb = lp.exact.XBatch.__new__(lp.exact.XBatch)
    xb.handle, xb.n_lps, xb.rows, xb.cols = h, n, R, C
    rc, st, npv = xb.solve(True, max_pivots)
    assert rc == capi.MI_OK
    seen = set()
    for q, (T, b) in enumerate(tabs):
        model = ec.VecModel.from_state(T, 1, b, C - 1)
        trace = []
        mst = model.solve(True, trace, max_pivots)
        lohi, D, gb, bits, gtrace, gn = _download(xb, q)
        assert st[q] == CODES[mst], (q, st[q], mst)
        assert gtrace == trace[:capi.XBATCH_TRACE_CAP] and gn == len(trace) == npv[q]
        assert gb == model.basis and D == model.D
        assert _same_entries(lohi, model.T)
        assert not model.stats["inexact"] and model.stats["max_bits"] <= 128
        assert bits == (128 if min_bits == 128 or model.stats["max_bits"] > 64 else 64)
        seen.add(mst)
    xb.close()
    return seen


@pytest.mark.parametrize("m,n,kw,cap,min_bits", [
    (3, 4, {}, 0, 0),
    (20, 3 * WG + 5, {}, 0, 0),
    (2 * WG + 3, 6, {"density": 0.3}, 0, 0),
    (300, 400, {}, 20, 0),
    (300, 400, {}, 20, 128),
])
def test_strides_and_ties_inside_one_workgroup(m, n, kw, cap, min_bits):
    seen = _slack_batch([ec.slack_tableau(m, n, seed, **kw) for seed in range(8)], cap, min_bits)
    assert seen <= {"optimal", "unbounded", "max_pivots"} and (cap == 0 or "max_pivots" in seen)


def test_planted_ties_one_workgroup_size_apart():
    tabs = []
    for seed in range(4):                                   # pricing: two equal best columns, WG apart
        T, b = ec.slack_tableau(20, 3 * WG + 5, seed)
        T[-1, 5] = T[-1, 5 + WG] = -9
        tabs.append((T, b))
    assert ec.VecModel.from_state(tabs[0][0], 1, tabs[0][1], tabs[0][0].shape[1] - 1).price(True) == 5
    _slack_batch(tabs)
    tabs = []
    for seed in range(4):                                   # ratio test: two equal best rows, WG apart
        T, b = ec.slack_tableau(2 * WG + 3, 6, seed, density=0.3)
        T[7, :6] = T[7 + WG, :6] = 3
        T[7, -1] = T[7 + WG, -1] = 1
        T[:7, :6] = 0                                       # (no lower row ties with them)
        tabs.append((T, b))
    model = ec.VecModel.from_state(tabs[0][0], 1, tabs[0][1], tabs[0][0].shape[1] - 1)
    assert model.ratio(model.price(True)) == 7
    _slack_batch(tabs)


# ---- 8. handle cycles -----------------------------------------------------------------------------------------
def test_batch_handle_cycles_do_not_lose_device_memory():
    import torch
    tabs = [lp.build_tableau(_reference("mixed_problem", 6, 3, 2, 1, s)[0], exact=True) for s in range(16)]

    def cycle():
        xa = lp.exact.XBatch([t[0] for t in tabs])
        xm = lp.exact.XBatch([t[1] for t in tabs])
        rc, st, _ = xa.solve_two_phase(xm, True, 0)
        assert rc == capi.MI_OK and not st.any()
        _download(xm, 15)
        xa.close()
        xm.close()
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(100):
        cycle()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20


# ---- 9. the trace buffer ---------------------------------------------------------------------------------------
def test_member_trace_buffer_stops_at_its_capacity_while_the_count_goes_on():
    CAP = capi.XBATCH_TRACE_CAP
    assert CAP >= 1024
    total = CAP + 60
    (xb,), _ = _batches(_beale_group()[:2])
    rc, st, npv = xb.solve(True, total)
    assert rc == capi.MI_OK and st.tolist() == [capi.MI_MAX_PIVOTS, capi.MI_OPTIMAL] and npv[0] == total
    _, _, _, _, trace, n = _download(xb, 0)                  # (_download: nothing is written past the capacity)
    assert n == total and trace == (PERIOD * (CAP // 6 + 1))[:CAP]
    L = capi.lib()
    e, r = np.full(200, -7, dtype=np.int64), np.full(200, -7, dtype=np.int64)
    cnt = ctypes.c_int64(0)
    assert L.mi355x_xbatch_trace(xb.handle, 0, _ptr(e), _ptr(r), 100, ctypes.byref(cnt)) == capi.MI_OK and cnt.value == total
    assert list(zip(e[:100].tolist(), r[:100].tolist())) == trace[:100] and (e[100:] == -7).all() and (r[100:] == -7).all()
    ref = _beale_state(total)
    assert _member_matrix(xb, 0) == (ref.matrix, ref.basis)


# ---- 10. float members ------------------------------------------------------------------------------------------
def test_float_members_take_the_double_path():
    def floaty(p):
        return lp.Problem(type=p.type, vars=list(p.vars), objective_var=p.objective_var,
                          objective_func=[(v, float(c)) for v, c in p.objective_func], constraints=list(p.constraints))
    rat = _beale_group()[1:]
    ps = [rat[0], floaty(rat[0]), rat[1], floaty(rat[2])]
    got = lp.solve_problems(ps, exact=True)
    today = lp.solve_problems(ps)
    for k in (0, 2):
        assert isinstance(got[k], lp.ExactTableau) and got[k]._batch is not None
        assert isinstance(lp.solution_objective_value(got[k]), Fraction)
    for k in (1, 3):
        assert type(got[k]) is type(today[k]) and not isinstance(got[k], lp.ExactTableau)
        names = [ps[k].objective_var] + list(ps[k].vars)
        assert [lp.solution_variable(got[k], v) for v in names] == [lp.solution_variable(today[k], v) for v in names]
        assert got[k].matrix.tolist() == today[k].matrix.tolist()


# ---- handles in the wrong role ----------------------------------------------------------------------------------
def test_mismatched_pairs_are_refused():
    refs = _mixed_refs()[:3]
    (xa, xm), _ = _batches([r[0] for r in refs])
    (ya, ym), _ = _batches([r[0] for r in refs[:2]])
    L = capi.lib()
    st = np.empty(3, dtype=np.int32)
    assert L.mi355x_xbatch_solve_two_phase(xa.handle, ym.handle, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG   # other count
    assert L.mi355x_xbatch_solve_two_phase(xm.handle, xa.handle, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG   # main is wider
    assert L.mi355x_xbatch_solve_two_phase(xa.handle, xm.handle, 1, 0, _ptr(st), None) == capi.MI_OK
    assert L.mi355x_xbatch_solve(xa.handle, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG                    # a job's batch
    assert L.mi355x_xbatch_solve_two_phase(ya.handle, xm.handle, 1, 0, _ptr(st), None) == capi.MI_BAD_ARG
    assert L.mi355x_xbatch_download(xa.handle, 3, None, None, None) == capi.MI_BAD_ARG
    h = ctypes.c_void_p()
    big = np.ones((2, 2, 4000), dtype=np.int64)
    assert L.mi355x_xbatch_create(ctypes.byref(h), 2, 2, 4000, _ptr(big), _ptr(big), _ptr(np.zeros(2, dtype=np.int64)),
                                  0, 0) == capi.MI_UNSUPPORTED and not h.value      # the snapshots do not fit the LDS


# ---- 11. k_xb_between past one trip of its strided loops -------------------------------------------------------
# The drive-out column search, the w / basis copy, the hand-over's column loop (src = nav for the last column)
# and xb_apply on the artificial tableau with more than one workgroup's worth of rows or columns, against the
# Fraction oracle and VecModel (tests/test_exact_host.py pins it to Model and so to the oracle) -- never
# against the one-tableau path.
WIDE_SEEDS = (0, 1, 2)


def _wide_refs():
    """Three members of one shape, artificial tableau 18 x 321 and main tableau 18 x 314: mixed_problem's 300
    variables with fewer rows than the one-tableau test's 40 + 6 + 4, whose full solve outgrows 128 bits
    (134 to 139 bits at seeds 5, 1, 2) -- these end optimal inside 64."""
    refs = [_reference("mixed_problem", 300, 8, 3, 2, s) for s in WIDE_SEEDS]
    for p, st, trace, t, stats, n1 in refs:
        assert st == "optimal" and stats["driveouts"] >= 1 and stats["max_bits"] <= 64 and n1 >= 3
        assert len(trace) > n1                                           # (phase 2 pivots the handed-over tableau)
    return refs


def test_wide_group_through_solve_problems():
    """Wider than one workgroup in both tableaux, through the public route: grouping, the batch pair, the
    read-back -- per member against the Fraction oracle."""
    refs = _wide_refs()
    got = lp.solve_problems([r[0] for r in refs], exact=True)
    assert got[0].phase1._matrix.shape == (18, 321) and got[0]._matrix.shape == (18, 314)
    assert all(g._batch is not None and g._batch[0] is got[0]._batch[0] for g in got)     # one batch, not one by one
    for r, g in zip(refs, got):
        _check_member(r, g)


@pytest.mark.parametrize("min_bits", [0, 128])
def test_wide_group_as_a_batch_pair_in_one_call_and_in_bounded_calls(min_bits):
    refs = _wide_refs()
    (xa, xm), _ = _batches([r[0] for r in refs], min_bits)
    rc, st, npv = xa.solve_two_phase(xm, True, 0)
    assert rc == capi.MI_OK and (st == capi.MI_OPTIMAL).all()
    _check_two_phase_batch(xa, xm, refs, npv, min_bits)
    if min_bits == 0:
        (xa, xm), _ = _batches([r[0] for r in refs])
        total = _one_pivot_per_call(xa, xm, refs)
        _check_two_phase_batch(xa, xm, refs, total)


@functools.lru_cache(maxsize=None)
def _pair_reference(n, m_le, m_ge, m_eq, seed, total):
    """(problem, art tableau, main tableau, art model after the drive-outs, main model, trace, n1, stats,
    status, drive-out pivots) of a mixed_problem under a cap of `total` pivots (0: none)."""
    p = ec.mixed_problem(lp, n, m_le, m_ge, m_eq, seed)
    art_t, main_t = rr.build_tableau(ec.to_dict(p))
    keep = {}
    st, trace, mm, stats = ec.model_solve((art_t, main_t), cls=ec.VecModel, keep=keep, total_pivots=total)
    assert mm is not None and not stats["inexact"] and stats["max_bits"] <= 128
    return p, art_t, main_t, keep["art"], mm, trace, keep["n1"], stats, st, keep.get("driveout_pivots", [])


def _check_pairs_against_models(pair, refs, calls, min_bits=0):
    """The batch pair (art, main) of the members of refs solved in `calls` (their max_pivots: they add up to
    the references' cap, or reach past the end of an uncapped reference): per member the status, both traces,
    both bases, D and every entry of both tableaux."""
    xa, xm = pair
    try:
        total = np.zeros((len(refs), 2), dtype=np.int64)
        for cap in calls:
            rc, st, npv = xa.solve_two_phase(xm, True, cap)
            assert rc == capi.MI_OK
            total += npv
        for q, (_, art_t, main_t, art, mm, trace, n1, stats, mst, _) in enumerate(refs):
            assert st[q] == CODES[mst], (q, st[q], mst)
            assert tuple(total[q]) == (n1 + stats["driveouts"], len(trace) - n1)
            bits = 128 if min_bits == 128 or stats["max_bits"] > 64 else 64
            lohi, D, basis, abits, atrace, an = _download(xa, q)
            assert atrace == trace[:n1] and an == n1 and abits == bits
            assert basis == art.basis and D == art.D and _same_entries(lohi, art.T)
            lohi, D, basis, mbits, mtrace, mn = _download(xm, q)
            assert mtrace == trace[n1:] and mn == len(trace) - n1 and mbits == bits
            assert basis == mm.basis and D == mm.D and _same_entries(lohi, mm.T)
    finally:
        xa.close()
        xm.close()


@pytest.mark.parametrize("total,calls,min_bits", [(32, (32,), 0), (32, (5,) * 6 + (2,), 0), (32, (32,), 128),
                                                  (60, (60,), 0)])
def test_between_phases_of_the_one_tableau_tests_wide_shape(total, calls, min_bits):
    """mixed_problem(300, 40, 6, 4), the shape of the one-tableau hand-over test (55 x 361 and 55 x 349): a full
    solve needs more than 128 bits, so the call is capped.  Every drive-out's column lies past the first trip
    of the search, the hand-over's column loop makes a second trip and its last column comes from the
    artificial tableau's last one.  In one call, in bounded calls, at 128 bits from the start, and (60
    pivots) escalating to 128 bits on the way, which replays the step."""
    refs = [_pair_reference(300, 40, 6, 4, seed, total) for seed in (5, 1, 2)]
    for _, art_t, main_t, _, _, _, n1, stats, st, drive in refs:
        assert len(art_t.matrix[0]) > len(main_t.matrix[0]) > WG and n1 >= 3
        assert st == "max_pivots" and stats["driveouts"] >= 1 and len(drive) == stats["driveouts"]
        assert (stats["max_bits"] > 64) == (total == 60)
        assert all(j >= WG and eligible[0] == j for j, _, eligible in drive)
    _check_pairs_against_models(_batches([r[0] for r in refs], min_bits)[0], refs, calls, min_bits)


def _planted(seed, row3, total=12):
    """A start that is phase-1 optimal at once (no positive entry in the artificial objective row) with two
    artificial variables basic at zero over the planted row row3 and a random one: both are driven out.
    300 structural columns, three slack rows; -> the tuple of _pair_reference with the integer starts
    ((art, basis), (main, basis)) in the problem's place."""
    rng = np.random.default_rng(seed)
    n, ms = 300, 3
    nv = n + ms                                                          # main: nv columns and the right-hand side
    main = np.zeros((ms + 3, nv + 1), dtype=np.int64)
    main[:ms, :n] = rng.integers(1, 4, size=(ms, n))
    main[np.arange(ms), n + np.arange(ms)] = 1
    main[:ms, -1] = rng.integers(5, 40, size=ms)
    main[ms, :n] = row3
    main[ms + 1, :n] = -rng.integers(0, 3, size=n)
    main[-1, :n] = -rng.integers(1, 4, size=n)
    art = np.zeros((ms + 3, nv + 3), dtype=np.int64)
    art[:, :nv] = main[:, :nv]
    art[:, -1] = main[:, -1]
    art[ms, nv + 1], art[ms + 1, nv] = 1, 1                              # dealt in decreasing row order
    art[-1] = 0
    art[-1, :nv] = main[ms, :nv] + main[ms + 1, :nv]
    mbasis = list(range(n, n + ms)) + [nv + 1, nv + 1]
    abasis = list(range(n, n + ms)) + [nv + 1, nv]
    art_t = rr.Tableau(art.tolist(), abasis, nv + 2, ms + 2, {}, False)
    main_t = rr.Tableau(main.tolist(), mbasis, nv, ms + 2, {}, True)
    keep = {}
    st, trace, mm, stats = ec.model_solve((art_t, main_t), cls=ec.VecModel, keep=keep, total_pivots=total)
    assert mm is not None and not stats["inexact"] and stats["max_bits"] <= 64 and keep["n1"] == 0, (st, stats)
    starts = ((art, np.array(abasis, dtype=np.int64)), (main, np.array(mbasis, dtype=np.int64)))
    return starts, art_t, main_t, keep["art"], mm, trace, 0, stats, st, keep["driveout_pivots"]


def _planted_pair(refs, min_bits=0):
    """The planted integer starts as a batch pair; creation must succeed."""
    pair = []
    for w in (0, 1):
        num = np.stack([r[0][w][0] for r in refs])
        pair.append(lp.exact.XBatch.from_states(num, np.ones_like(num), np.stack([r[0][w][1] for r in refs]),
                                                min_bits=min_bits))
    return tuple(pair)


def test_planted_drive_out_columns_beyond_and_across_the_first_trip():
    """Members whose first drive-out row has its first eligible (non-zero, non-basic) column at an index past
    the workgroup size, and members with eligible columns on both sides of it, held by different threads:
    the lowest wins.  Both facts are read from the model's drive-out pivots."""
    refs = []
    for seed in range(3):
        row = np.zeros(300, dtype=np.int64)
        row[WG + 14 + seed:] = -np.random.default_rng(seed).integers(0, 3, size=300 - WG - 14 - seed)
        row[WG + 14 + seed] = -2
        refs.append(_planted(seed, row))
    for seed in range(3, 6):
        row = -np.random.default_rng(seed).integers(1, 4, size=300)
        row[:3 + seed] = 0
        refs.append(_planted(seed, row))
    for r in refs[:3]:
        j, i, eligible = r[9][0]
        assert j >= WG and eligible[0] == j and len(r[9]) == 2
    for r in refs[3:]:
        j, i, eligible = r[9][0]
        assert j < WG and j == min(eligible) and sum(e < WG for e in eligible) > 100
        assert sum(e >= WG for e in eligible) > 40 and len({e % WG for e in eligible}) > 200
    _check_pairs_against_models(_planted_pair(refs), refs, (12,))
    _check_pairs_against_models(_planted_pair(refs, 128), refs, (12,), min_bits=128)


@pytest.mark.parametrize("calls,min_bits", [((0,), 0), ((9,) * 4, 0), ((0,), 128)])
def test_between_phases_of_a_group_taller_than_one_workgroup(calls, min_bits):
    """264 constraint rows, artificial rows on both sides of row 256, drive-outs in rows past it, phase 2
    pivoting the handed-over tableau: the w / basis copy, the snapshots of xb_apply on the artificial tableau
    and the basic-column scan run past one trip, at 64 and at 128 bits."""
    refs = [_pair_reference(10, 250, 6, 4, seed, 0) for seed in (0, 2, 3)]
    for _, art_t, main_t, art, mm, trace, n1, stats, st, drive in refs:
        m = len(art_t.matrix) - 1
        arts = [i for i in range(m) if art_t.basis[i] >= main_t.var_count]
        assert m > WG and min(arts) < WG < max(arts) and (m + 1 + len(art_t.matrix[0])) * 16 <= 48 * 1024
        assert st == "optimal" and stats["driveouts"] >= 1 and all(i > WG for _, i, _ in drive)
        assert len(trace) > n1 and stats["max_bits"] <= 64
        assert any(b < 10 for b in art.basis[WG:])             # a structural column basic in a row past 256
    _check_pairs_against_models(_batches([r[0] for r in refs], min_bits)[0], refs, calls, min_bits)
