"""Exact batches built on the device (mi355x_xbatch_create_lps: k_xb_assemble_lps) against the batches the
host builds from build_tableau(exact=True) (mi355x_xbatch_create) -- start states, widths, statuses, pivot
sequences and final entries, member for member -- and against the Python-int statement of the kernel
(tests/exact_lps_cases.assemble) at the shapes where its loops take more than one trip; then the public
functions on top: mi355x_solve_problems(exact=True, device_build=True) and solve_lps_exact."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_cases as ec
from tests import exact_lps_cases as xc
from tests import pivot_rule_cases as prc
from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi
xl = lp.exact_lps
pytestmark = pytest.mark.gpu
CAP = 4000                                    # every solve carries a finite cap


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _download(xb, q):
    """(T as rows of Python ints, D, basis, bits, trace, trace count) of member q through the C ABI."""
    L = capi.lib()
    R, C = xb.rows, xb.cols
    T = np.empty(R * C * 2, dtype=np.int64)
    D = np.empty(2, dtype=np.int64)
    b = np.empty(R - 1, dtype=np.int64)
    assert L.mi355x_xbatch_download(xb.handle, q, _ptr(T), _ptr(D), _ptr(b)) == capi.MI_OK
    lo, hi = T[0::2].reshape(R, C), T[1::2].reshape(R, C)
    if np.array_equal(hi, lo >> 63):
        rows = lo.tolist()
    else:
        rows = [[lp.exact._int128(a, c) for a, c in zip(rl, rh)] for rl, rh in zip(lo.tolist(), hi.tolist())]
    bits = ctypes.c_int(0)
    assert L.mi355x_xbatch_bits(xb.handle, q, ctypes.byref(bits)) == capi.MI_OK
    n = ctypes.c_int64(0)
    e, r = np.empty(capi.XBATCH_TRACE_CAP, dtype=np.int64), np.empty(capi.XBATCH_TRACE_CAP, dtype=np.int64)
    assert L.mi355x_xbatch_trace(xb.handle, q, _ptr(e), _ptr(r), capi.XBATCH_TRACE_CAP, ctypes.byref(n)) == capi.MI_OK
    k = min(n.value, capi.XBATCH_TRACE_CAP)
    return rows, lp.exact._int128(D[0], D[1]), b.tolist(), bits.value, list(zip(e[:k].tolist(), r[:k].tolist())), n.value


def _host_pair(problems, min_bits=0, pivot_rule="dantzig"):
    """(main XBatch, artificial XBatch or None) of problems of one group, built on the host."""
    tabs = [lp.build_tableau(p, exact=True) for p in problems]
    if isinstance(tabs[0], list):
        return (lp.exact.XBatch([t[1] for t in tabs], min_bits=min_bits, pivot_rule=pivot_rule),
                lp.exact.XBatch([t[0] for t in tabs], min_bits=min_bits, pivot_rule=pivot_rule))
    return lp.exact.XBatch(tabs, min_bits=min_bits, pivot_rule=pivot_rule), None


def _device_pair(problems, min_bits=0, pivot_rule="dantzig"):
    lows = [xl.lower_problem(p) for p in problems]
    return xl.create_lps(np.stack([l.num for l in lows]), np.stack([l.den for l in lows]),
                         np.stack([l.sense for l in lows]), min_bits=min_bits, pivot_rule=pivot_rule)


def _same_members(got, want, n, trace=False):
    """Every member of two batches (None: both) holds the same T, D, basis and width (and trace)."""
    assert (got is None) == (want is None)
    if got is None:
        return
    assert (got.rows, got.cols, got.n_lps) == (want.rows, want.cols, want.n_lps) and got.n_lps == n
    for q in range(n):
        a, b = _download(got, q), _download(want, q)
        assert a[:4] == b[:4], q
        if trace:
            assert a[4:] == b[4:], q


def _close(*batches):
    for b in batches:
        if b is not None:
            b.close()


def _solve(main, art, is_max, cap=CAP):
    if art is None:
        rc, st, npv = main.solve(is_max, cap)
    else:
        rc, st, npv = art.solve_two_phase(main, is_max, cap)
    assert rc == capi.MI_OK
    return st.tolist(), npv.tolist()


@functools.lru_cache(maxsize=None)
def _random_groups():
    """Groups of random_problem members as group_lowered forms them: [(problems, is_max)], a dozen at the most."""
    ps = [ec.random_problem(lp, s) for s in range(160)]
    host, groups = xl.group_lowered(ps)
    assert set(host.values()) == {"alone"}
    out = [([ps[k] for k, _ in members], key[4]) for key, members in groups.items()]
    assert len(out) >= 6 and sum(len(g) for g, _ in out) >= 13 and {key[4] for key in groups} == {True, False}
    return out


def _mixed():
    return [ec.mixed_problem(lp, 6, 3, 2, 1, s) for s in range(8)]


# ---- before any solve ------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_bits", [0, 128])
def test_start_states_equal_the_host_built_batches(min_bits):
    sets = [ps for ps, _ in _random_groups()] + [_mixed(), [xc.dense_slack_problem(lp, 8, s) for s in range(6)]]
    for ps in sets:
        hm, ha = _host_pair(ps, min_bits)
        dm, da = _device_pair(ps, min_bits)
        _same_members(dm, hm, len(ps))
        _same_members(da, ha, len(ps))
        if min_bits == 128:
            assert [_download(dm, q)[3] for q in range(len(ps))] == [128] * len(ps)
        _close(hm, ha, dm, da)


# ---- the smallest shapes at which the kernel's loops take another trip ------------------------------------------
def _tall_pattern(i):
    """300 rows, all three senses, a third of the right-hand sides negative, 273 artificial rows."""
    neg = i % 3 == 0
    if i % 9 == 4:
        return 2, neg
    if i % 10 == 7:
        return (1 if neg else 0), neg                   # not artificial: `>=` flipped, or `<=` as it stands
    return (0 if neg else 1), neg                       # artificial: `<=` flipped, or `>=` as it stands


def _check_against_the_statement(num, den, sense, min_bits=0, bits=64):
    main, art = xl.create_lps(num, den, sense, min_bits=min_bits)
    for q in range(num.shape[0]):
        Dm, M, mb, Da, A, ab = xc.assemble(num[q], den[q], sense[q])
        assert _download(main, q)[:4] == (M, Dm, mb, bits), q
        assert (art is None) == (A is None)
        if art is not None:
            assert _download(art, q)[:4] == (A, Da, ab, bits), q
    shapes = (main.rows, main.cols, art.cols if art else None)
    _close(main, art)
    return shapes


def test_more_rows_than_a_workgroup_has_threads():
    num, den, sense = xc.array_members(3, 300, 3, 11, _tall_pattern, dens=(1, 2, 3), frac_rows=(0, 150, 257, 299, 300))
    n_eq, n_art = xl.row_counts(num, sense)
    assert n_art.tolist() == [273] * 3 and n_eq.tolist() == [33] * 3 and set(sense[0].tolist()) == {0, 1, 2}
    assert 90 <= int((num[0, :300, -1] < 0).sum()) <= 110
    assert _check_against_the_statement(num, den, sense) == (301, 3 + 267 + 1, 3 + 267 + 1 + 273)


def test_more_columns_than_a_workgroup_has_threads():
    pattern = lambda i: ((1, False), (2, True), (0, False))[i]
    num, den, sense = xc.array_members(3, 3, 300, 12, pattern, dens=(1, 2, 3, 4, 6))
    assert _check_against_the_statement(num, den, sense) == (4, 300 + 2 + 1, 300 + 2 + 1 + 2)
    assert _check_against_the_statement(num, den, sense, min_bits=128, bits=128) == (4, 303, 305)


def test_a_member_with_a_single_row():
    for s, neg in ((0, False), (0, True), (1, False), (1, True), (2, False), (2, True)):
        num, den, sense = xc.array_members(2, 1, 2, 13 + s, lambda i: (s, neg), dens=(1, 3, 5))
        art = s == 2 or (s == 1) != neg
        assert _check_against_the_statement(num, den, sense) == (2, 2 + (s != 2) + 1, (2 + (s != 2) + 1 + 1) if art else None)


# ---- plain cases ------------------------------------------------------------------------------------------------
def _problem(cons, obj=(1, 2), kind="max"):
    return lp.Problem(type=kind, vars=["x", "y"], objective_var="w", objective_func=list(zip(["x", "y"], obj)), constraints=cons)


def _plain_groups():
    F = Fraction
    row = lambda op, a, b, rhs: (op, [("x", a), ("y", b)], rhs)
    return {
        "reduction": [xc.reduction_problem(lp), _problem([row(">=", F(1, 2), F(1, 3), 1), row(">=", F(1, 4), F(2, 3), 2)], (-1, -1))],
        "all =": [_problem([row("=", 1, F(1, 2), 3), row("=", F(2, 3), 1, -2)]), _problem([row("=", 2, 1, 4), row("=", 1, F(1, 5), -1)])],
        ">= 0": [_problem([row("<=", 1, 1, 4), row(">=", 1, F(1, 3), 0)]), _problem([row("<=", 2, 1, 5), row(">=", F(1, 2), 1, 0)])],
        "no artificial row": [_problem([row("<=", 1, F(1, 2), 4), row(">=", 1, 3, -1)]), _problem([row("<=", 3, 1, 6), row(">=", -1, 2, F(-1, 2))])],
    }


@pytest.mark.parametrize("name", ["reduction", "all =", ">= 0", "no artificial row"])
def test_plain_cases(name):
    ps = _plain_groups()[name]
    hm, ha = _host_pair(ps)
    dm, da = _device_pair(ps)
    if name == "reduction":
        assert _download(da, 0)[1] == 36 and _download(da, 0)[0][2] == [36, 36, -36, -36, 0, 0, 72]
    if name == "all =":
        assert (dm.cols, da.cols) == (3, 5)                            # no slack column
    if name == ">= 0":
        assert _download(da, 0)[2] == [2, 4] and _download(da, 0)[0][1][3] < 0       # not flipped: slack -D, artificial
    assert (da is None) == (name == "no artificial row")
    _same_members(dm, hm, 2)
    _same_members(da, ha, 2)
    is_max = ps[0].type == "max"
    assert _solve(dm, da, is_max) == _solve(hm, ha, is_max)
    _same_members(dm, hm, 2, trace=True)
    _close(hm, ha, dm, da)


# ---- widths -----------------------------------------------------------------------------------------------------
WIDE_MIXED = [(s, 28) for s in range(8)]                          # tests/test_gpu_exact_batch.py: all but seed 5 leave 64 bits


def test_members_that_overflow_64_bits_are_assembled_again_on_the_device():
    ps = [ec.wide_mixed_problem(lp, s, e) for s, e in WIDE_MIXED]
    hm, ha = _host_pair(ps)
    dm, da = _device_pair(ps)
    _same_members(dm, hm, 8)
    _same_members(da, ha, 8)
    assert [_download(da, q)[3] for q in range(8)] == [64] * 8
    st_d, st_h = _solve(dm, da, True), _solve(hm, ha, True)
    assert st_d == st_h and st_d[0] == [capi.MI_OPTIMAL] * 8
    _same_members(dm, hm, 8, trace=True)
    _same_members(da, ha, 8, trace=True)
    assert [_download(dm, q)[3] for q in range(8)] == [128 if s != 5 else 64 for s, _ in WIDE_MIXED]
    _close(hm, ha, dm, da)
    # in calls of three pivots: the restart replays up to the same cumulative count
    hm, ha = _host_pair(ps)
    dm, da = _device_pair(ps)
    for _ in range(40):
        st_d, st_h = _solve(dm, da, True, 3), _solve(hm, ha, True, 3)
        assert st_d == st_h
        if capi.MI_MAX_PIVOTS not in st_d[0]:
            break
    assert st_d[0] == [capi.MI_OPTIMAL] * 8
    _same_members(dm, hm, 8, trace=True)
    _close(hm, ha, dm, da)


def test_a_member_past_128_bits_leaves_its_neighbours_alone():
    # (wide_problem(seed 2, e = 60) needs 182 bits on the way, tests/test_gpu_exact_batch.py)
    ps = [ec.wide_problem(lp, s, 60) for s in range(6)]
    hm, ha = _host_pair(ps)
    dm, da = _device_pair(ps)
    assert da is None and ha is None
    st_d, st_h = _solve(dm, da, True), _solve(hm, ha, True)
    assert st_d == st_h and st_d[0] == [capi.MI_EXACT_OVERFLOW if s == 2 else capi.MI_OPTIMAL for s in range(6)]
    for q in (0, 1, 3, 4, 5):
        assert _download(dm, q) == _download(hm, q)
    _close(hm, dm)
    # and one whose start state itself needs more than 128 bits: the product of four row LCMs of 41 bits each
    num, den, sense = xc.array_members(3, 4, 2, 21, lambda i: (0, False), lo=0)
    den[1, :4, 0] = [(1 << 40) + 15, (1 << 40) + 37, (1 << 40) + 91, (1 << 40) + 99]
    num[1, :4, 0] = 1
    main, art = xl.create_lps(num, den, sense)
    assert xc.assemble(num[1], den[1], sense[1])[0].bit_length() > 128 and art is None
    others, _ = xl.create_lps(num[[0, 2]], den[[0, 2]], sense[[0, 2]])
    st, npv = _solve(main, None, True)
    st2, npv2 = _solve(others, None, True)
    assert st[1] == capi.MI_EXACT_OVERFLOW and [st[0], st[2]] == st2 and [npv[0], npv[2]] == npv2
    assert capi.MI_EXACT_OVERFLOW not in st2
    assert _download(main, 0) == _download(others, 0) and _download(main, 2) == _download(others, 1)
    _close(main, others)


# ---- solves -----------------------------------------------------------------------------------------------------
def test_one_call_equals_the_host_built_batch():
    for ps, is_max in _random_groups() + [(_mixed(), True)]:
        hm, ha = _host_pair(ps)
        dm, da = _device_pair(ps)
        assert _solve(dm, da, is_max) == _solve(hm, ha, is_max)
        _same_members(dm, hm, len(ps), trace=True)
        _same_members(da, ha, len(ps), trace=True)
        _close(hm, ha, dm, da)


def test_calls_of_five_pivots_equal_the_host_built_batch():
    for ps, is_max in _random_groups()[:6] + [(_mixed(), True)]:
        hm, ha = _host_pair(ps)
        dm, da = _device_pair(ps)
        for _ in range(60):
            st_d, st_h = _solve(dm, da, is_max, 5), _solve(hm, ha, is_max, 5)
            assert st_d == st_h
            if capi.MI_MAX_PIVOTS not in st_d[0]:
                break
        assert capi.MI_MAX_PIVOTS not in st_d[0]
        _same_members(dm, hm, len(ps), trace=True)
        _same_members(da, ha, len(ps), trace=True)
        _close(hm, ha, dm, da)


def test_blands_rule_on_a_degenerate_group():
    ps = prc.beale_variants(lp)                                        # Beale's and Chvatal's LPs cycle under the default rule
    hm, ha = _host_pair(ps, pivot_rule="bland")
    dm, da = _device_pair(ps, pivot_rule="bland")
    st_d, st_h = _solve(dm, da, True, 200), _solve(hm, ha, True, 200)
    assert st_d == st_h and st_d[0] == [capi.MI_OPTIMAL] * 4
    _same_members(dm, hm, 4, trace=True)
    _close(hm, dm)
    dm, da = _device_pair(ps)                                          # (and the default rule does cycle on them)
    assert _solve(dm, da, True, 60)[0][0] == capi.MI_MAX_PIVOTS
    _close(dm)


# ---- the public functions ---------------------------------------------------------------------------------------
def _public_list():
    F = Fraction
    row = lambda op, a, b, rhs: (op, [("x", a), ("y", b)], rhs)
    ps = _mixed()[:4]                                                  # a two-phase group
    ps += [xc.dense_slack_problem(lp, 8, s) for s in range(3)]        # a single-phase group
    ps += [ec.random_problem(lp, s) for s in (3, 7, 11, 13, 17, 19)]  # groups of their own or members alone
    ps.append(_problem([row("<=", 1, 1, 4), row(">=", 1, 1, 1), row("=", 1, -1, F(1, 2))]))          # alone
    ps.append(lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1), ("y", 2)],
                         integer_vars=["x"], constraints=[row("<=", 2, 3, 7), row("<=", 1, 0, F(5, 2))]))
    ps.append(_problem([row("<=", 1.5, 1, 4), row("<=", 1, 1, 3)]))   # a float
    ps += [_problem([row("<=", 1, 1, 4), row(">=", 1, 1, 5)]), _problem([row("<=", 1, 2, 4), row(">=", 1, 2, 6)])]   # infeasible
    ps += [_problem([row("<=", 1, -1, 4), row(">=", 1, 1, 1)]), _problem([row("<=", 1, -2, 4), row(">=", 2, 1, 1)])]   # unbounded
    return ps


def _reduced_cost(sol, v):
    try:
        return lp.solution_reduced_cost(sol, v)
    except ValueError as e:                                            # (a variable without a lower bound)
        return str(e)


def _same_solution(a, b, p):
    if isinstance(b, Exception):
        assert type(a) is type(b), (a, b)
        return
    assert not isinstance(a, Exception), a
    assert lp.solution_objective_value(a) == lp.solution_objective_value(b)
    for v in p.vars:
        assert lp.solution_variable(a, v) == lp.solution_variable(b, v)
        assert _reduced_cost(a, v) == _reduced_cost(b, v)
    assert type(a) is type(b)
    if isinstance(a, lp.ExactTableau):
        assert a.var_mapping == b.var_mapping
        assert a.n_pivots == b.n_pivots and (a.phase1 is None) == (b.phase1 is None)
        assert a.matrix.tolist() == b.matrix.tolist() and a.basis_columns.tolist() == b.basis_columns.tolist()


def test_solve_problems_device_build_equals_the_default_route():
    ps = _public_list()
    host, groups = xl.group_lowered(ps)
    assert "integer variables" in host.values() and "float" in host.values() and "alone" in host.values()
    assert sum(key[3] > 0 for key in groups) >= 2 and sum(key[3] == 0 for key in groups) >= 1
    want = lp.solve_problems(ps, exact=True, errorp=False, max_pivots=CAP)
    got = lp.solve_problems(ps, exact=True, device_build=True, errorp=False, max_pivots=CAP)
    for p, a, b in zip(ps, got, want):
        _same_solution(a, b, p)
    kinds = {type(b) for b in want if isinstance(b, Exception)}
    assert lp.InfeasibleProblemError in kinds and lp.UnboundedProblemError in kinds
    built = [a for k, a in enumerate(got) if k not in host and isinstance(a, lp.ExactTableau)]
    assert len(built) >= 7 and all(a._batch is not None and a._handle is None for a in built)
    first = next(k for k, b in enumerate(want) if isinstance(b, Exception))
    for kw in ({}, {"device_build": True}):
        with pytest.raises(type(want[first])):
            lp.solve_problems(ps, exact=True, max_pivots=CAP, **kw)
    with pytest.raises(ValueError):
        lp.solve_problems(ps, device_build=True)
    got = lp.solve_problems(ps[:7], exact=True, device_build=True, pivot_rule="bland", max_pivots=CAP)
    want = lp.solve_problems(ps[:7], exact=True, pivot_rule="bland", max_pivots=CAP)
    for p, a, b in zip(ps, got, want):
        _same_solution(a, b, p)


def test_solve_lps_exact_on_the_same_data_as_arrays():
    pattern = lambda i: ((0, False), (1, False), (2, False), (0, True), (1, True))[i]
    num, den, sense = xc.feasible_members(3, 4, 31, pattern)
    other = lambda i: ((0, False), (0, False), (2, False), (0, True), (1, True))[i]      # one artificial row fewer
    num, den, sense = (np.concatenate(pair) for pair in zip((num, den, sense), xc.feasible_members(3, 4, 32, other)))
    assert xl.row_counts(num, sense)[1].tolist() == [3, 3, 3, 2, 2, 2]
    ps = [xc.problem_of_arrays(lp, num[q], den[q], sense[q], is_max=False) for q in range(6)]
    want = lp.solve_problems(ps, exact=True, errorp=False, max_pivots=CAP)
    a, b = (num[:, :5, :4], den[:, :5, :4]), (num[:, :5, 4], den[:, :5, 4])
    c = (-num[:, 5, :4], den[:, 5, :4])
    got = xl.solve_lps_exact(a, b, c, sense, is_max=False, max_pivots=CAP)
    unreduced = xl.solve_lps_exact((a[0] * 2, a[1] * 2), (b[0] * -3, b[1] * -3), c, sense, c0=np.arange(6), is_max=False,
                                   max_pivots=CAP)
    assert not any(isinstance(w, Exception) for w in want)             # (x = 1 is feasible and c >= 0 bounds the minimum)
    for q, (p, g, u, w) in enumerate(zip(ps, got, unreduced, want)):
        assert g.status == capi.MI_OPTIMAL and g.objective == lp.solution_objective_value(w) == u.objective - q
        assert g.x == [lp.solution_variable(w, v) for v in p.vars] == u.x
        assert g.reduced_costs == [lp.solution_reduced_cost(w, v) for v in p.vars] == u.reduced_costs
        assert g.pivots == (w.n_pivots if isinstance(w.n_pivots, int) else tuple(w.n_pivots)) == u.pivots


# ---- handle cycles ----------------------------------------------------------------------------------------------
def test_handle_cycles_do_not_lose_device_memory():
    import torch
    lows = [xl.lower_problem(p) for p in _mixed()]
    num, den, sense = (np.stack([getattr(l, f) for l in lows]) for f in ("num", "den", "sense"))

    def cycle():
        main, art = xl.create_lps(num, den, sense)
        st, _ = _solve(main, art, True)
        assert not any(st)
        _download(main, 7)
        _close(art, main)
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(50):
        cycle()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20
