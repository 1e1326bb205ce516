"""The 256-bit width of the exact solves (opt-in: exact_max_bits=256 / mi355x_xtab_create_wide): the device's
wide arithmetic primitive by primitive against Python ints (mi355x_test_xarith opcodes 16 and 17,
mi355x_test_xarith8), solves that need more than 128 bits against the fraction-free model and the Fraction
oracle (tests/exact_cases.py, oracle/rational_ref.py), the decline past 256 bits, bounded calls across the
two restarts, 256 bits from the start, tableaux of many workgroups forced to 256 bits, the two download
forms and the fallback of solve_problems from a batch.  Every expected value comes from the model or from
Python ints; every overflow here is an ordinary status code."""
import ctypes
import random

import numpy as np
import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests.helpers import lp_amd
from tests.test_gpu_exact_arith import M64, X_INEXACT, X_OVERFLOW, _signed, edges, rand_signed

lp = lp_amd()
pytestmark = pytest.mark.gpu
OP4 = {"inv256": 16, "ctz256": 17}
OP8 = {"mul256": 0, "add512": 1, "sub512": 2, "neg512": 3, "lt512": 4, "eq512": 5, "subovf256": 6, "fit256": 7,
       "div256": 8, "rem256": 9}
TOP = (1 << 255) - 1
_ERRORS = {"unbounded": lp.UnboundedProblemError, "infeasible": lp.InfeasibleProblemError,
           "art_nonzero": lp.SolverError, "art_stuck": lp.SolverError}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------- 1. the arithmetic
def _limbs(values, n):
    raw = b"".join((int(v) & ((1 << 64 * n) - 1)).to_bytes(8 * n, "little") for v in values)
    return np.frombuffer(raw, dtype="<i8").reshape(len(values), n).copy()


def _ints(limbs, bits):
    out = []
    for row in limbs.tolist():
        out.append(_signed(sum((x & M64) << (64 * k) for k, x in enumerate(row)), bits))
    return out


def probe(L, op, a, b=None):
    """(out limbs, rc) of one launch of a primitive over the operand lists: four limbs per element for the
    opcodes of OP4, eight for those of OP8."""
    n, nl = len(a), 4 if op in OP4 else 8
    A, B = _limbs(a, nl), _limbs(b if b is not None else [0] * n, nl)
    out = np.full((n, nl), -0x5A5A5A5A, dtype=np.int64)
    rc = np.full(n, -77, dtype=np.int32)
    f, code = (L.mi355x_test_xarith, OP4[op]) if op in OP4 else (L.mi355x_test_xarith8, OP8[op])
    assert f(code, n, _p(A), _p(B), _p(out), _p(rc), 0) == 0, L.mi355x_last_error()
    return out, rc


def wide_edges(W):
    """edges(W) of the 64 / 128-bit tests, and around every limb boundary of W bits: +-(2^k - 1), +-2^k,
    +-(2^k + 1), every limb alone all ones or all zeros."""
    lo, hi = -(1 << (W - 1)), (1 << (W - 1)) - 1
    vals = set(edges(256)) if W >= 256 else set(edges(W))
    for k in list(range(63, W, 64)) + list(range(64, W, 64)) + [W - 2, W - 1]:
        for m in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            vals.update((m, -m))
    for i in range(W // 64):
        vals.add(_signed(M64 << (64 * i), W))
        vals.add(_signed(~(M64 << (64 * i)), W))
    vals.update((lo, hi, -hi))
    return sorted(v for v in vals if lo <= v <= hi)


def pairs(W, seed, n_random=1500, step=2):
    e = wide_edges(W)[::step]
    rng = random.Random(seed)
    return ([x for x in e for _ in e] + rand_signed(rng, W, n_random),
            [y for _ in e for y in e] + rand_signed(rng, W, n_random))


def test_xmul_256_equals_python(hooks_lib):
    a, b = pairs(256, 1)
    prod = [x * y for x, y in zip(a, b)]
    assert len(a) >= 1000
    assert sum(p < 0 and p % (1 << 128) == 0 for p in prod) >= 10 and sum(p < 0 and p % (1 << 256) == 0 for p in prod) >= 10
    assert sum(x < 0 and y < 0 for x, y in zip(a, b)) >= 100 and sum((x < 0) != (y < 0) for x, y in zip(a, b)) >= 100
    out, rc = probe(hooks_lib, "mul256", a, b)
    assert not rc.any()
    assert _ints(out, 512) == prod


@pytest.mark.parametrize("op", ["add512", "sub512", "neg512", "lt512", "eq512"])
def test_512_bit_operations_equal_python(hooks_lib, op):
    a, b = pairs(512, 2, step=3)
    b[-200:] = a[-200:]                                       # equal random operands for eq / lt
    assert len(a) >= 1000
    for k in (64, 128, 192, 256, 320, 384, 448):              # a carry and a borrow across every limb boundary
        assert sum((x % (1 << k)) + (y % (1 << k)) >= 1 << k for x, y in zip(a, b)) >= 20
        assert sum((x % (1 << k)) < (y % (1 << k)) for x, y in zip(a, b)) >= 20
    out, rc = probe(hooks_lib, op, a, b)
    assert not rc.any()
    if op == "neg512":
        assert _ints(out, 512) == [_signed(-x, 512) for x in a]
    elif op in ("lt512", "eq512"):
        f = (lambda x, y: x < y) if op == "lt512" else (lambda x, y: x == y)
        assert out[:, 0].tolist() == [int(f(x, y)) for x, y in zip(a, b)] and not out[:, 1:].any()
        assert sum(x == y for x, y in zip(a, b)) >= 200
    else:
        f = (lambda x, y: x + y) if op == "add512" else (lambda x, y: x - y)
        assert _ints(out, 512) == [_signed(f(x, y), 512) for x, y in zip(a, b)]


def test_xsub_ovf_256_flags_exactly_the_differences_that_leave_512_bits(hooks_lib):
    a, b = pairs(512, 3, step=3)
    out, rc = probe(hooks_lib, "subovf256", a, b)
    lo, hi = -(1 << 511), (1 << 511) - 1
    want = [int(not lo <= x - y <= hi) for x, y in zip(a, b)]
    assert sum(w and x >= 0 for w, x in zip(want, a)) >= 50 and sum(w and x < 0 for w, x in zip(want, a)) >= 50
    assert rc.tolist() == want
    got = _ints(out, 512)
    assert [g for g, w in zip(got, want) if not w] == [x - y for x, y, w in zip(a, b, want) if not w]


def test_xfit_256_accepts_exactly_the_symmetric_range(hooks_lib):
    named = [TOP, -TOP, -(TOP + 1), TOP + 1, -(TOP + 2), TOP + 2, 0, 1, -1, 1 << 256, -(1 << 256), (1 << 256) - 1,
             -((1 << 256) - 1), (1 << 256) + TOP, -(1 << 256) - TOP - 1, (1 << 511) - 1, -(1 << 511)]
    a = named + wide_edges(512) + rand_signed(random.Random(4), 512, 1500) + rand_signed(random.Random(5), 257, 1500)
    out, rc = probe(hooks_lib, "fit256", a)
    want = [int(abs(x) > TOP) for x in a]
    assert want[:4] == [0, 0, 1, 1] and 500 <= sum(want) <= len(want) - 500
    assert rc.tolist() == want
    got = _ints(out[:, :4], 256)
    assert [g for g, w in zip(got, want) if not w] == [x for x, w in zip(a, want) if not w]
    assert not out[:, 4:].any()


def test_xctz_256_counts_across_every_limb(hooks_lib):
    rng = random.Random(6)
    a = [1 << k for k in range(256)]
    a += [(rng.getrandbits(255 - k) | 1) << k for k in range(255) for _ in range(4)]
    a += [v for v in wide_edges(256) if v]
    want = [((v & -v).bit_length() - 1) for v in a]
    assert {0, 63, 64, 127, 128, 191, 192, 255} <= set(want) and len(a) >= 1000
    out, rc = probe(hooks_lib, "ctz256", a)
    assert not rc.any()
    assert out[:, 0].tolist() == want and not out[:, 1:].any()
    _, rc = probe(hooks_lib, "ctz256", [0, 1])
    assert rc.tolist() == [-1, 0]


def test_xinv_odd_256_is_the_inverse_modulo_2_to_the_256(hooks_lib):
    rng = random.Random(7)
    a = [v for v in wide_edges(256) if v & 1] + [v | 1 for v in rand_signed(rng, 256, 1500)]
    assert len(a) >= 1000 and -1 in a and TOP in a
    out, rc = probe(hooks_lib, "inv256", a)
    assert not rc.any()
    got = _ints(out, 256)
    assert all((g * d) % (1 << 256) == 1 for g, d in zip(got, a))


def _divisors(rng):
    """Positive D below 2^255: odd, 2^k, odd * 2^k with k across each limb boundary."""
    W = 256
    odd = [v for v in wide_edges(W) if v > 0 and v & 1][::3] + [v | 1 for v in rand_signed(rng, W, 30) if v > 0]
    D = list(odd) + [1 << k for k in range(0, W - 1, 3)] + [1 << k for k in (63, 64, 65, 127, 128, 129, 191, 192, 193, 254)]
    for k in (1, 7, 62, 63, 64, 65, 100, 126, 127, 128, 129, 160, 190, 191, 192, 193, 230, 250, 253):
        for o in (3, 5, 0xFFFFFFFF, (1 << 61) - 1, (1 << 63) + 1, (1 << 127) - 1, rng.getrandbits(W) | 1):
            if (o << k) <= TOP:
                D.append(o << k)
        D.append((rng.getrandbits(W - 1 - k) | 1) << k)
    assert all(0 < d <= TOP for d in D)
    return sorted(set(D))


def test_xdiv_256_quotients_overflow_and_remainders(hooks_lib):
    rng = random.Random(8)
    W = 256
    D = _divisors(rng)
    tz = lambda d: (d & -d).bit_length() - 1
    assert sum(d & 1 for d in D) >= 20 and sum(d & (d - 1) == 0 for d in D) >= 60
    assert sum(d & (d - 1) != 0 and not d & 1 for d in D) >= 60
    for lo_, hi_ in ((1, 63), (64, 127), (128, 191), (192, 254)):
        assert sum(lo_ <= tz(d) <= hi_ and d & (d - 1) != 0 for d in D) >= 5
    qs_fit = [0, 1, -1, 2, -2, TOP, -TOP, TOP - 1, -(TOP - 1)] + wide_edges(W)[1:-1][::16]
    N, dd, want_rc, want_q = [], [], [], []

    def case(n, d, rc, q=0):
        assert abs(n) < 1 << (2 * W - 1) and (rc == 0) == (n % d == 0 and abs(n // d) <= TOP)
        assert (rc == X_INEXACT) == (n % d != 0)
        N.append(n); dd.append(d); want_rc.append(rc); want_q.append(q)
    for d in D:
        for q in qs_fit + rand_signed(rng, W, 4):
            case(q * d, d, 0, q)
        room = 2 * W - 2 - d.bit_length()
        for q in (TOP + 1, -(TOP + 1), TOP + 2, -(TOP + 2), 1 << W, -(1 << W), (1 << W) + 1):
            if abs(q).bit_length() <= room:
                case(q * d, d, X_OVERFLOW)
        if room > W:
            case(-(rng.getrandbits(room) | (1 << (room - 1))) * d, d, X_OVERFLOW)
        if d > 1:
            k, rs = tz(d), []
            rs.append(rng.randrange(1, d) | (0 if d & 1 else 1))
            if d >> k > 1:
                rs += [(rng.randrange(1, d >> k)) << k, 1 << k, d - (1 << k)]
            for r in rs:
                for q in (0, 1, rng.getrandbits(W - 2), TOP, TOP + 1):
                    if abs(q).bit_length() <= room:
                        case(q * d + r, d, X_INEXACT)
                        case(-(q * d + r), d, X_INEXACT)
    n_even_r = sum(rc == X_INEXACT and (n % d) % (d & -d) == 0 for n, d, rc in zip(N, dd, want_rc))
    assert n_even_r >= 100 and want_rc.count(X_OVERFLOW) >= 100 and want_rc.count(0) >= 1000
    out, rc = probe(hooks_lib, "div256", N, dd)
    bad = [(hex(n), hex(d), w, int(g)) for n, d, w, g in zip(N, dd, want_rc, rc.tolist()) if w != g]
    assert not bad, bad[:5]
    got = _ints(out[:, :4], W)
    bad = [(hex(n), hex(d), q, g) for n, d, w, q, g in zip(N, dd, want_rc, want_q, got) if w == 0 and q != g]
    assert not bad, bad[:5]
    _, rc = probe(hooks_lib, "div256", [5, 5], [0, -3])
    assert rc.tolist() == [-1, -1]


def test_xrem_256_equals_python(hooks_lib):
    rng = random.Random(9)
    Ns = [v for v in wide_edges(512) if abs(v) < 1 << 511][::4]
    ds = [v for v in wide_edges(256) if 0 < v < 1 << 255][::6]
    a = [n for n in Ns for _ in ds] + rand_signed(rng, 512, 1000)
    b = [d for _ in Ns for d in ds] + [abs(v) for v in rand_signed(rng, 256, 1000)]
    assert max(abs(n).bit_length() for n in a) == 511 and max(d.bit_length() for d in b) == 255 and len(a) >= 1000
    out, rc = probe(hooks_lib, "rem256", a, b)
    assert not rc.any()
    assert _ints(out[:, :4], 256) == [abs(n) % d for n, d in zip(a, b)]


# ---------------------------------------------------------------- the solves
def _trace(sol):
    tr = [] if sol.phase1 is None else [tuple(x) for x in sol.phase1.pivot_trace().tolist()]
    return tr + [tuple(x) for x in sol.pivot_trace().tolist()]


def _model(p):
    tabs = rr.build_tableau(ec.to_dict(p))
    mst, mtrace, _, stats = ec.model_solve(tabs)
    return tabs, mst, mtrace, stats


def _check_wide(p, **kw):
    """p needs more than 128 and at most 256 bits (the model says): solved with exact_max_bits=256 it gives the
    oracle's status, trace, basis and entries, at 256 bits."""
    tabs, mst, mtrace, stats = _model(p)
    assert 128 < stats["max_bits"] <= 256 and stats["inexact"] == 0
    st, trace, t = ec.oracle_outcome(tabs)
    assert (st, trace) == (mst, mtrace)
    if st != "optimal":
        with pytest.raises(_ERRORS[st]):
            lp.solve_problem(p, exact=True, exact_max_bits=256, **kw)
        return stats, None
    sol = lp.solve_problem(p, exact=True, exact_max_bits=256, **kw)
    assert sol.bits == 256 and (sol.phase1 is None or sol.phase1.bits == 256)
    assert _trace(sol) == trace
    assert sol.basis_columns.tolist() == t.basis
    assert sol.matrix.tolist() == t.matrix
    return stats, sol


def test_single_phase_solve_at_256_bits():
    p = ec.wide_problem(lp, 2, 60)
    stats, sol = _check_wide(p)
    assert stats["max_bits"] == 182 and sol.n_pivots == 2
    with pytest.raises(lp.UnsupportedConstraintError) as e:                  # without the option: declined, as before
        lp.solve_problem(p, exact=True)
    assert e.value.constraint == ("exact", "overflow", "128 bits")


def test_single_phase_solve_in_bounded_calls_counts_no_pivot_twice():
    p = ec.wide_problem(lp, 2, 60)
    whole = lp.solve_problem(p, exact=True, exact_max_bits=256)
    stats, sol = _check_wide(p, chunk=1)
    assert sol.n_pivots == stats["pivots"] == len(_trace(sol)) == 2
    assert sol.matrix.tolist() == whole.matrix.tolist() and _trace(sol) == _trace(whole)


def wide_problem_8(seed=71, e=60):
    """The 8 x 8 member of exact_cases.wide_problem's family."""
    rng = random.Random(seed)
    names = ["x%d" % i for i in range(8)]
    cons = [("<=", [(v, rng.randint(1 << e, 1 << (e + 1))) for v in names], rng.randint(1 << e, 1 << (e + 1)))
            for _ in range(8)]
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, rng.randint(1, 1 << e)) for v in names], constraints=cons)


def test_a_problem_past_256_bits_is_declined_with_the_256_bit_condition():
    p = wide_problem_8()
    _, mst, mtrace, stats = _model(p)
    assert stats["max_bits"] > 256 and (mst, stats["max_bits"], len(mtrace)) == ("optimal", 362, 5)
    with pytest.raises(lp.UnsupportedConstraintError) as e:
        lp.solve_problem(p, exact=True, exact_max_bits=256)
    assert e.value.constraint == ("exact", "overflow", "256 bits")
    # at the C level: MI_EXACT_OVERFLOW, the message names the width, and the handle stays dead
    t = lp.build_tableau(p, p, exact=True, max_bits=256)
    L, n = lp.capi.lib(), ctypes.c_int64(0)
    for _ in range(2):
        assert L.mi355x_xtab_solve(t._h, 1, 0, ctypes.byref(n)) == lp.capi.MI_EXACT_OVERFLOW
        assert b"256 bits" in L.mi355x_last_error()
    T = np.zeros(9 * 17 * 4, dtype=np.int64)
    assert L.mi355x_xtab_download_limbs(t._h, 4, _p(T), None, None) == lp.capi.MI_EXACT_OVERFLOW


def gen_problem(seed, copy_eq_row=False):
    """The issue's generator of two-phase problems with 40-bit coefficients.  copy_eq_row: its first `=` row
    once more at the end, as a `>=` row (an exact copy leaves a zero row, which ends art_stuck without a
    drive-out; this one leaves an artificial variable basic at zero over a row that is not zero)."""
    rng = random.Random(seed)
    names = ["x0", "x1", "x2", "x3"]
    cons = []
    for _ in range(4):
        op = rng.choice(["<=", ">=", "="])
        cons.append((op, [(v, rng.randint(-(1 << 40), 1 << 41)) for v in names], rng.randint(0, 1 << 41)))
    typ = rng.choice(["max", "min"])
    obj = [(v, rng.randint(1, 1 << 40)) for v in names]
    if copy_eq_row:
        row = [c for c in cons if c[0] == "="][0]
        cons.append((">=", row[1], row[2]))
    return lp.Problem(type=typ, vars=names, objective_var="w", objective_func=obj, constraints=cons)


@pytest.mark.parametrize("seed,status,bits", [(40, "infeasible", 193), (500, "unbounded", 187), (680, "art_stuck", 171)])
def test_two_phase_outcomes_without_a_solution_at_256_bits(seed, status, bits):
    p = ec.random_problem(lp, seed)
    tabs, mst, _, stats = _model(p)
    assert isinstance(tabs, tuple) and (mst, stats["max_bits"]) == (status, bits)
    _check_wide(p)


@pytest.mark.parametrize("seed", [0, 5, 14, 16, 20])
def test_two_phase_optimal_at_256_bits(seed):
    p = gen_problem(seed)
    tabs, mst, _, stats = _model(p)
    assert isinstance(tabs, tuple) and mst == "optimal" and 162 <= stats["max_bits"] <= 205
    stats, sol = _check_wide(p)
    assert sum(sol.n_pivots) == stats["pivots"]


@pytest.mark.parametrize("seed", [0, 5])
def test_two_phase_drive_out_on_a_negative_element_at_256_bits(seed):
    p = gen_problem(seed, copy_eq_row=True)
    _, mst, mtrace, stats = _model(p)
    assert mst == "optimal" and stats["driveouts"] >= 1 and stats["negative_pivots"] >= 1
    stats, sol = _check_wide(p)
    assert sum(sol.n_pivots) == len(mtrace) + stats["driveouts"]


def test_two_phase_in_bounded_calls_restarts_both_phases_together():
    p = gen_problem(0)
    stats, sol = _check_wide(p, chunk=1)
    assert sum(sol.n_pivots) == stats["pivots"] == len(_trace(sol))
    assert sol.n_pivots[0] == len(sol.phase1.pivot_trace())


def test_two_phase_handles_must_allow_the_same_width():
    p = gen_problem(0)
    art, main = lp.build_tableau(p, p, exact=True, max_bits=256)
    main2 = lp.build_tableau(p, p, exact=True)[1]
    npv = (ctypes.c_int64 * 2)()
    L = lp.capi.lib()
    assert L.mi355x_xtab_solve_two_phase(art._h, main2._h, int(main.is_max), 0, npv) == lp.capi.MI_BAD_ARG
    assert b"max_bits" in L.mi355x_last_error()


def test_width_256_from_the_start_gives_the_same_trace_and_values():
    done = 0
    for seed in range(200):                                    # (the seed list of tests/test_gpu_exact.py)
        p = ec.random_problem(lp, seed)
        if _model(p)[3]["max_bits"] > 64:
            continue
        try:
            a = lp.solve_problem(p, exact=True)
        except lp.SolverError:
            continue
        b = lp.solve_problem(p, exact=True, exact_bits=256, exact_max_bits=256)
        assert a.bits == 64 and b.bits == 256 and (b.phase1 is None or b.phase1.bits == 256)
        assert _trace(a) == _trace(b)
        assert a.matrix.tolist() == b.matrix.tolist() and a.basis_columns.tolist() == b.basis_columns.tolist()
        done += 1
        if done == 10:
            break
    assert done == 10


# ---------------------------------------------------------------- 7. shapes of many workgroups, forced to 256 bits
class XTabW:
    """An exact device tableau from an integer matrix through mi355x_xtab_create_wide."""

    def __init__(self, T, basis, min_bits=256, max_bits=256):
        T = np.ascontiguousarray(T, dtype=np.int64)
        basis = np.ascontiguousarray(basis, dtype=np.int64)
        self.shape, self.h = T.shape, ctypes.c_void_p()
        rc = lp.capi.lib().mi355x_xtab_create_wide(ctypes.byref(self.h), T.shape[0], T.shape[1], _p(T),
                                                   _p(np.ones_like(T)), _p(basis), 0, min_bits, max_bits)
        assert rc == lp.capi.MI_OK, lp.capi.lib().mi355x_last_error()

    def solve(self, is_max, max_pivots=0):
        n = ctypes.c_int64(-1)
        rc = lp.capi.lib().mi355x_xtab_solve(self.h, int(is_max), max_pivots, ctypes.byref(n))
        return rc, n.value

    def limbs(self, n=4):
        """(T as an (R * C, n) limb array, D's limbs, basis, the call's status)."""
        R, C = self.shape
        raw = np.full((R * C, n), 0x77, dtype=np.int64)
        D = np.full(n, 0x77, dtype=np.int64)
        b = np.full(R - 1, -7, dtype=np.int64)
        rc = lp.capi.lib().mi355x_xtab_download_limbs(self.h, n, _p(raw), _p(D), _p(b))
        return raw, D, b, rc

    def trace(self, cap=1 << 12):
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


def _forced_256(T, basis, pivots, is_max=True):
    """`pivots` pivots of the model (in int64 numpy throughout) and of the device at 256 bits: trace, basis,
    D and every entry, limb for limb."""
    nv = T.shape[1] - 1
    model = ec.VecModel.from_state(T, 1, basis, nv)
    trace = []
    assert model.solve(is_max, trace, pivots) == "max_pivots" and len(trace) == pivots
    assert model.T.dtype == np.int64 and model.stats["inexact"] == 0
    x = XTabW(T, basis)
    try:
        assert x.solve(is_max, pivots) == (lp.capi.MI_MAX_PIVOTS, pivots), lp.capi.lib().mi355x_last_error()
        assert x.bits == 256 and x.trace() == trace
        raw, D, b, rc = x.limbs()
        assert rc == lp.capi.MI_OK and b.tolist() == model.basis
        assert D.tolist() == [model.D, 0, 0, 0]
        assert np.array_equal(raw[:, 0].reshape(T.shape), model.T)
        assert (raw[:, 1:] == (raw[:, :1] >> 63)).all()                       # sign extension, every entry
    finally:
        x.close()
    return model, trace


def test_forced_256_two_column_blocks_with_a_ragged_tail():
    T, basis = ec.slack_tableau(20, 279, 3)
    assert T.shape == (21, 300)
    _forced_256(T, basis, 6)


def test_forced_256_update_grid_stride_in_x():
    T, basis = ec.slack_tableau(6, 20000, 2, entries=(1, 3))
    assert T.shape[1] > 16384
    model, trace = _forced_256(T, basis, 4)
    assert (model.T[:, 64 * 256:] != T[:, 64 * 256:]).any()                   # the second x-stride's columns change


def test_forced_256_update_grid_stride_in_y():
    m, n = 4100, 3
    T, basis = ec.slack_tableau(m, n, 1, rhs=(2, 9), density=0.5)
    assert T.shape[0] > 4096
    model, trace = _forced_256(T, basis, 3)
    assert (model.T[4096:m, :n] != T[4096:m, :n]).any()                        # the y-stride's rows change


def test_forced_256_multi_trip_scans_and_reduction_trees():
    T, basis = ec.slack_tableau(300, 400, 1)
    assert T.shape == (301, 701)                                               # m = 300 and nv = 700: neither a power of two
    model, trace = _forced_256(T, basis, 8)
    assert max(e for e, _ in trace) >= 256 and max(r for _, r in trace) >= 128   # a second trip of the pricing scan


# ---------------------------------------------------------------- 8. downloads
def test_downloads_on_narrow_and_wide_handles():
    T, basis = ec.slack_tableau(5, 6, 4)
    T[-1, :6] = [-3, 2, -1, -2, 1, -2]                                        # (negative entries stay after the pivots)
    model = ec.VecModel.from_state(T, 1, basis, T.shape[1] - 1)
    trace = []
    model.solve(True, trace, 2)
    L = lp.capi.lib()
    x = XTabW(T, basis, min_bits=0, max_bits=256)                             # stays at 64 bits
    try:
        assert x.solve(True, 2)[1] == 2 and x.bits == 64
        assert (model.T < 0).any()
        for n in (2, 4):
            raw, D, b, rc = x.limbs(n)
            assert rc == lp.capi.MI_OK and D.tolist() == [model.D] + [0] * (n - 1)
            assert np.array_equal(raw[:, 0].reshape(T.shape), model.T) and (raw[:, 1:] == (raw[:, :1] >> 63)).all()
        assert x.limbs(3)[3] == lp.capi.MI_BAD_ARG
    finally:
        x.close()
    x = XTabW(T, basis)                                                       # at 256 bits from the start
    try:
        assert x.solve(True, 2)[1] == 2 and x.bits == 256
        lo_hi = np.full((T.size, 2), 0x55, dtype=np.int64)
        D = np.full(2, 0x55, dtype=np.int64)
        b = np.full(T.shape[0] - 1, 0x55, dtype=np.int64)
        assert L.mi355x_xtab_download(x.h, _p(lo_hi), _p(D), _p(b)) == lp.capi.MI_BAD_ARG
        assert b"mi355x_xtab_download_limbs" in L.mi355x_last_error()
        assert (lo_hi == 0x55).all() and (D == 0x55).all() and (b == 0x55).all()        # nothing written
        raw, D4, _, rc = x.limbs(2)
        assert rc == lp.capi.MI_BAD_ARG and (raw == 0x77).all() and (D4 == 0x77).all()
        assert x.limbs(4)[3] == lp.capi.MI_OK
    finally:
        x.close()


# ---------------------------------------------------------------- 9. solve_problems falls back from a batch
def test_solve_problems_solves_the_member_a_batch_declines_at_256_bits():
    seeds = [1, 2, 3, 4]
    problems = [ec.wide_problem(lp, s, 60) for s in seeds]
    bits = [_model(p)[3]["max_bits"] for p in problems]
    assert bits[1] == 182 and all(b <= 128 for k, b in enumerate(bits) if k != 1)
    out = lp.solve_problems(problems, exact=True, exact_max_bits=256, errorp=False)
    alone = lp.solve_problem(problems[1], exact=True, exact_max_bits=256)
    assert out[1].bits == 256 and out[1]._batch is None
    assert out[1].matrix.tolist() == alone.matrix.tolist() and _trace(out[1]) == _trace(alone)
    assert out[1].basis_columns.tolist() == alone.basis_columns.tolist()
    for k in (0, 2, 3):
        assert out[k]._batch is not None and out[k].bits == 128
        st, trace, t = ec.oracle_outcome(rr.build_tableau(ec.to_dict(problems[k])))
        assert st == "optimal" and _trace(out[k]) == trace and out[k].matrix.tolist() == t.matrix
    # without the option: the declined condition in that member's slot, as before
    out = lp.solve_problems(problems, exact=True, errorp=False)
    assert isinstance(out[1], lp.UnsupportedConstraintError) and out[1].constraint == ("exact", "overflow", "128 bits")
    assert all(out[k]._batch is not None for k in (0, 2, 3))
