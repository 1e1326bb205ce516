"""The wide integer arithmetic under the exact kernels (kernels_exact.inc: u128_mul, s256_*, xmul,
xsub_ovf, xfit, xdiv, xrem, xinv_odd, xctz), primitive by primitive against Python's int, through the
test build's arithmetic probe (mi355x_test_xarith: the same __device__ functions the solve kernels
call, one opcode per launch over a few thousand operand tuples).  Every comparison is exact.

Operands: a hand-written edge list crossed with itself -- 0, +-1, +-(2^k - 1), +-2^k, +-(2^k + 1) around
every limb boundary, the all-ones limb patterns, the most negative value of the width -- plus seeded
random operands whose bit length is itself uniform, so that small and large magnitudes meet."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OP = {"mul64": 0, "mul128": 1, "add256": 2, "sub256": 3, "neg256": 4, "lt256": 5, "subovf64": 6, "subovf128": 7,
      "fit64": 8, "fit128": 9, "div64": 10, "div128": 11, "rem": 12, "inv64": 13, "inv128": 14, "ctz": 15}
X_OVERFLOW, X_INEXACT = 110, 111               # kXOverflow, kXInexact (simplex_kernels.h)
M64 = (1 << 64) - 1
_KS = (31, 32, 33, 62, 63, 64, 65, 95, 96, 126, 127, 128, 129, 191, 192, 193, 254, 255)


def _limbs(values):
    """Python ints -> (n, 4) int64 limbs, little-endian, two's complement at 256 bits."""
    raw = b"".join((int(v) & ((1 << 256) - 1)).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<i8").reshape(len(values), 4).copy()


def _ints(limbs, bits):
    """The low `bits` of every element of an (n, 4) limb array as signed Python ints."""
    out = []
    for row in limbs.tolist():
        v = sum((x & M64) << (64 * k) for k, x in enumerate(row)) & ((1 << bits) - 1)
        out.append(v - (1 << bits) if v >> (bits - 1) else v)
    return out


def _signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def probe(L, op, a, b=None):
    """(out limbs (n, 4), rc (n,)) of one launch of primitive `op` over the operand lists a, b."""
    n = len(a)
    A, B = _limbs(a), _limbs(b if b is not None else [0] * n)
    out = np.full((n, 4), -0x5A5A5A5A, dtype=np.int64)
    rc = np.full(n, -77, dtype=np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert L.mi355x_test_xarith(OP[op], n, p(A), p(B), p(out), p(rc), 0) == 0, L.mi355x_last_error()
    return out, rc


def edges(W):
    """The edge list inside the signed W-bit range, the most negative value included."""
    lo, hi = -(1 << (W - 1)), (1 << (W - 1)) - 1
    vals = {0, 1, -1, lo, hi, -hi}
    for k in _KS:
        for m in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            vals.update((m, -m))
    # all-ones 64-bit limbs: each limb alone, neighbouring pairs, all of them (as W-bit two's complement)
    nl = W // 64
    for i in range(nl):
        vals.add(_signed(M64 << (64 * i), W))
        vals.add(_signed(~(M64 << (64 * i)), W))
        if i + 1 < nl:
            vals.add(_signed(((1 << 128) - 1) << (64 * i), W))
    vals.update((-(1 << 63), -(1 << 127)))
    return sorted(v for v in vals if lo <= v <= hi)


def rand_signed(rng, W, n):
    """n values, bit length uniform in 1 .. W - 1, random sign."""
    out = []
    for _ in range(n):
        bl = rng.randint(1, W - 1)
        v = rng.getrandbits(bl) | (1 << (bl - 1))
        out.append(-v if rng.random() < 0.5 else v)
    return out


def pairs(W, seed, n_random=2000):
    """The edge list crossed with itself, plus random pairs."""
    e = edges(W)
    a = [x for x in e for _ in e]
    b = [y for _ in e for y in e]
    rng = random.Random(seed)
    return a + rand_signed(rng, W, n_random), b + rand_signed(rng, W, n_random)


def test_the_edge_lists_hold_what_they_promise():
    e64, e128 = edges(64), edges(128)
    assert -(1 << 63) in e64 and (1 << 63) - 1 in e64 and 1 << 63 not in e64
    assert {-(1 << 127), -(1 << 63), M64, -(1 << 64), (1 << 127) - 1, (1 << 96) + 1, -((1 << 65) - 1)} <= set(e128)
    assert all(-(1 << 63) <= v < 1 << 63 for v in e64) and all(-(1 << 127) <= v < 1 << 127 for v in e128)
    assert len(e64) >= 30 and len(e128) >= 60 and len(edges(256)) >= 100


@pytest.mark.parametrize("W", [64, 128])
def test_xmul_equals_python(hooks_lib, W):
    a, b = pairs(W, 100 + W)
    if W == 128:
        def mid_carries(x, y):
            x, y = abs(x), abs(y)
            p00, p01, p10 = (x & M64) * (y & M64), (x & M64) * (y >> 64), (x >> 64) * (y & M64)
            return (p00 >> 64) + (p01 & M64) + (p10 & M64) >= 1 << 64
        assert sum(mid_carries(x, y) for x, y in zip(a, b)) >= 100          # u128_mul's (mid >> 64)
        # s256_neg with lo == 0: a negative product whose low 128 bits are zero
        assert sum(x * y < 0 and (x * y) % (1 << 128) == 0 for x, y in zip(a, b)) >= 10
    out, rc = probe(hooks_lib, "mul%d" % W, a, b)
    assert not rc.any()
    assert _ints(out, 2 * W) == [x * y for x, y in zip(a, b)]
    if W == 64:
        assert not out[:, 2:].any()


@pytest.mark.parametrize("op", ["add256", "sub256", "neg256", "lt256"])
def test_s256_operations_equal_python(hooks_lib, op):
    e = edges(256)
    rng = random.Random(7)
    sub = e[::3] + [1 << 128, -(1 << 128), 1 << 192, (1 << 128) - 1, -(1 << 127), 1 << 127]   # (about 50 x 50 pairs)
    a = [x for x in sub for _ in sub] + rand_signed(rng, 256, 2000)
    b = [y for _ in sub for y in sub] + rand_signed(rng, 256, 2000)
    if op == "neg256":
        a = e + rand_signed(rng, 256, 2000)
        assert sum(x != 0 and x % (1 << 128) == 0 for x in a) >= 8 and 0 in a          # lo == 0: the carry into hi
        out, rc = probe(hooks_lib, op, a)
        assert _ints(out, 256) == [_signed(-x, 256) for x in a]
    elif op == "lt256":
        # equal high halves, low halves that differ in their top bit (an unsigned comparison)
        assert sum((x >> 128) == (y >> 128) and ((x >> 127) & 1) != ((y >> 127) & 1) for x, y in zip(a, b)) >= 10
        out, rc = probe(hooks_lib, op, a, b)
        assert out[:, 0].tolist() == [int(x < y) for x, y in zip(a, b)] and not out[:, 1:].any()
    else:
        f = (lambda x, y: x + y) if op == "add256" else (lambda x, y: x - y)
        # a carry / borrow across the 128-bit limb
        if op == "add256":
            assert sum((x % (1 << 128)) + (y % (1 << 128)) >= 1 << 128 for x, y in zip(a, b)) >= 100
        else:
            assert sum((x % (1 << 128)) < (y % (1 << 128)) for x, y in zip(a, b)) >= 100
        out, rc = probe(hooks_lib, op, a, b)
        assert _ints(out, 256) == [_signed(f(x, y), 256) for x, y in zip(a, b)]
    assert not rc.any()


@pytest.mark.parametrize("W", [64, 128])
def test_xsub_ovf_flags_exactly_the_differences_that_leave_the_width(hooks_lib, W):
    a, b = pairs(2 * W, 200 + W)
    out, rc = probe(hooks_lib, "subovf%d" % W, a, b)
    lo, hi = -(1 << (2 * W - 1)), (1 << (2 * W - 1)) - 1
    want = [int(not lo <= x - y <= hi) for x, y in zip(a, b)]
    assert 50 <= sum(want) <= len(want) - 50
    assert rc.tolist() == want
    got = _ints(out, 2 * W)
    assert [g for g, w in zip(got, want) if not w] == [x - y for x, y, w in zip(a, b, want) if not w]


@pytest.mark.parametrize("W", [64, 128])
def test_xfit_accepts_exactly_the_symmetric_range(hooks_lib, W):
    top = (1 << (W - 1)) - 1
    named = [top, -top, -(top + 1), top + 1, -(top + 2), top + 2, 0, 1, -1, 1 << W, -(1 << W), (1 << W) - 1,
             -((1 << W) - 1), (1 << W) + top, -(1 << W) - top - 1, (1 << (2 * W - 1)) - 1, -(1 << (2 * W - 1))]
    a = named + edges(2 * W) + rand_signed(random.Random(300 + W), 2 * W, 3000)
    out, rc = probe(hooks_lib, "fit%d" % W, a)
    want = [int(abs(x) > top) for x in a]
    assert want[:4] == [0, 0, 1, 1]                        # +-(2^(W-1) - 1) accepted, -2^(W-1) and 2^(W-1) refused
    assert rc.tolist() == want
    got = _ints(out, W)
    assert [g for g, w in zip(got, want) if not w] == [x for x, w in zip(a, want) if not w]


def _divisors(W, rng):
    """Positive D below 2^(W-1): odd, 2^k, odd * 2^k; at 128 bits also with 64 and more trailing zeros."""
    top = (1 << (W - 1)) - 1
    odd = [v for v in edges(W) if v > 0 and v & 1] + [v | 1 for v in rand_signed(rng, W, 40) if v > 0]
    D = list(odd)
    D += [1 << k for k in range(W - 1)]
    for k in list(range(1, W - 2, 5)) + ([64, 65, 90, 125] if W == 128 else [61]):
        for o in (3, 5, 0xFFFFFFFF, (1 << 61) - 1, (1 << 63) + 1, rng.getrandbits(W) | 1):
            if (o << k) <= top:
                D.append(o << k)
        o = rng.getrandbits(W - 1 - k) | 1                                  # the widest odd part that fits
        D.append(o << k)
    assert all(0 < d <= top for d in D)
    return sorted(set(D))


@pytest.mark.parametrize("W", [64, 128])
def test_xdiv_quotients_overflow_and_remainders(hooks_lib, W):
    rng = random.Random(400 + W)
    top = (1 << (W - 1)) - 1
    D = _divisors(W, rng)
    tz = lambda d: (d & -d).bit_length() - 1
    assert sum(d & 1 for d in D) >= 20 and sum(d & (d - 1) == 0 for d in D) == W - 1
    assert sum(d & (d - 1) != 0 and not d & 1 for d in D) >= 20
    if W == 128:
        assert sum(d & M64 == 0 and d & (d - 1) != 0 for d in D) >= 8 and sum(tz(d) >= 64 for d in D) >= 60
    qs_fit = [0, 1, -1, 2, -2, top, -top, top - 1, -(top - 1)] + [q for q in edges(W) if abs(q) <= top][::4]
    N, dd, want_rc, want_q = [], [], [], []

    def case(n, d, rc, q=0):
        assert abs(n) < 1 << (2 * W - 1) and (rc == 0) == (n % d == 0 and abs(n // d) <= top)
        assert (rc == X_INEXACT) == (n % d != 0)
        N.append(n); dd.append(d); want_rc.append(rc); want_q.append(q)
    for d in D:
        # exact, the quotient fits (by one bit at +-top)
        for q in qs_fit + rand_signed(rng, W, 6):
            case(q * d, d, 0, q)
        # exact, the quotient misses the symmetric range by one bit or more
        room = 2 * W - 2 - d.bit_length()                       # |q| < 2^room keeps |N| below 2^(2W - 2)
        for q in (top + 1, -(top + 1), top + 2, -(top + 2), 1 << W, -(1 << W), (1 << W) + 1):
            if abs(q).bit_length() <= room:
                case(q * d, d, X_OVERFLOW)
        if room > W:
            q = rng.getrandbits(room) | (1 << (room - 1))
            case(-q * d, d, X_OVERFLOW)
        # a remainder: odd r (the low-bit test when D is even), r a multiple of 2^shift (only the
        # multiply-back catches it), under small, large and too-wide quotients, negative N as well
        if d > 1:
            k, rs = tz(d), []
            rs.append(rng.randrange(1, d) | (0 if d & 1 else 1))
            if d >> k > 1:
                rs += [(rng.randrange(1, d >> k)) << k, 1 << k, d - (1 << k)]
            for r in rs:
                assert 0 < r < d
                for q in (0, 1, rng.getrandbits(W - 2), top, top + 1):
                    if abs(q).bit_length() <= room:
                        case(q * d + r, d, X_INEXACT)
                        case(-(q * d + r), d, X_INEXACT)
    n_even_r = sum(rc == X_INEXACT and (n % d) % (d & -d) == 0 for n, d, rc in zip(N, dd, want_rc))
    assert n_even_r >= 100 and want_rc.count(X_OVERFLOW) >= 100 and want_rc.count(0) >= 1000
    assert sum(n < 0 for n in N) >= len(N) // 3
    out, rc = probe(hooks_lib, "div%d" % W, N, dd)
    bad = [(hex(n), hex(d), w, int(g)) for n, d, w, g in zip(N, dd, want_rc, rc.tolist()) if w != g]
    assert not bad, bad[:5]
    got = _ints(out, W)
    bad = [(hex(n), hex(d), q, g) for n, d, w, q, g in zip(N, dd, want_rc, want_q, got) if w == 0 and q != g]
    assert not bad, bad[:5]


def test_xrem_equals_python(hooks_lib):
    rng = random.Random(500)
    Ns = [v for v in edges(256) if abs(v) < 1 << 255]
    ds = [v for v in edges(128) if 0 < v < 1 << 127]
    a = [n for n in Ns[::2] for _ in ds[::2]] + rand_signed(rng, 256, 2000)
    b = [d for _ in Ns[::2] for d in ds[::2]] + [abs(v) for v in rand_signed(rng, 128, 2000)]
    assert max(abs(n).bit_length() for n in a) == 255 and max(d.bit_length() for d in b) == 127
    out, rc = probe(hooks_lib, "rem", a, b)
    assert not rc.any()
    assert _ints(out, 128) == [abs(n) % d for n, d in zip(a, b)]


@pytest.mark.parametrize("W", [64, 128])
def test_xinv_odd_is_the_inverse_modulo_2_to_the_width(hooks_lib, W):
    rng = random.Random(600 + W)
    a = [v for v in edges(W) if v & 1] + [v | 1 for v in rand_signed(rng, W, 3000)]
    assert len(a) >= 3010 and any(v < 0 for v in a) and -1 in a and (1 << (W - 1)) - 1 in a
    out, rc = probe(hooks_lib, "inv%d" % W, a)
    assert not rc.any()
    got = _ints(out, W)
    assert all((g * d) % (1 << W) == 1 for g, d in zip(got, a))
    assert [g % (1 << W) for g in got] == [pow(d % (1 << W), -1, 1 << W) for d in a]


def test_xctz_counts_on_both_sides_of_bit_64(hooks_lib):
    rng = random.Random(700)
    a = [1 << k for k in range(128)]
    a += [(rng.getrandbits(127 - k) | 1) << k for k in range(127) for _ in range(8)]
    a += [v for v in edges(128) if v]                                       # (negative ones as their bit patterns)
    want = [((v & -v).bit_length() - 1) for v in a]
    assert sum(w >= 64 for w in want) >= 500 and sum(w < 64 for w in want) >= 500 and 63 in want and 64 in want
    out, rc = probe(hooks_lib, "ctz", a)
    assert not rc.any()
    assert out[:, 0].tolist() == want and not out[:, 1:].any()
