"""The 256-bit width of the exact solves, without a GPU: the host's wide integer (csrc/xwide.h) through a
stand-alone program built with the host compiler under AddressSanitizer and UBSan and compared with Python
ints, the argument checks of the new entry points, and the Python layer's fallback from a batch to a 256-bit
single tableau with a stubbed batch result."""
import ctypes
import os
import random
import shutil
import subprocess
from math import gcd

import pytest

from tests.helpers import ROOT, lp_amd

lp = lp_amd()
M256, M512 = (1 << 256) - 1, (1 << 512) - 1
TOP = (1 << 255) - 1


def _hex(v, bits=256):
    return "%0*x" % (bits // 4, v & ((1 << bits) - 1))


def _signed(v, bits=256):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _limb_patterns():
    """Every combination of all-ones / all-zero limbs, and their neighbours: each carry and borrow boundary."""
    vals = set()
    for mask in range(16):
        v = sum(((1 << 64) - 1) << (64 * i) for i in range(4) if mask >> i & 1)
        for d in (-1, 0, 1):
            vals.add(_signed(v + d))
    vals.update((TOP, -TOP, -TOP - 1, 0, 1, -1))
    return sorted(vals)


def _rand(rng, bits):
    bl = rng.randint(1, bits - 1)
    v = rng.getrandbits(bl) | (1 << (bl - 1))
    return -v if rng.random() < 0.5 else v


@pytest.fixture(scope="module")
def xwide(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("xwide") / "xwide_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "xwide_check.cpp"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_multiply_with_overflow_flag(xwide):
    rng = random.Random(1)
    e = _limb_patterns()
    pairs = [(a, b) for a in e for b in e[::3]] + [(_rand(rng, 256), _rand(rng, 256)) for _ in range(600)]
    pairs += [(_rand(rng, 128), _rand(rng, 128)) for _ in range(600)]            # products that fit
    pairs += [(1 << 127, 1 << 128), (-(1 << 127), 1 << 128), (1 << 127, -(1 << 128)), (TOP, 1), (-TOP - 1, 1), (-TOP - 1, -1)]
    assert len(pairs) >= 1000
    got = xwide(["mul %s %s" % (_hex(a), _hex(b)) for a, b in pairs])
    n_ok = 0
    for (a, b), g in zip(pairs, got):
        fits = -(1 << 255) <= a * b <= TOP
        n_ok += fits
        assert g == ("ok " + _hex(a * b) if fits else "ovf"), (hex(a), hex(b), g)
    assert 300 <= n_ok <= len(pairs) - 300
    full = xwide(["full %s %s" % (_hex(a), _hex(b)) for a, b in pairs])
    assert full == [_hex(a * b, 512) for a, b in pairs]


def test_divide_and_reduce_by_64_bit_values(xwide):
    rng = random.Random(2)
    ds = [1, 2, 3, 7, (1 << 31) - 1, 1 << 32, (1 << 63) - 1, (1 << 63) - 25, 1 << 62, 10 ** 18]
    cases = [(a, d) for a in _limb_patterns() for d in ds[::2]]
    cases += [(_rand(rng, 256), rng.choice(ds + [rng.randint(1, (1 << 63) - 1)])) for _ in range(1000)]
    got = xwide(["div %s %d" % (_hex(a), d) for a, d in cases])
    for (a, d), g in zip(cases, got):
        q = abs(a) // d * (-1 if a < 0 else 1)                  # C's truncation
        assert g == "%s %d" % (_hex(q), a - q * d), (hex(a), d, g)


def test_lcm_chain_and_its_overflow(xwide):
    rng = random.Random(3)
    primes = [(1 << 61) - 1, (1 << 31) - 1, 1000000007, 998244353, 2305843009213693921, 4611686018427387847, 9223372036854775783]
    chains = [[rng.randint(1, 1 << rng.randint(1, 62)) for _ in range(rng.randint(1, 8))] for _ in range(1000)]
    chains += [[rng.choice(primes[:4]) * rng.randint(1, 3) if rng.random() < 0.5 else rng.choice(primes)
                for _ in range(rng.randint(3, 7))] for _ in range(200)]
    assert all(0 < d < 1 << 63 for c in chains for d in c)
    chains += [[1 << 62, 3 << 61, (1 << 63) - 1, (1 << 62) - 1, (1 << 61) - 1, 1000000007]]
    got = xwide(["lcm " + " ".join(map(str, c)) for c in chains])
    n_ovf = 0
    for c, g in zip(chains, got):
        l, ok = 1, True
        for d in c:
            l = l // gcd(l, d) * d
            if l > TOP:
                ok = False
                break
        n_ovf += not ok
        assert g == ("ok " + _hex(l) if ok else "ovf"), (c, g)
    assert 5 <= n_ovf <= len(chains) - 1000


def test_symmetric_range_at_256_bits(xwide):
    rng = random.Random(4)
    named = [TOP, -TOP, -TOP - 1, 0, 1, -1]
    assert xwide(["sym " + _hex(v) for v in named]) == ["1", "1", "0", "1", "1", "1"]
    wide = named + [TOP + 1, -TOP - 2, 1 << 256, -(1 << 256), (1 << 256) + TOP, (1 << 511) - 1, -(1 << 511)]
    wide += [_signed(v, 512) for v in (M512, M256, M512 ^ M256, 1 << 255, (M512 ^ M256) | (1 << 255))]
    wide += [_rand(rng, 512) for _ in range(500)] + [_rand(rng, 257) for _ in range(500)]
    got = xwide(["fit " + _hex(v, 512) for v in wide])
    assert got == ["ok " + _hex(v) if abs(v) <= TOP else "no" for v in wide]
    assert got[:3] == ["ok " + _hex(TOP), "ok " + _hex(-TOP), "no"]
    pairs = [(a, b) for a in _limb_patterns()[::2] for b in _limb_patterns()[::2]]
    assert xwide(["cmp %s %s" % (_hex(a), _hex(b)) for a, b in pairs]) == ["%d %d" % (a < b, a == b) for a, b in pairs]


def test_argument_validation_without_device():
    L = lp.capi.lib()
    h = ctypes.c_void_p()
    one = (ctypes.c_int64 * 4)(1, 1, 1, 1)
    args = (ctypes.byref(h), 2, 2, one, one, one, 0)
    assert L.mi355x_xtab_create_wide(*args, 0, 192) == lp.capi.MI_BAD_ARG
    assert L.mi355x_xtab_create_wide(*args, 256, 128) == lp.capi.MI_BAD_ARG
    assert L.mi355x_xtab_create_wide(*args, 96, 256) == lp.capi.MI_BAD_ARG
    assert L.mi355x_xtab_create_wide(None, 2, 2, one, one, one, 0, 0, 256) == lp.capi.MI_BAD_ARG
    assert not h.value
    assert L.mi355x_xtab_download_limbs(None, 4, None, None, None) == lp.capi.MI_BAD_ARG
    assert L.mi355x_xtab_download_limbs(None, 3, None, None, None) == lp.capi.MI_BAD_ARG
    fake = ctypes.c_void_p(ctypes.addressof(one))             # limbs is refused before the handle is looked at
    assert L.mi355x_xtab_download_limbs(fake, 3, None, None, None) == lp.capi.MI_BAD_ARG
    assert b"limbs" in L.mi355x_last_error()


def _lp(k):
    return lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1 + k), ("y", 2)],
                      constraints=[("<=", [("x", 1), ("y", 1 + k)], 4 + k), ("<=", [("x", 3), ("y", 1)], 6)])


def test_batch_members_that_overflow_128_bits_fall_back_to_a_single_256_bit_solve(monkeypatch):
    """solve_problems(exact=True, exact_max_bits=256) with a stubbed batch: the member the batch declines is
    solved again alone with 256 bits allowed, the others keep the batch's results."""
    ex = lp.exact
    problems = [_lp(k) for k in range(4)]
    declined = ex._declined(("overflow", "128 bits"))
    other = ex._declined(("start", "basis columns are not unit columns"))
    calls = {"batch": [], "alone": []}

    def fake_batch(members, is_max, device=0, max_pivots=0, min_bits=0, chunk=None):
        calls["batch"].append((len(members), min_bits))
        return ["solved-in-batch-0", declined, other, "solved-in-batch-3"]

    def fake_solver(problem, **kw):
        calls["alone"].append((problems.index(problem), kw["exact_bits"], kw["exact_max_bits"]))
        return "solved-alone"
    monkeypatch.setattr(ex, "solve_exact_batch", fake_batch)
    monkeypatch.setattr(lp.simplex, "mi355x_simplex_solver", fake_solver)
    monkeypatch.setattr(ex.ExactTableau, "_h", property(lambda self: pytest.fail("a device handle was asked for")))
    out = lp.solve_problems(problems, exact=True, exact_max_bits=256, errorp=False)
    assert out == ["solved-in-batch-0", "solved-alone", other, "solved-in-batch-3"]
    assert calls == {"batch": [(4, 0)], "alone": [(1, 0, 256)]}
    # a start width of 256 reaches the one-by-one solves; the batch is asked for at most 128
    calls["batch"].clear(); calls["alone"].clear()
    lp.solve_problems(problems, exact=True, exact_bits=256, exact_max_bits=256, errorp=False)
    assert calls == {"batch": [(4, 128)], "alone": [(1, 256, 256)]}
    # without the option the condition stays in the member's slot, as before
    calls["batch"].clear(); calls["alone"].clear()
    out = lp.solve_problems(problems, exact=True, errorp=False)
    assert out[1] is declined and calls["alone"] == []
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problems(problems, exact=True)


def test_width_arguments_are_checked_up_front():
    p = _lp(0)
    ip = lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1), ("y", 2)],
                    integer_vars=["x"], constraints=[("<=", [("x", 1), ("y", 1)], 4)])
    with pytest.raises(ValueError, match="branch-and-bound"):
        lp.mi355x_simplex_solver(ip, exact=True, branch_and_bound=True, exact_max_bits=256)
    with pytest.raises(ValueError):
        lp.mi355x_simplex_solver(p, exact=True, exact_max_bits=192)
    with pytest.raises(ValueError):
        lp.mi355x_simplex_solver(p, exact=True, exact_bits=256)              # (above the default limit of 128)
    with pytest.raises(ValueError):
        lp.solve_problems([p, p], exact=True, exact_bits=256)
    t = lp.build_tableau(p, p, exact=True, min_bits=256, max_bits=256)
    assert (t.min_bits, t.max_bits) == (256, 256)
    assert lp.exact._declined(("overflow", "256 bits")).constraint == ("exact", "overflow", "256 bits")
    with pytest.raises(lp.UnsupportedConstraintError) as e:
        lp.exact.check(lp.capi.MI_EXACT_OVERFLOW, "x", 256)
    assert e.value.constraint == ("exact", "overflow", "256 bits")
