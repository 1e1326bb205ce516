#!/usr/bin/env python
"""What the pivot rules of the exact batches cost, per pivot and in pivots: --members (256) LPs of the 41 x 341
degenerate slack shape -- tests/exact_cases.slack_tableau(40, 300, seed, rhs=(0, 2), density=0.5), seeds 0 .. --
as ONE batch of exact tableaux (mi355x_xbatch_create / _set_pivot_rule / _solve), under each rule.

Per rule: the pivots made (all members), the wall time of the solve calls alone (the batch is created before
the clock starts, a fresh one per run) and pivots / s, the median of --reps runs after a warm-up; every member
must end MI_OPTIMAL within --cap pivots.

The library is reached through ctypes alone, and --lib names it, so that the same tool times a build of
another commit in the same session; a library without mi355x_xbatch_set_pivot_rule runs the default rule only.

    python tools/xbatch_rule_rate.py [--lib PATH] [--members 256] [--reps 5] [--cap 3000] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import exact_cases as ec                                  # noqa: E402

RULES = (("dantzig", 0), ("bland", 1), ("dantzig-bland", 2))
_p, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def _ptr(a):
    return a.ctypes.data_as(_p)


def load(path):
    L = ctypes.CDLL(path)
    L.mi355x_xbatch_create.argtypes = [ctypes.POINTER(_p), _i64, _i64, _i64, _p, _p, _p, _int, _int]
    L.mi355x_xbatch_solve.argtypes = [_p, _int, _i64, _p, _p]
    L.mi355x_xbatch_destroy.argtypes = [_p]
    L.mi355x_xbatch_destroy.restype = None
    L.mi355x_last_error.restype = ctypes.c_char_p
    if hasattr(L, "mi355x_xbatch_set_pivot_rule"):
        L.mi355x_xbatch_set_pivot_rule.argtypes = [_p, _int]
    return L


def run(L, num, den, basis, rule, cap, chunk):
    """One fresh batch solved to the end in calls of `chunk` pivots: (seconds of the solve calls, pivots)."""
    n, R, C = num.shape
    h = _p()
    assert L.mi355x_xbatch_create(ctypes.byref(h), n, R, C, _ptr(num), _ptr(den), _ptr(basis), 0, 0) == 0, L.mi355x_last_error()
    try:
        if rule:
            assert L.mi355x_xbatch_set_pivot_rule(h, rule) == 0, L.mi355x_last_error()
        st = np.empty(n, dtype=np.int32)
        npv = np.zeros(n, dtype=np.int64)
        total, done = 0, 0
        t0 = time.perf_counter()
        while True:
            assert L.mi355x_xbatch_solve(h, 1, chunk, _ptr(st), _ptr(npv)) == 0, L.mi355x_last_error()
            total += int(npv.sum())
            done += chunk
            if not (st == 3).any() or done >= cap:                    # MI_MAX_PIVOTS: a member left at the call's cap
                break
        dt = time.perf_counter() - t0
        assert (st == 0).all(), "members not optimal within %d pivots: %s" % (cap, sorted(set(st.tolist())))
        return dt, total
    finally:
        L.mi355x_xbatch_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "linear-programming_amd", "libmi355x_simplex.so"))
    ap.add_argument("--label", default="this build")
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=3000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = load(args.lib)
    tabs = [ec.slack_tableau(40, 300, seed, rhs=(0, 2), density=0.5) for seed in range(args.members)]
    num = np.ascontiguousarray(np.stack([T for T, _ in tabs]))
    den = np.ones_like(num)
    basis = np.ascontiguousarray(np.stack([b for _, b in tabs]))
    lines = ["# %s: %d members of the 41 x 341 degenerate slack shape in one exact batch; median of %d after a warm-up"
             % (args.label, args.members, args.reps),
             "%-14s %10s %12s %12s %8s %8s" % ("rule", "pivots", "wall s", "pivots/s", "min s", "max s")]
    print("\n".join(lines), flush=True)
    for name, rule in RULES:
        if rule and not hasattr(L, "mi355x_xbatch_set_pivot_rule"):
            continue
        times, pivots = [], None
        for k in range(args.reps + 1):
            dt, total = run(L, num, den, basis, rule, args.cap, args.chunk)
            assert pivots is None or pivots == total
            pivots = total
            if k:
                times.append(dt)
        med = statistics.median(times)
        line = "%-14s %10d %12.5f %12.0f %8.5f %8.5f" % (name, pivots, med, pivots / med, min(times), max(times))
        lines.append(line)
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
