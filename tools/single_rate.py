#!/usr/bin/env python
"""What the single-float path (mi355x_stab_*) achieves, recorded, not gated.  Median of --reps runs after a warm-up;
every timed region ends with the status read back.

  1. the LDS-resident solve (k_s_solve) against the select / update pair on small LPs, among them 96 x 300 and 61 x 97:
     pivots/s of a whole solve (upload outside the timed region);
  2. the f32 pair against the f64 per-pivot path (mi355x_tab_* with block size 1, the resident solve off, on the dense
     and on the compact representation) on BASELINE config 2 (1024 x 512) and config 3 (8192 x 4096), the same LP with
     its inputs rounded to float32 values, over a fixed number of pivots;
  3. k_s_update's achieved bytes/s (HIP events around repeated launches) as a share of the 8 TB/s HBM peak, next to
     k_update's on the same shape.

    python tools/single_rate.py [--reps 5] [--pivots 64] [--out profiles/single_rate.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lp = importlib.import_module("linear-programming_amd")
HBM_PEAK = 8e12
PAIR, LDS = 1, 2


def f32_lp(n, m, seed=1234):
    M, b = lp.synth.tableau(n, m, lp.synth.seed_for(9, seed))
    return np.ascontiguousarray(M.astype(np.float32)), b


def single_tableau(M, b):
    return lp.SingleTableau(None, lp.Problem(type="max"), M, b, M.shape[1] - 1, M.shape[0] - 1, {})


def time_single(M, b, form, cap, reps):
    lp.single.set_form(form)
    out = []
    for k in range(reps + 1):
        t = single_tableau(M, b)
        t._h                                                    # upload outside the timed region
        t0 = time.perf_counter()
        st, n = lp.single.solve_status(t, max_pivots=cap, chunk=1 << 30 if cap == 0 else cap)
        dt = time.perf_counter() - t0
        assert t.info()["form"] == form
        if k:
            out.append(n / dt)
        del t
    lp.single.set_form(0)
    return statistics.median(out), n, st


def time_double(M32, b, cap, reps, compact):
    L = lp.capi.lib()
    M = np.ascontiguousarray(M32.astype(np.float64))
    L.mi355x_tune_set_block(1)
    L.mi355x_tune_set_resident(1)
    L.mi355x_tune_set_compact(1 if compact else 0)
    out = []
    try:
        for k in range(reps + 1):
            h = ctypes.c_void_p()
            lp.capi.check(L.mi355x_tab_create(ctypes.byref(h), M.shape[0], M.shape[1], M.ctypes.data_as(ctypes.c_void_p),
                                              b.ctypes.data_as(ctypes.c_void_p), 0), "mi355x_tab_create")
            n = ctypes.c_int64(0)
            t0 = time.perf_counter()
            st = lp.capi.check(L.mi355x_tab_solve(h, 1, 1024.0, cap, ctypes.byref(n)), "mi355x_tab_solve")
            dt = time.perf_counter() - t0
            L.mi355x_tab_destroy(h)
            if k:
                out.append(n.value / dt)
    finally:
        L.mi355x_tune_set_block(0)
        L.mi355x_tune_set_resident(0)
        L.mi355x_tune_set_compact(1)
    return statistics.median(out), n.value, st


def update_rate_single(M, b, launches):
    L = lp.capi.lib()
    lp.single.set_form(PAIR)
    t = single_tableau(M, b)
    ms, nbytes = ctypes.c_double(0), ctypes.c_int64(0)
    lp.capi.check(L.mi355x_stab_debug_update_time(t._h, 0, 0, launches, ctypes.byref(ms), ctypes.byref(nbytes)),
                  "mi355x_stab_debug_update_time")
    lp.single.set_form(0)
    return ms.value * 1e3, nbytes.value, nbytes.value / (ms.value * 1e-3)


def update_rate_double(M32, b, pivots):
    """k_update by the handle's own events (mi355x_tab_timing_*), dense representation, one launch per pivot."""
    L = lp.capi.lib()
    M = np.ascontiguousarray(M32.astype(np.float64))
    L.mi355x_tune_set_block(1)
    L.mi355x_tune_set_resident(1)
    L.mi355x_tune_set_compact(0)
    try:
        h = ctypes.c_void_p()
        lp.capi.check(L.mi355x_tab_create(ctypes.byref(h), M.shape[0], M.shape[1], M.ctypes.data_as(ctypes.c_void_p),
                                          b.ctypes.data_as(ctypes.c_void_p), 0), "mi355x_tab_create")
        npv = ctypes.c_int64(0)
        lp.capi.check(L.mi355x_tab_solve_async(h, 1, 1024.0, 8, 1), "warm")
        L.mi355x_tab_sync(h, ctypes.byref(npv))
        L.mi355x_tab_timing_enable(h, 1)
        lp.capi.check(L.mi355x_tab_solve_async(h, 1, 1024.0, pivots, 0), "run")
        L.mi355x_tab_sync(h, ctypes.byref(npv))
        nl, sm, mn = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
        L.mi355x_tab_timing_read(h, ctypes.byref(nl), ctypes.byref(sm), ctypes.byref(mn))
        ld = ctypes.c_int64(0)
        L.mi355x_tab_shape(h, None, None, ctypes.byref(ld))
        L.mi355x_tab_destroy(h)
    finally:
        L.mi355x_tune_set_block(0)
        L.mi355x_tune_set_resident(0)
        L.mi355x_tune_set_compact(1)
    us = sm.value / max(nl.value, 1) * 1e3
    nbytes = 2 * M.shape[0] * ld.value * 8
    return us, nbytes, nbytes / (us * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pivots", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["single-float path: rates (median of %d after a warm-up)" % args.reps, ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("1. whole solves, LDS form (k_s_solve) against the pair (k_s_select + k_s_update): pivots/s")
    say("   m x n        stored KiB   pivots   LDS          pair         LDS / pair")
    for m, n in ((24, 40), (61, 97), (80, 200), (96, 300), (97, 300)):
        M, b = f32_lp(n, m)
        kib = M.shape[0] * ((M.shape[1] + 3) // 4 * 4) * 4 / 1024
        if single_tableau(M, b).info()["form"] != LDS:
            say("   %-12s %8.1f   does not fit the LDS budget" % ("%d x %d" % (m, n), kib))
            continue
        r_l, k, st = time_single(M, b, LDS, 0, args.reps)
        r_p, k2, st2 = time_single(M, b, PAIR, 0, args.reps)
        assert (k, st) == (k2, st2)
        say("   %-12s %8.1f   %6d   %10.0f   %10.0f   %6.2f" % ("%d x %d" % (m, n), kib, k, r_l, r_p, r_l / r_p))
    say("")
    say("2. f32 pair against the f64 per-pivot path (block size 1), %d pivots of the same LP: pivots/s" % args.pivots)
    say("   config          f32 pair     f64 dense    f64 compact   f32 / f64 dense")
    big = {}
    for name, n, m in (("2 (1024 x 512)", 1024, 512), ("3 (8192 x 4096)", 8192, 4096)):
        M, b = f32_lp(n, m)
        big[name] = (M, b)
        r_s, k, _ = time_single(M, b, PAIR, args.pivots, args.reps)
        r_d, kd, _ = time_double(M, b, args.pivots, args.reps, compact=False)
        r_c, kc, _ = time_double(M, b, args.pivots, args.reps, compact=True)
        assert k == kd == kc == args.pivots
        say("   %-15s %10.0f   %10.0f   %10.0f   %6.2f" % (name, r_s, r_d, r_c, r_s / r_d))
    say("")
    say("3. the update kernels alone (HIP events), dense tableau: us per launch, bytes read + written, share of 8 TB/s")
    for name, (M, b) in big.items():
        us, nb, rate = update_rate_single(M, b, args.pivots)
        say("   config %-15s k_s_update  %8.1f us   %6.1f MB   %5.2f TB/s   %.2f of peak" % (name, us, nb / 1e6, rate / 1e12, rate / HBM_PEAK))
        us, nb, rate = update_rate_double(M, b, args.pivots)
        say("   config %-15s k_update    %8.1f us   %6.1f MB   %5.2f TB/s   %.2f of peak" % (name, us, nb / 1e6, rate / 1e12, rate / HBM_PEAK))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
