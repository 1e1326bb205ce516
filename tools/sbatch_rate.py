#!/usr/bin/env python
"""What batches of single-float LPs (mi355x_sbatch_*) achieve, recorded, not gated.  Every figure is a median of
--reps runs after a warm-up; every timed region is one solve call (it ends with the members' control blocks read
back); uploads are outside the timed regions on both sides.

  1. batches of N members against the same members one by one through mi355x_stab_* (the only route without the
     batch), timed in the same run: pivots/s.  The members are distinct LPs of one shape (up to 256 distinct ones,
     repeated to N); the one-by-one rate is measured on up to 64 of them (it does not depend on N);
  2. 256 against 1024 threads per member at N = 1024, with the members resident per compute unit beside it: where
     the threshold of sbatch_threads_for comes from;
  3. where the batch loses: every shape at which the batch of N = 256 is not faster than one by one.

    python tools/sbatch_rate.py [--reps 5] [--out profiles/sbatch_rate.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lp = importlib.import_module("linear-programming_amd")
DISTINCT = 256


def members(n, m, count):
    out = []
    for k in range(min(count, DISTINCT)):
        M, b = lp.synth.tableau(n, m, lp.synth.seed_for(9, 1234 + k))
        out.append((np.ascontiguousarray(M.astype(np.float32)), b))
    Ms = np.stack([out[k % len(out)][0] for k in range(count)])
    bs = np.stack([out[k % len(out)][1] for k in range(count)])
    return Ms, bs


def time_batch(Ms, bs, threads, reps):
    """-> (pivots/s, pivots per call, info)"""
    lp.single.set_batch_threads(threads)
    rates = []
    try:
        for k in range(reps + 1):
            sb = lp.SingleBatch.from_arrays(Ms, bs)
            info = sb.info()
            t0 = time.perf_counter()
            st, npv = sb.solve(True, 1024, 0)
            dt = time.perf_counter() - t0
            assert not st.any(), "a member did not end MI_OPTIMAL"
            sb.close()
            if k:
                rates.append(int(npv.sum()) / dt)
    finally:
        lp.single.set_batch_threads(0)
    return statistics.median(rates), int(npv.sum()), info


def time_one_by_one(Ms, bs, reps):
    count = min(len(Ms), 64)
    rates = []
    for k in range(reps + 1):
        tabs = [lp.SingleTableau(None, lp.Problem(type="max"), Ms[q], bs[q], Ms.shape[2] - 1, Ms.shape[1] - 1, {})
                for q in range(count)]
        for t in tabs:
            t._h                                                # upload outside the timed region
        t0 = time.perf_counter()
        total = 0
        for t in tabs:
            st, n = lp.single.solve_status(t, chunk=1 << 30)
            assert st == 0
            total += n
        dt = time.perf_counter() - t0
        del tabs
        if k:
            rates.append(total / dt)
    return statistics.median(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["batches of single-float LPs: rates (median of %d after a warm-up)" % args.reps, ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shapes = ((24, 40), (61, 97), (96, 300))
    loses = []
    say("1. a batch of N members (auto workgroup) against the same members one by one (mi355x_stab_*): pivots/s")
    say("   m x n        N      threads   pivots     batch          one by one     batch / one by one")
    for m, n in shapes:
        one = None
        for N in (1, 64, 256, 1024, 4096):
            Ms, bs = members(n, m, N)
            if one is None:
                one = time_one_by_one(*members(n, m, 64), args.reps)
            rate, piv, info = time_batch(Ms, bs, 0, args.reps)
            say("   %-12s %-6d %-9d %-10d %-14.0f %-14.0f %.2f" % ("%d x %d" % (m, n), N, info["workgroup_threads"], piv,
                                                                  rate, one, rate / one))
            if N == 256 and rate <= one:
                loses.append("%d x %d" % (m, n))
    say("")
    say("2. 256 against 1024 threads per member, N = 1024: pivots/s (members resident per compute unit)")
    say("   m x n        stored quads   256 threads          1024 threads         256 / 1024")
    for m, n in ((24, 40), (40, 60), (61, 97), (64, 150), (80, 200), (96, 300)):
        Ms, bs = members(n, m, 1024)
        quads = Ms.shape[1] * ((Ms.shape[2] + 3) // 4)
        r256, _, i256 = time_batch(Ms, bs, 256, args.reps)
        r1024, _, i1024 = time_batch(Ms, bs, 1024, args.reps)
        say("   %-12s %-14d %-12.0f (%2d)   %-12.0f (%2d)   %.2f" % ("%d x %d" % (m, n), quads, r256, i256["members_per_cu"],
                                                                    r1024, i1024["members_per_cu"], r256 / r1024))
    say("")
    say("3. where the batch loses (N = 256 not faster than one by one): %s" % (", ".join(loses) if loses else "nowhere"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
