#!/usr/bin/env python
"""What the GLOBAL form of a single-float batch (mi355x_sbatch_create_global: one workgroup per member, the member's
tableau left in HBM) achieves beyond the LDS budget, recorded, not gated.  Every figure is a median of --reps runs
after a warm-up, with the minimum and maximum beside it; every timed region is one solve call (it ends with the
members' control blocks read back); uploads are outside the timed regions on both sides.

  1. batches of N members at 256 and at 1024 threads against the same members one by one through mi355x_stab_* (the
     route without the batch: the select / update pair), timed in the same run: pivots/s.  The members are distinct
     LPs of one shape (tests/single_cases.py's synthetic generator, up to 256 distinct ones, repeated to N); the
     one-by-one rate is measured on up to 32 of them (it does not depend on N).  "faster": the batch's median is above
     the one-by-one MAXIMUM, i.e. beyond that figure's own spread.  1024 x 2048 (12.7 MB stored, N = 8, 64, 256) extends
     the table of global_batch_min_members beyond the four shapes;
  2. 256 against 1024 threads at two shapes between 98 x 300 and 130 x 1030: where the threshold of sgbatch_threads_for
     lies;
  3. the batch's bytes per pivot against HBM peak at 1024 members of 256 x 512 (about 840 MB: beyond the last-level
     cache);
  4. what the table says about the workgroup and about the fewest members that make a batch.

    python tools/sbatch_global_rate.py [--reps 5] [--out profiles/sbatch_global_rate.txt]
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
from tests import single_cases as sc                       # noqa: E402

DISTINCT = 256
HBM_PEAK = 8.0e12                                            # bytes/s, the data sheet's figure
SHAPES = ((98, 300), (256, 512), (130, 1030), (512, 1024), (1024, 2048))
COUNTS = (2, 8, 64, 256, 1024)
COUNTS_OF = {(1024, 2048): (8, 64, 256)}                     # (1024 of them would be 13 GB)
BETWEEN = ((128, 384), (192, 400))                           # 274 KiB and 458 KiB stored


def members(n, m, count):
    out = [sc.synthetic(n, m, seed=1234 + k) for k in range(min(count, DISTINCT))]
    Ms = np.stack([out[k % len(out)][0] for k in range(count)])
    bs = np.stack([out[k % len(out)][1] for k in range(count)])
    return Ms, bs


def spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def time_batch(Ms, bs, threads, reps):
    """-> ((median, min, max) pivots/s, pivots per call, info)"""
    lp.single.set_batch_global_threads(threads)
    rates = []
    try:
        for k in range(reps + 1):
            sb = lp.SingleBatch.from_arrays(Ms, bs, form="global")
            info = sb.info()
            t0 = time.perf_counter()
            st, npv = sb.solve(True, 1024, 0)
            dt = time.perf_counter() - t0
            assert not st.any(), "a member did not end MI_OPTIMAL"
            sb.close()
            if k:
                rates.append(int(npv.sum()) / dt)
    finally:
        lp.single.set_batch_global_threads(0)
    return spread(rates), int(npv.sum()), info


def time_one_by_one(Ms, bs, reps):
    count = min(len(Ms), 32)
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
    return spread(rates)


def bytes_per_pivot(rows, cols):
    """What one pivot of the global form moves: the update reads and writes every quad that holds a column; pricing
    reads the objective row, the ratio test the entering and the last column (a 4-byte entry per row each), the
    scaling the pivot row."""
    ldl = (cols + 3) // 4 * 4
    return 2 * rows * ldl * 4 + 2 * ldl * 4 + 2 * rows * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="two shapes, N <= 64: a rehearsal of the script")
    args = ap.parse_args()
    lines = ["global-form batches of single-float LPs: rates (median of %d after a warm-up, min .. max)" % args.reps, ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    shapes = SHAPES[:2] if args.quick else SHAPES
    counts_of = {s: (COUNTS[:3] if args.quick else COUNTS_OF.get(s, COUNTS)) for s in shapes}
    table = {}
    say("1. a global-form batch of N members against the same members one by one (mi355x_stab_*): pivots/s")
    say("   m x n        N      threads  pivots    batch    (min .. max)            one by one (min .. max)         batch / one   faster")
    for m, n in shapes:
        one = time_one_by_one(*members(n, m, 32), args.reps)
        for N in counts_of[(m, n)]:
            Ms, bs = members(n, m, N)
            for threads in (256, 1024):
                (med, lo, hi), piv, info = time_batch(Ms, bs, threads, args.reps)
                assert info["form"] == 3 and info["workgroup_threads"] == threads
                faster = med > one[2]
                table[(m, n, N, threads)] = (med, lo, hi, piv, faster)
                say("   %-12s %-6d %-8d %-9d %-8.0f (%8.0f .. %-8.0f)   %-8.0f (%8.0f .. %-8.0f)   %-13.2f %s"
                    % ("%d x %d" % (m, n), N, threads, piv, med, lo, hi, one[0], one[1], one[2], med / one[0],
                       "yes" if faster else "no"))
                flush()
            del Ms, bs
    say("")
    say("2. 256 against 1024 threads between 98 x 300 and 130 x 1030: pivots/s (median, min .. max)")
    say("   m x n        stored bytes   N      256 threads                       1024 threads                      256 / 1024")
    for m, n in () if args.quick else BETWEEN:
        for N in (256, 1024):
            Ms, bs = members(n, m, N)
            r256, _, _ = time_batch(Ms, bs, 256, args.reps)
            r1024, _, _ = time_batch(Ms, bs, 1024, args.reps)
            say("   %-12s %-14d %-6d %-8.0f (%8.0f .. %-8.0f)   %-8.0f (%8.0f .. %-8.0f)   %.2f"
                % ("%d x %d" % (m, n), Ms.shape[1] * ((Ms.shape[2] + 31) // 32 * 32) * 4, N, r256[0], r256[1], r256[2],
                   r1024[0], r1024[1], r1024[2], r256[0] / r1024[0]))
            flush()
    say("")
    key = (256, 512, 1024)
    if all(key + (t,) in table for t in (256, 1024)):
        rows, cols = 257, 769
        per = bytes_per_pivot(rows, cols)
        say("3. bytes per pivot against HBM peak, 1024 members of 256 x 512 (%.0f MB stored): %d bytes per pivot"
            % (1024 * rows * 800 * 4 / 1e6, per))
        for t in (256, 1024):
            med = table[key + (t,)][0]
            say("   %4d threads: %.0f pivots/s x %d bytes = %.2f TB/s = %.0f %% of the %.1f TB/s peak"
                % (t, med, per, med * per / 1e12, 100 * med * per / HBM_PEAK, HBM_PEAK / 1e12))
        say("")
    say("4. per shape: the faster workgroup at every N, and the fewest members from which the batch (at that workgroup) is faster")
    for m, n in shapes:
        counts = counts_of[(m, n)]
        best = {N: max((256, 1024), key=lambda t: table[(m, n, N, t)][0]) for N in counts}
        wins = [N for N in counts if table[(m, n, N, best[N])][4]]
        first = None
        for N in counts:                                     # the first N from which every larger N wins as well
            if all(table[(m, n, K, best[K])][4] for K in counts if K >= N):
                first = N
                break
        rows, ld = m + 1, (m + n + 1 + 31) // 32 * 32
        say("   %-12s stored %-9d bytes   best threads %s   faster at N in %s   from N = %s on"
            % ("%d x %d" % (m, n), rows * ld * 4, " ".join("%d:%d" % (N, best[N]) for N in counts), wins, first))
    flush()


if __name__ == "__main__":
    main()
