#!/usr/bin/env python
"""What RAGGED batches of single-float LPs (mi355x_sbatch_create_ragged) achieve, recorded, not gated.  Every figure
is a median of --reps runs after a warm-up, with the smallest and the largest run beside it where a rule rests on the
spread; the two sides of a comparison are run in turn.

  1. N members of ONE shape as a ragged batch against the same members as a batch of one shape
     (mi355x_sbatch_create), at 24 x 40, 61 x 97 and 96 x 300 and N = 16 ... 4096 (the routing rule of single.py rests on
     the rows at 256; RAGGED_UNIFORM_MIN_MEMBERS is read off the other counts): what the member list, the
     descriptor load and the per-member sense cost where the uniform batch already applies.  Timed: one solve call,
     uploads outside.
  2. 256 members over 16 shapes, 16 of each, four shapes in each occupancy class: ONE ragged batch against the route
     without mixed_shapes -- 16 batches of one shape, one after the other.
  3. 256 members of 256 distinct shapes: ONE ragged batch against the route without mixed_shapes -- one by one through
     mi355x_stab_*.
     2 and 3 time what solve_problems_single does with built tableaux on either route: create (upload included), solve,
     download of every member.  build-tableau on the host is the same work on both routes and is left out.
  4. the list of 2 with the classes hook at 4 (one launch per occupancy class) against the hook at 1 (one launch per
     round at the largest member's LDS size).  Timed: one solve call, uploads outside.
  5. the same two settings where residency could matter: 4095 members of 24 x 40 and one of 96 x 300.

    python tools/sbatch_ragged_rate.py [--reps 5] [--out profiles/sbatch_ragged_rate.txt]
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
CAP = 1 << 20
#: m x n, four per occupancy class at 256 threads (4, 3, 2, 1 members per compute unit)
SIXTEEN = ((24, 40), (30, 50), (40, 60), (16, 100), (61, 97), (60, 110), (64, 120), (50, 150),
           (64, 150), (70, 160), (72, 180), (60, 200), (80, 200), (85, 220), (90, 250), (96, 300))


def member(m, n, k):
    M, b = lp.synth.tableau(n, m, lp.synth.seed_for(9, 1234 + k))
    return np.ascontiguousarray(M.astype(np.float32)), b


def medians_of(runs, reps):
    """runs: functions -> (pivots, seconds), taken in turn (a, b, a, b, ...: neither side has the warmer device);
    -> per function (median, min, max) of pivots/s over reps runs after a warm-up"""
    rates = [[] for _ in runs]
    for k in range(reps + 1):
        for out, run in zip(rates, runs):
            piv, dt = run()
            if k:
                out.append(piv / dt)
    return [(statistics.median(r), min(r), max(r)) for r in rates]


def solve_ragged(members, classes=0):
    lp.single.set_batch_ragged_classes(classes)
    try:
        sb = lp.SingleBatch.from_ragged([M for M, _ in members], [b for _, b in members], [True] * len(members))
    finally:
        lp.single.set_batch_ragged_classes(0)
    t0 = time.perf_counter()
    st, npv = sb.solve(None, 1024, CAP)
    dt = time.perf_counter() - t0
    assert not st.any(), "a member did not end MI_OPTIMAL"
    info = sb.info()
    classes_seen = sorted({sb.member_shape(q)["occupancy_class"] for q in range(sb.n_lps)})
    sb.close()
    return int(npv.sum()), dt, info, classes_seen


def solve_uniform(members):
    sb = lp.SingleBatch.from_arrays(np.stack([M for M, _ in members]), np.stack([b for _, b in members]))
    t0 = time.perf_counter()
    st, npv = sb.solve(True, 1024, CAP)
    dt = time.perf_counter() - t0
    assert not st.any(), "a member did not end MI_OPTIMAL"
    sb.close()
    return int(npv.sum()), dt


def route_ragged(members):
    t0 = time.perf_counter()
    sb = lp.SingleBatch.from_ragged([M for M, _ in members], [b for _, b in members], [True] * len(members))
    st, npv = sb.solve(None, 1024, CAP)
    for q in range(sb.n_lps):
        sb.download(q)
    sb.close()
    dt = time.perf_counter() - t0
    assert not st.any()
    return int(npv.sum()), dt


def route_grouped(members):
    """The route without mixed_shapes: a group of one shape is a batch, a member alone goes through mi355x_stab_*."""
    groups = {}
    for M, b in members:
        groups.setdefault(M.shape, []).append((M, b))
    total = 0
    t0 = time.perf_counter()
    for group in groups.values():
        if len(group) > 1:
            sb = lp.SingleBatch.from_arrays(np.stack([M for M, _ in group]), np.stack([b for _, b in group]))
            st, npv = sb.solve(True, 1024, CAP)
            for q in range(sb.n_lps):
                sb.download(q)
            sb.close()
            assert not st.any()
            total += int(npv.sum())
        else:
            M, b = group[0]
            t = lp.SingleTableau(None, lp.Problem(type="max"), M, b, M.shape[1] - 1, M.shape[0] - 1, {})
            st, n = lp.single.solve_status(t, max_pivots=CAP)
            t.matrix
            assert st == 0
            total += n
    return total, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["ragged batches of single-float LPs: rates (median of %d after a warm-up)" % args.reps, ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("1. N members of one shape: ragged batch against the batch of one shape, one solve call: pivots/s")
    say("   m x n        N      pivots     ragged (min .. max)                      uniform (min .. max)                     ragged / uniform")
    slower, slower_256 = [], []
    for m, n in ((24, 40), (61, 97), (96, 300)):
        distinct = [member(m, n, k) for k in range(256)]
        for count in (16, 64, 256, 1024, 4096):
            ms = [distinct[k % 256] for k in range(count)]
            r, u = medians_of((lambda: solve_ragged(ms)[:2], lambda: solve_uniform(ms)), args.reps)
            piv = solve_uniform(ms)[0]
            below = r[0] < u[1]                               # below the uniform figure's own run-to-run spread
            say("   %-12s %-6d %-10d %-12.0f (%-12.0f .. %-12.0f) %-12.0f (%-12.0f .. %-12.0f) %.3f%s"
                % ("%d x %d" % (m, n), count, piv, r[0], r[1], r[2], u[0], u[1], u[2], r[0] / u[0], " *" if below else ""))
            if below:
                (slower_256 if count == 256 else slower).append("%d x %d at %d" % (m, n, count))
    say("   * ragged below the uniform figure's own spread (its smallest run) at N = 256, the rows the routing rule")
    say("     of single.py rests on: %s; at the other counts: %s"
        % (", ".join(slower_256) if slower_256 else "nowhere", ", ".join(slower) if slower else "nowhere"))
    say("")

    sixteen = [member(m, n, 16 * s + k) for s, (m, n) in enumerate(SIXTEEN) for k in range(16)]
    order = np.random.default_rng(7).permutation(len(sixteen))
    sixteen = [sixteen[k] for k in order]                      # list order: the shapes interleaved
    _, _, info, classes_seen = solve_ragged(sixteen, 4)
    say("2. 256 members over 16 shapes (16 of each; occupancy classes %s): create + solve + download of every member"
        % (classes_seen,))
    r, g = medians_of((lambda: route_ragged(sixteen), lambda: route_grouped(sixteen)), args.reps)
    piv = route_ragged(sixteen)[0]
    say("   pivots     one ragged batch     16 batches of one shape     ragged / grouped")
    say("   %-10d %-20.0f %-27.0f %.2f" % (piv, r[0], g[0], r[0] / g[0]))
    say("")

    distinct = [member(m, n, 16 * (m - 8) + (n - 20)) for m in range(8, 24) for n in range(20, 36)]
    assert len({M.shape for M, _ in distinct}) == 256
    say("3. 256 members of 256 distinct shapes (8..23 x 20..35): create + solve + download of every member")
    r, g = medians_of((lambda: route_ragged(distinct), lambda: route_grouped(distinct)), args.reps)
    piv = route_ragged(distinct)[0]
    say("   pivots     one ragged batch     one by one (mi355x_stab_*)  ragged / one by one")
    say("   %-10d %-20.0f %-27.0f %.2f" % (piv, r[0], g[0], r[0] / g[0]))
    say("")

    def classes_against_one(members):
        a, o = medians_of((lambda: solve_ragged(members, 4)[:2], lambda: solve_ragged(members, 1)[:2]), args.reps)
        say("   a launch per class (min .. max)          one class (min .. max)                   per class / one class")
        say("   %-12.0f (%-12.0f .. %-12.0f) %-12.0f (%-12.0f .. %-12.0f) %.2f"
            % (a[0], a[1], a[2], o[0], o[1], o[2], a[0] / o[0]))

    say("4. the list of 2, one solve call: the hook at 4 (one launch per occupancy class) against 1 (one launch)")
    classes_against_one(sixteen)
    say("")
    say("5. 4095 members of 24 x 40 and one of 96 x 300, one solve call: the same two settings")
    small = [member(24, 40, k) for k in range(256)]
    classes_against_one([small[k % 256] for k in range(2047)] + [member(96, 300, 0)] + [small[k % 256] for k in range(2048)])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
