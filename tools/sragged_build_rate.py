#!/usr/bin/env python3
"""What RAGGED single-float batches BUILT ON THE DEVICE (mi355x_sbatch_create_lps_ragged, _create_nodes_ragged) achieve
against the parent commit's routes, recorded, not gated.  Every figure is the median of 5 runs after a warm-up, with
minimum and maximum; the two sides of a comparison run in turn.

  (a) 256 Problems of 256 distinct shapes, single-phase, and the same count two-phase; create, solve and download timed:
      solve_problems_single_from_rows(ps, mixed_shapes=True) against solve_problems_single_from_rows(ps) (every member
      alone) and against solve_problems(ps, precision="single", mixed_shapes=True) (the host-built ragged batch)
  (b) create alone, 1024 members over 16 shapes: from_lps_ragged against from_ragged of host-built tableaux
  (c) whole branch-and-bound searches (tools/sbb_rate.py's problems) at bb_width 4 / 16 / 64 with and without
      mixed_shapes=True; creates per round

    python tools/sragged_build_rate.py [--out profiles/sragged_build_rate.txt] [--quick]
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
F32 = np.float32
OUT = []


def say(text=""):
    print(text, flush=True)
    OUT.append(text)


def timed(fns, runs=5):
    """The sides in turn, `runs` times after one warm-up each -> per side (median, min, max) in ms."""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return "%9.2f ms (%.2f .. %.2f)" % t


def problem(m, ncv, seed, two_phase):
    rng = np.random.default_rng(seed)
    names = ["x%d" % j for j in range(ncv)]
    x0 = rng.integers(1, 4, size=ncv)
    cons = []
    for i in range(m):
        a = rng.integers(1, 24, size=ncv)
        ge = two_phase and i % 3 == 0
        rhs8 = int(a @ x0) + (-1 if ge else 1) * int(rng.integers(1, 8))
        cons.append((">=" if ge else "<=", [(v, F32(int(k)) / F32(8)) for v, k in zip(names, a)], F32(rhs8) / F32(8)))
    return lp.Problem(type="max" if seed % 2 else "min", vars=names, objective_var="w",
                      objective_func=[(v, F32(int(c)) / F32(4)) for v, c in zip(names, rng.integers(1, 9, size=ncv))],
                      constraints=cons)


def part_a(count):
    say("(a) %d Problems of %d distinct shapes (m 3..18 x ncv 4..19): create + solve + download" % (count, count))
    for two in (False, True):
        ps = [problem(3 + k // 16, 4 + k % 16, k, two) for k in range(count)]
        rows = lp.single_lps.solve_problems_single_from_rows
        sides = [lambda: rows(ps, mixed_shapes=True, errorp=False, max_pivots=400),
                 lambda: rows(ps, errorp=False, max_pivots=400),
                 lambda: lp.solve_problems(ps, precision="single", mixed_shapes=True, errorp=False, max_pivots=400)]
        r = timed(sides, runs=5)
        kind = "two-phase" if two else "single-phase"
        say("    %-12s from rows, ragged (device-built) %s" % (kind, fmt(r[0])))
        say("    %-12s from rows, parent (one by one)   %s   %.2f x" % (kind, fmt(r[1]), r[1][0] / r[0][0]))
        say("    %-12s host-built ragged batch          %s   %.2f x" % (kind, fmt(r[2]), r[2][0] / r[0][0]))
    say("    by member count (single-phase), ragged from rows against one by one:")
    for n in (2, 4, 8, 16, 64):
        ps = [problem(3 + k // 16, 4 + k % 16, k, False) for k in range(n)]
        rows = lp.single_lps.solve_problems_single_from_rows
        r = timed([lambda: rows(ps, mixed_shapes=True, errorp=False, max_pivots=400),
                   lambda: rows(ps, errorp=False, max_pivots=400)])
        say("      %3d members  %s  against %s   %.2f x" % (n, fmt(r[0]), fmt(r[1]), r[1][0] / r[0][0]))


def part_b(count):
    say("(b) create alone, %d members over 16 shapes" % count)
    for two in (False, True):
        ps = [problem(3 + k % 16, 4 + k % 16, k, two) for k in range(count)]
        lows = [lp.single_lps.lower_problem_rows_single(p) for p in ps]
        tabs = [lp.single.build_tableau_single(p) for p in ps]
        mains = [t[1] if two else t for t in tabs]
        arts = [t[0] for t in tabs] if two else None

        def device():
            made = lp.SingleBatch.from_lps_ragged([w.L for w in lows], [w.sense for w in lows], [w.is_max for w in lows],
                                                  [w.col_int_sum for w in lows])
            for b in made:
                if b is not None:
                    b.close()

        def host():
            made = [lp.SingleBatch.from_ragged([t.matrix for t in mains], [t.basis_columns for t in mains],
                                               [t.is_max for t in mains])]
            if two:
                made.append(lp.SingleBatch.from_ragged([t.matrix for t in arts], [t.basis_columns for t in arts], None))
            for b in made:
                b.close()
        r = timed([device, host])
        say("    %-12s device-built %s   upload of host-built tableaux %s   %.2f x" %
            ("two-phase" if two else "single-phase", fmt(r[0]), fmt(r[1]), r[1][0] / r[0][0]))


def part_c():
    from tests import single_bb_cases as C                            # (tools/sbb_rate.py's problems)
    problems = [(name, C.to_problem(lp, C.case(name)[0])) for name in ("le_7", "ge_0", "eq_22")]
    say("(c) whole searches, mixed_shapes=True against without")
    for name, p in problems:
        for width in (4, 16, 64):
            stats = {}

            def run(mixed):
                s = lp.single_bb.SingleBranchAndBound(p, width=width, max_pivots=400, **({"mixed_shapes": True} if mixed else {}))
                try:
                    s.run()
                except lp.SolverError:
                    pass
                stats[mixed] = (s.rounds.n_creates, s.rounds.n_create_rounds, len(s.trace()), s.rounds.ragged_batched)
            r = timed([lambda: run(True), lambda: run(False)])
            per = {k: "%.2f" % (v[0] / max(1, v[1])) for k, v in stats.items()}
            say("    %-6s width %2d  %2d nodes, %2d in ragged batches  ragged %s (%s creates / round)  parent %s (%s)   %.2f x" %
                (name, width, stats[True][2], stats[True][3], fmt(r[0]), per[True], fmt(r[1]), per[False], r[1][0] / r[0][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sragged_build_rate.txt"))
    ap.add_argument("--quick", action="store_true", help="64 / 256 members instead of 256 / 1024")
    a = ap.parse_args()
    say("ragged single-float batches built on the device: median of 5 after a warm-up (min .. max), sides in turn")
    part_a(64 if a.quick else 256)
    part_b(256 if a.quick else 1024)
    part_c()
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
