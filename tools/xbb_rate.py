#!/usr/bin/env python
"""Wall time of the exact branch-and-bound, mi355x_simplex_solver(p, exact=True, branch_and_bound=True), at
bb_width 1, 8 and 32 -- node tableaux assembled on the device (mi355x_xbatch_create_nodes) and read back
light (mi355x_xbatch_readback) -- against the same search (exact_bb.search) whose every round builds its
nodes with build_tableau(exact=True) on the host and solves them through mi355x_solve_problems(exact=True).

Two sets: the reference's integer cases (tests/golden/reference_ilp_cases.json) and the seeded random
rational integer programs of tests/exact_bb_cases.py.  Per set, path and width: a warm-up, then the median
of --reps runs of the whole set; both paths must process the same nodes.

    python tools/xbb_rate.py [--reps 5] [--out profiles/xbb_rate.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lp = importlib.import_module("linear-programming_amd")
xbb = importlib.import_module("linear-programming_amd.exact_bb")
from tests import bb_oracle as B                                      # noqa: E402
from tests import exact_bb_cases as X                                 # noqa: E402


def host_built_round(problem):
    """The solve_round the parent commit can already do: every node through build_tableau(exact=True),
    the round through mi355x_solve_problems(exact=True)."""
    def solve_round(entries):
        ps = [B.node_problem(problem, e, Fraction(1)) for e in entries]
        for p in ps:
            p.integer_vars = []
        out = []
        for p, r in zip(ps, lp.solve_problems(ps, exact=True, errorp=False)):
            if isinstance(r, Exception):
                out.append((xbb._status_of(r), None, None))
            else:
                out.append((lp.capi.MI_OPTIMAL, lp.solution_objective_value(r), {v: lp.solution_variable(r, v) for v in p.vars}))
        return out
    return solve_round


def run_set(problems, width, assembled):
    nodes = 0
    for p in problems:
        rounds = xbb.DeviceRounds(p) if assembled else host_built_round(p)
        nodes += len(xbb.search(p, rounds, width).trace)
    return nodes


def timed(fn, reps):
    times = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        nodes = fn()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = B.load_cases()
    sets = [("reference integer cases", [B.problem_of(cases[n]["problem"], exact=True) for n in sorted(cases)]),
            ("random rational programs", [p for _, p, _ in X.random_cases()])]
    lines = ["# exact branch-and-bound: nodes assembled on the device against nodes built by build_tableau(exact=True) "
             "and solved through mi355x_solve_problems(exact=True); whole set, median of %d after a warm-up" % a.reps,
             "%-28s %6s %7s %12s %12s %7s" % ("set", "width", "nodes", "assembled s", "host-built s", "ratio")]
    for name, ps in sets:
        for w in (1, 8, 32):
            ta, na = timed(lambda: run_set(ps, w, True), a.reps)
            tb, nb = timed(lambda: run_set(ps, w, False), a.reps)
            assert na == nb, (na, nb)
            lines.append("%-28s %6d %7d %12.4f %12.4f %7.2f" % (name, w, na, ta, tb, tb / ta))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
