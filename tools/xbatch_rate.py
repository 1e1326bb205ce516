#!/usr/bin/env python
"""Wall time of many exact rational LPs: mi355x_solve_problems(ps, exact=True) -- groups of same-shape
members as one batch of exact tableaux, one workgroup per member -- against the one-by-one path,
[solve_problem(p, exact=True) for p in ps], on the same problems in the same run.

Problem sets: 64, 256 and 1024 members of tests/exact_cases.mixed_problem(lp, 6, 3, 2, 1, seed) (two-phase,
artificial 11 x 19 / main 11 x 14, two drive-outs each) and of slack_tableau(32, 32, seed) as max problems
(single phase, 33 x 65).  Per set and path: a warm-up, then the median of --reps runs; pivots/s counts both
phases and the drive-outs of the members that have a solution (a generated member may be unbounded or
infeasible: both paths then hold its condition).  Every batch member's outcome is compared with the
one-by-one result.

Both paths build every member's tableau on the host first (build_tableau(exact=True), Fraction arithmetic in
Python, the same work in both); the columns "after build" time what is left once the tableaux exist --
uploads, solves and hand-overs -- which is where the two paths differ.

The device-built route, mi355x_solve_problems(ps, exact=True, device_build=True), is a third path on the same
sets in the same run: the members are lowered to rows of numerators and denominators (exact_lps.lower_problem)
and their tableaux built on the device (mi355x_xbatch_create_lps).  "built s" is its wall time, "b/built" the
host-built batch's wall time over it, "lower s" the time of the lowering and grouping alone
(exact_lps.group_lowered) and "share" that time's part of "built s".  Every member's outcome is compared with
the host-built batch's.

    python tools/xbatch_rate.py [--counts 64,256,1024] [--reps 5] [--out profiles/xbatch_rate.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lp = importlib.import_module("linear-programming_amd")
from tests import exact_cases as ec                                  # noqa: E402


def slack_problem(m, n, seed):
    """slack_tableau(m, n, seed) as the max problem whose build-tableau result it is."""
    T, _ = ec.slack_tableau(m, n, seed)
    names = ["x%d" % j for j in range(n)]
    cons = [("<=", [(v, int(a)) for v, a in zip(names, T[i, :n])], int(T[i, -1])) for i in range(m)]
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, int(-c)) for v, c in zip(names, T[m, :n])], constraints=cons)


def pivots(sol):
    if isinstance(sol, Exception):
        return 0
    return sum(sol.n_pivots) if isinstance(sol.n_pivots, tuple) else sol.n_pivots


def one_by_one(ps):
    out = []
    for p in ps:
        try:
            out.append(lp.solve_problem(p, exact=True))
        except lp.SolverError as e:
            out.append(e)
    return out


def timed(fn, reps, prepare=None):
    """Median wall time of fn(prepare()) over reps runs after a warm-up; prepare is not timed."""
    times = []
    for k in range(reps + 1):
        arg = prepare() if prepare else None
        t0 = time.perf_counter()
        out = fn(arg) if prepare else fn()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def batch_after_build(plan):
    alone, groups, groups2, failed = plan
    assert not alone and not failed
    for (_, is_max), members in groups.items():
        lp.exact.solve_exact_batch([t for _, t in members], is_max)
    for (_, _, is_max), members in groups2.items():
        lp.exact.solve_exact_batch([(a, t) for _, a, t in members], is_max)


def one_by_one_after_build(tabs):
    for t in tabs:
        try:
            lp.exact.n_solve_exact(t)
        except lp.SolverError:
            pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xbatch_rate.txt"))
    args = ap.parse_args()
    lines = ["# exact LPs: one batch (mi355x_solve_problems(exact=True)) against one by one "
             "(solve_problem(p, exact=True)); median of %d after a warm-up; 'after': the same without the "
             "host's build-tableau, which both paths share; 'built': the batch with device_build=True, 'b/built' "
             "batch s over it, 'lower': its lowering and grouping alone, 'share' their part of 'built'" % args.reps,
             "%-30s %6s %8s %12s %12s %14s %14s %7s %12s %12s %7s %10s %8s %10s %6s" % (
                 "set", "n", "pivots", "batch s", "one-by-one s", "batch piv/s", "1-by-1 piv/s", "ratio",
                 "batch after", "1-by-1 after", "ratio", "built s", "b/built", "lower s", "share")]
    print("\n".join(lines), flush=True)
    sets = (("mixed 6,3,2,1", lambda s: ec.mixed_problem(lp, 6, 3, 2, 1, s)),
            ("slack 32x32", lambda s: slack_problem(32, 32, s)))
    for name, make in sets:
        for n in [int(c) for c in args.counts.split(",")]:
            ps = [make(s) for s in range(n)]
            tb, batch = timed(lambda: lp.solve_problems(ps, exact=True, errorp=False), args.reps)
            t1, single = timed(lambda: one_by_one(ps), args.reps)
            k = sum(pivots(s) for s in batch)
            assert k == sum(pivots(s) for s in single)
            for a, b in zip(batch, single):
                if isinstance(b, Exception):
                    assert type(a) is type(b)
                    continue
                assert a._batch is not None and b._batch is None
                assert lp.solution_objective_value(a) == lp.solution_objective_value(b)
                assert a.basis_columns.tolist() == b.basis_columns.tolist()
            ab, _ = timed(batch_after_build, args.reps, lambda: lp.exact.group_exact_problems(ps))
            a1, _ = timed(one_by_one_after_build, args.reps, lambda: [lp.build_tableau(p, exact=True) for p in ps])
            td, built = timed(lambda: lp.solve_problems(ps, exact=True, device_build=True, errorp=False), args.reps)
            tl, (host, _) = timed(lambda: lp.exact_lps.group_lowered(ps), args.reps)
            assert not host and k == sum(pivots(s) for s in built)
            for a, b in zip(built, batch):
                if isinstance(b, Exception):
                    assert type(a) is type(b)
                    continue
                assert a._batch is not None and a._handle is None
                assert lp.solution_objective_value(a) == lp.solution_objective_value(b)
                assert a.basis_columns.tolist() == b.basis_columns.tolist()
            name_n = "%s (%d solved)" % (name, sum(not isinstance(s, Exception) for s in batch))
            line = "%-30s %6d %8d %12.4f %12.4f %14.0f %14.0f %7.1f %12.4f %12.4f %7.1f %10.4f %8.1f %10.4f %6.2f" % (
                name_n, n, k, tb, t1, k / tb, k / t1, t1 / tb, ab, a1, a1 / ab, td, tb / td, tl, tl / td)
            lines.append(line)
            print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
