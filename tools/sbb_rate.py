#!/usr/bin/env python
"""Wall time of the single-float branch-and-bound, mi355x_simplex_solver(p, precision="single",
branch_and_bound=True) -- node tableaux assembled on the device (mi355x_sbatch_create_nodes) and read back light
(mi355x_sbatch_readback) -- against the same search (exact_bb.search with the float32 readings) whose every round
builds its nodes on the host (build-tableau with Lisp's contagion) and solves them through
mi355x_solve_problems(precision="single"): the route a user would otherwise have to write.

Part 1: whole searches on three model-terminating cases of tests/single_bb_cases.py at bb_width 1, 8 and 32.
Part 2: one wide set of nodes of ONE depth (--nodes of them, depth 3, on a 33-column assembly base), split into
its pieces: the host lowering per node, the upload (SingleBatch.from_arrays), the assembly call
(mi355x_sbatch_create_nodes: upload of the node rows, k_sbb_assemble, control blocks), and the solve + read-back
that both routes share.

Per measurement: a warm-up, then the median of --reps runs; wall time around calls that end synchronised.

    python tools/sbb_rate.py [--reps 5] [--nodes 512] [--out profiles/sbb_rate.txt]
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
sbb = importlib.import_module("linear-programming_amd.single_bb")
xbb = importlib.import_module("linear-programming_amd.exact_bb")
from tests import single_bb_cases as C                                # noqa: E402

CAP = C.PIVOT_CAP


def host_built_round(problem):
    """The solve_round this commit's public list call gives: every node's problem through
    mi355x_solve_problems(precision="single")."""
    def solve_round(entries):
        ps = [sbb.node_problem(problem, e) for e in entries]
        for p in ps:
            p.integer_vars = []
        out = []
        for p, r in zip(ps, lp.solve_problems(ps, precision="single", errorp=False, max_pivots=CAP)):
            if isinstance(r, Exception):
                out.append((xbb._status_of(r), None, None))
            else:
                out.append((lp.capi.MI_OPTIMAL, lp.tableau_objective_value(r), {v: lp.tableau_variable(r, v) for v in problem.vars}))
        return out
    return solve_round


def run_search(p, width, assembled):
    rounds = sbb.DeviceRounds(p, max_pivots=CAP) if assembled else host_built_round(p)
    return len(xbb.search(p, rounds, width, fractional=sbb.fractional(0), floor=sbb.floor, ceil=sbb.ceil).trace)


def timed(fn, reps):
    times, out = [], None
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# single-float branch-and-bound: nodes assembled on the device against nodes built on the host and solved "
             "through mi355x_solve_problems(precision=\"single\"); median of %d after a warm-up" % a.reps,
             "# part 1: whole searches",
             "%-12s %6s %7s %12s %12s %7s" % ("case", "width", "nodes", "assembled s", "host-built s", "ratio")]
    loses = []
    for name in ("le_7", "ge_0", "eq_22"):
        p = C.to_problem(lp, C.case(name)[0])
        for w in (1, 8, 32):
            ta, na = timed(lambda: run_search(p, w, True), a.reps)
            tb, nb = timed(lambda: run_search(p, w, False), a.reps)
            assert na == nb, (na, nb)
            lines.append("%-12s %6d %7d %12.5f %12.5f %7.2f" % (name, w, na, ta, tb, tb / ta))
            if tb <= ta:
                loses.append("%s at width %d" % (name, w))
            print(lines[-1], flush=True)
    # part 2: one depth, many nodes
    d, n = 3, a.nodes
    base = C.assembly_base(33, d, n_ge=1, seed=1)
    p = C.to_problem(lp, base)
    entries = C.assembly_nodes(7, d, n, 1)
    g = sbb.GeneralFormSingle(p)
    b = sbb.Base(g)
    is_max = p.type == "max"

    def lower():
        return [sbb.host_tableaux(p, e) for e in entries]

    def upload(built):
        return [lp.SingleBatch.from_arrays(np.stack([t[k].matrix for t in built]),
                                           np.stack([t[k].basis_columns for t in built])) for k in (1, 0)]

    def solve(main, art):
        st = art.solve_two_phase(main, is_max, 1024, CAP)[0]
        sbb.readback(main)
        return st
    built = lower()
    t_lower, _ = timed(lower, a.reps)
    t_upload, _ = timed(lambda: upload(built), a.reps)
    t_asm, _ = timed(lambda: b.create_nodes(entries), a.reps)
    t_solve_a, st_a = timed(lambda: solve(*b.create_nodes(entries)), a.reps)
    t_solve_h, st_h = timed(lambda: solve(*upload(built)), a.reps)
    assert np.array_equal(st_a, st_h)
    t_form, _ = timed(lambda: sbb.Base(sbb.GeneralFormSingle(p)).close(), a.reps)
    lines += ["# part 2: %d nodes of depth %d, %d x %d main and %d x %d artificial tableaux" %
              (n, d, g.matrix.shape[0] + d, 33, g.matrix.shape[0] + d, 33 + g.n_art + 1),
              "%-44s %10.5f s" % ("host lowering (build-tableau per node)", t_lower),
              "%-44s %10.5f s" % ("upload (SingleBatch.from_arrays, both)", t_upload),
              "%-44s %10.5f s" % ("host-built total before the solve", t_lower + t_upload),
              "%-44s %10.5f s" % ("device assembly (mi355x_sbatch_create_nodes)", t_asm),
              "%-44s %10.5f s" % ("base: general form + upload, once per search", t_form),
              "%-44s %10.5f s" % ("assembly + solve + light read-back", t_solve_a),
              "%-44s %10.5f s" % ("upload + solve + light read-back", t_solve_h),
              "%-44s %10.2f" % ("ratio before the solve (host-built / assembled)", (t_lower + t_upload) / t_asm),
              "%-44s %10.2f" % ("ratio end to end", (t_lower + t_solve_h) / t_solve_a)]
    if t_lower + t_solve_h <= t_solve_a:
        loses.append("%d nodes of one depth" % n)
    lines.append("# where device assembly loses (not faster than host-built): %s" % (", ".join(loses) or "nowhere"))
    b.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
