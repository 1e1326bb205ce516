"""Exact mode throughput: pivots / s of the fraction-free integer tableaux (mi355x_xtab_*).

    python tools/exact_throughput.py [--sizes 10,30,60] [--oracle-max 12]

Assignment LPs (max sum c_ij x_ij, sum_j x_ij <= 1, sum_i x_ij <= 1) are totally unimodular: D stays 1
and the entries stay small, a growth-free shape large enough to time.  Each size is solved at width 64
and with 128 bits forced (same trace, checked), next to oracle/rational_ref.py on the CPU for sizes up
to --oracle-max.  A dense random rational LP shows the growth: the width it ends at.  One JSON line per
measurement."""
import argparse
import json
import os
import random
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import lp_amd  # noqa: E402

lp = lp_amd()


def assignment(n, seed):
    rng = random.Random(seed)
    names = ["x%d_%d" % (i, j) for i in range(n) for j in range(n)]
    cons = [("<=", [("x%d_%d" % (i, j), 1) for j in range(n)], 1) for i in range(n)]
    cons += [("<=", [("x%d_%d" % (i, j), 1) for i in range(n)], 1) for j in range(n)]
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, rng.randint(1, 1000)) for v in names], constraints=cons)


def dense(n, seed):
    rng = random.Random(seed)
    names = ["x%d" % i for i in range(n)]
    cons = [("<=", [(v, Fraction(rng.randint(1, 30), rng.randint(1, 7))) for v in names], rng.randint(10, 50))
            for _ in range(n)]
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, Fraction(rng.randint(1, 20), rng.randint(1, 5))) for v in names],
                      constraints=cons)


def timed(p, bits):
    t = lp.build_tableau(p, exact=True, min_bits=bits)
    t._h                                                   # upload outside the timed region
    t0 = time.perf_counter()
    lp.exact.n_solve_exact(t)
    dt = time.perf_counter() - t0
    return t, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,30,60")
    ap.add_argument("--oracle-max", type=int, default=12)
    ap.add_argument("--dense", type=int, default=12)
    a = ap.parse_args()
    timed(assignment(4, 0), 64)                            # code object, first launches
    for n in [int(x) for x in a.sizes.split(",")]:
        p = assignment(n, n)
        t64, d64 = timed(p, 64)
        t128, d128 = timed(p, 128)
        tr = t64.pivot_trace().tolist()
        assert tr == t128.pivot_trace().tolist() and t64.matrix.tolist() == t128.matrix.tolist()
        out = {"shape": "assignment", "n": n, "rows": n * 2 + 1, "cols": n * n + 2 * n + 1, "pivots": len(tr),
               "pivots_per_s_64": len(tr) / d64, "pivots_per_s_128": len(tr) / d128, "bits": t64.bits}
        if n <= a.oracle_max:
            import oracle.rational_ref as rr
            from tests import exact_cases as ec
            tabs = rr.build_tableau(ec.to_dict(p))
            t0 = time.perf_counter()
            ref_trace = []
            rr.solve_any(tabs, ref_trace)
            out["oracle_pivots_per_s"] = len(ref_trace) / (time.perf_counter() - t0)
            out["oracle_trace_equal"] = [tuple(x) for x in tr] == ref_trace
        print(json.dumps(out), flush=True)
    p = dense(a.dense, 1)
    try:
        t, d = timed(p, 0)
        print(json.dumps({"shape": "dense", "n": a.dense, "pivots": len(t.pivot_trace()), "seconds": d,
                          "bits": t.bits}), flush=True)
    except lp.UnsupportedConstraintError:
        print(json.dumps({"shape": "dense", "n": a.dense, "declined": "overflow beyond 128 bits"}), flush=True)


if __name__ == "__main__":
    main()
