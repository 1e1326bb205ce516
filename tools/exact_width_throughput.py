"""Pivots / s of the single exact tableau (mi355x_xtab_*) with 128 bits forced against 256 bits forced.

    python tools/exact_width_throughput.py [--sizes 10,30] [--widths 128,256]

The same assignment LPs as tools/exact_throughput.py (totally unimodular: every value fits 64 bits, so both
widths make the same pivots, which is checked), at two tableau sizes.  Per size and width: the median of 5
solves after a warm-up, the upload outside the timed region.  --widths 128 alone runs on a commit without
the 256-bit width (the 128-bit kernels are the same on both sides of it).  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from exact_throughput import assignment, lp  # noqa: E402


def timed(p, bits):
    kw = {"max_bits": 256} if bits > 128 else {}
    t = lp.build_tableau(p, exact=True, min_bits=bits, **kw)
    t._h                                                   # upload outside the timed region
    t0 = time.perf_counter()
    lp.exact.n_solve_exact(t)
    return t, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,30")
    ap.add_argument("--widths", default="128,256")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    widths = [int(x) for x in a.widths.split(",")]
    for n in [int(x) for x in a.sizes.split(",")]:
        p = assignment(n, n)
        out = {"shape": "assignment", "n": n, "rows": n * 2 + 1, "cols": n * n + 2 * n + 1}
        traces = []
        for bits in widths:
            timed(p, bits)                                 # warm-up: code object, first launches
            runs = [timed(p, bits) for _ in range(a.repeats)]
            t = runs[-1][0]
            assert t.bits == bits
            traces.append((t.pivot_trace().tolist(), t.matrix.tolist()))
            out["pivots"] = len(traces[-1][0])
            out["pivots_per_s_%d" % bits] = out["pivots"] / statistics.median(d for _, d in runs)
        assert all(x == traces[0] for x in traces)
        if 128 in widths and 256 in widths:
            out["ratio_256_over_128"] = out["pivots_per_s_256"] / out["pivots_per_s_128"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
