"""Branch-and-bound throughput: a seeded synthetic multi-constraint integer knapsack (default 64
binary-bounded variables x 32 `<=` rows, max) searched by the library's branch-and-bound job
(mi355x_simplex_solver_bb_*) with a fixed node budget, at several widths of speculative node
batches.  Prints one JSON line per width: nodes processed / s, node LPs solved / s (speculative
ones included), the deepest node, and whether the trace equals the width-1 trace.

    python tools/bb_throughput.py [--vars 64] [--rows 32] [--max-nodes 100] [--widths 1,16,256]
                                  [--int-tolerance 1024]

With exact integrality (the product default) the knapsack dives on values a few ulps off an integer,
as the reference would; the node budget bounds the run.  A last line compares assembling
--assembly-nodes node tableaux of one depth on the device (k_assemble, through the test hook
mi355x_bb_debug_assemble, download included) with the host build-tableau of the same nodes, and gives
the bytes per node the device assembly keeps off PCIe.

Node tableaux of depth >= 1 are assembled on the device by k_assemble; the per-kernel view comes
from running this under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.bb_oracle import node_problem, trace_key  # noqa: E402
from tests.helpers import lp_amd  # noqa: E402

lp = lp_amd()


def knapsack(n, m, seed):
    rng = np.random.default_rng(seed)
    names = ["x%d" % i for i in range(n)]
    w = rng.integers(5, 60, size=(m, n)).astype(float)
    cap = np.floor(w.sum(axis=1) / 2.0) + 0.5
    v = rng.integers(10, 100, size=n).astype(float)
    return lp.Problem(type="max", vars=names, objective_func=list(zip(names, v.tolist())),
                      integer_vars=[names[i] for i in rng.permutation(n)],
                      var_bounds=[(x, (0.0, 1.0)) for x in names],
                      constraints=[("<=", list(zip(names, w[r].tolist())), float(cap[r])) for r in range(m)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vars", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--max-nodes", type=int, default=100)
    ap.add_argument("--int-tolerance", type=float, default=0.0)
    ap.add_argument("--assembly-nodes", type=int, default=256)
    ap.add_argument("--widths", default="1,16,256")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    if lp.capi.device_count() < 1:
        raise SystemExit("needs a GPU")
    p = knapsack(a.vars, a.rows, a.seed)
    ref = None
    for w in [int(x) for x in a.widths.split(",")]:
        bb = lp.native.BranchAndBound(p, width=w, int_tolerance=a.int_tolerance)
        t0 = time.perf_counter()
        done, rc = 0, lp.capi.MI_MAX_PIVOTS
        while rc == lp.capi.MI_MAX_PIVOTS and done < a.max_nodes:
            rc, k = bb.step(min(64, a.max_nodes - done))
            done += k
        dt = time.perf_counter() - t0
        st, tr = bb.stats(), bb.trace()
        if ref is None:
            ref = tr
        same = trace_key(tr) == trace_key(ref[:len(tr)]) if len(tr) <= len(ref) else False
        print(json.dumps({"width": w, "status": rc, "nodes": st["processed"], "node_lps": st["solved"],
                          "max_depth": st["max_depth"], "seconds": round(dt, 4),
                          "nodes_per_s": round(st["processed"] / dt, 1), "node_lps_per_s": round(st["solved"] / dt, 1),
                          "trace_equals_width1": same}), flush=True)
    assembly(p, a.assembly_nodes, a.seed)


def assembly(p, n, seed):
    """n nodes of depth 4 with no artificial rows: device assembly (k_assemble + download) against
    the host build-tableau of the same node problems."""
    import ctypes
    rng = np.random.default_rng(seed)
    npb = lp.native.NativeProblem(p)
    nodes = [tuple((p.vars[int(rng.integers(0, len(p.vars)))], 0, 0.0) for _ in range(4)) for _ in range(n)]
    var = np.array([[npb.index[v] for v, _, _ in q] for q in nodes], np.int64)
    sen = np.zeros((n, 4), np.int32)
    bnd = np.zeros((n, 4))
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    L = lp.capi.lib()
    R, C, AC = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    args = [npb._h, n, 4, ptr(var), ptr(sen), ptr(bnd), 0, ctypes.byref(R), ctypes.byref(C), ctypes.byref(AC)]
    lp.capi.check(L.mi355x_bb_debug_assemble(*args, None, None, None, None), "assemble")
    M = np.empty((n, R.value, C.value)); MB = np.empty((n, R.value - 1), np.int64)
    best = []
    for _ in range(3):
        t0 = time.perf_counter()
        lp.capi.check(L.mi355x_bb_debug_assemble(*args, ptr(M), ptr(MB), None, None), "assemble")
        best.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for q in nodes:
        lp.native.NativeProblem(node_problem(p, q)).build_tableau()
    host = time.perf_counter() - t0
    print(json.dumps({"assembly_nodes": n, "rows": R.value, "cols": C.value,
                      "device_assemble_plus_download_s": round(min(best), 5), "host_build_s": round(host, 5),
                      "tableau_bytes_per_node": R.value * C.value * 8,
                      "note": "device time includes downloading every tableau (the search itself downloads none)"}),
          flush=True)


if __name__ == "__main__":
    main()
