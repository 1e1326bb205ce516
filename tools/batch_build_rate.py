#!/usr/bin/env python
"""What building a double-precision batch costs: the host-built route (build_tableau per member, np.stack,
mi355x_multibatch_create) against the device-built one (lower_problem_rows per member,
mi355x_multibatch_create_lps), alternating in ONE process on the same members.

Shapes: BASELINE config 4's -- all-`<=` LPs of 256 constraints x 512 variables, tableau 257 x 769 -- at 128 and
1024 members, and a mixed two-phase set of 32 rows x 36 columns (`<=`, `>=`, `=`, negated rows; main tableau
33 x 65, artificial 33 x 77) at 256 and 1024 members.  Per shape and count, the median of --reps runs after a
warm-up of that shape; every timed region ends in a synchronise (the create entries wait for their stream, the
solves read their status back, the read-backs wait for their copy):

  create    from_arrays on tableaux already built (main + artificial)  |  from_lps on rows already lowered
  e2e       solve_problems(ps)  |  solve_problems(ps, from_rows=True)  |  solve_lps(arrays); `lower` is
            group_lowered_rows(ps) alone, `share` its part of the from_rows time.  On the first `e2e-n` members
            only, as many as hold --e2e-terms coefficients: the Problem objects cost Python per coefficient
            on both routes (tens of milliseconds per config-4 member), which is what this leg shows and why
            it can be bounded.
  kernels   device time of k_blp_rows + k_assemble + k_art_objective by HIP events
            (mi355x_batch_lps_timing), the bytes they write -- rows x ld of both tableaux and both bases, from the
            shapes -- and that rate as a share of the HBM peak (8 TB/s).

Every device-built member's result is compared with the host-built one.

    python tools/batch_build_rate.py [--reps 5] [--e2e-terms 134217728] [--out profiles/batch_build_rate.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lp = importlib.import_module("linear-programming_amd")
from tests import lps_cases as lc                                    # noqa: E402

HBM_PEAK = 8.0e12
CAP = 1 << 20


def config4_members(n, seed):
    """n all-`<=` members of max c . x, A x <= b, 256 x 512, A, b, c > 0."""
    rng = np.random.default_rng(seed)
    m, ncv = 256, 512
    L = np.zeros((n, m + 1, ncv + 1))
    L[:, :m, :ncv] = rng.uniform(0.1, 1.0, (n, m, ncv))
    L[:, :m, ncv] = rng.uniform(50.0, 100.0, (n, m))
    L[:, m, :ncv] = -rng.uniform(0.5, 1.5, (n, ncv))
    return L, np.zeros((n, m), dtype=np.int32), True


def mixed_members(n, seed):
    """n two-phase members of min c . x with 32 rows x 36 columns: per 8 rows four `<=`, one `>=`, one `=`, one `>=`
    written with a negative right-hand side (negated: `<=`), one `<=` written so (negated: `>=`); x = 1 is feasible."""
    rng = np.random.default_rng(seed)
    m, ncv = 32, 36
    a = rng.uniform(0.1, 1.0, (n, m, ncv))
    s = a.sum(axis=2)
    L = np.zeros((n, m + 1, ncv + 1))
    sense = np.zeros((n, m), dtype=np.int32)
    for i in range(m):
        k = i % 8
        if k < 4:
            L[:, i, :ncv], L[:, i, ncv] = a[:, i], s[:, i] + 1.0
        elif k == 4:
            L[:, i, :ncv], L[:, i, ncv], sense[:, i] = a[:, i], s[:, i] - 0.05, 1
        elif k == 5:
            L[:, i, :ncv], L[:, i, ncv], sense[:, i] = a[:, i], s[:, i], 2
        elif k == 6:
            L[:, i, :ncv], L[:, i, ncv], sense[:, i] = -a[:, i], -s[:, i] - 1.0, 1
        else:
            L[:, i, :ncv], L[:, i, ncv] = -a[:, i], -s[:, i] + 0.05
    L[:, m, :ncv] = -rng.uniform(0.5, 1.5, (n, ncv))
    return L, sense, False


def host_arrays(L, sense):
    """(main matrices, main bases, artificial matrices, artificial bases) as build_tableau gives them (lc.assemble
    states it; the all-`<=` shape vectorised)."""
    n, m, ncv = L.shape[0], L.shape[1] - 1, L.shape[2] - 1
    if not sense.any() and not (L[:, :m, ncv] < 0).any():
        M = np.zeros((n, m + 1, ncv + m + 1))
        M[:, :, :ncv], M[:, :, -1] = L[:, :, :ncv], L[:, :, ncv]
        M[:, np.arange(m), ncv + np.arange(m)] = 1.0
        return M, np.tile(ncv + np.arange(m, dtype=np.int64), (n, 1)), None, None
    parts = [lc.assemble(L[q], sense[q]) for q in range(n)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4))


def timed(fn, reps):
    """Median wall time of fn() over reps runs after a warm-up, and the last result."""
    times = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def same(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b)
    return np.array_equal(a.matrix.view(np.uint64), b.matrix.view(np.uint64)) and \
        np.array_equal(a.basis_columns, b.basis_columns) and a.n_pivots == b.n_pivots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--devices", type=int, default=1)
    ap.add_argument("--e2e-terms", type=int, default=1 << 27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_build_rate.txt"))
    args = ap.parse_args()
    lib = lp.capi.lib()
    lines = ["# f64 batches: host-built (build_tableau, np.stack, mi355x_multibatch_create) against device-built "
             "(lower_problem_rows, mi355x_multibatch_create_lps) in one process; median of %d after a warm-up of every "
             "shape; 'create': handles from arrays already built / rows already lowered; 'e2e': solve_problems(ps) | "
             "solve_problems(ps, from_rows=True) | solve_lps on the first e2e-n members, 'lower' group_lowered_rows "
             "alone and its share of the from_rows time; 'kernels': the assembly kernels by HIP events, the bytes they "
             "write, share of 8 TB/s" % args.reps,
             "%-22s %6s %11s %11s %7s %6s %10s %10s %7s %10s %9s %6s %10s %9s %8s %6s" % (
                 "shape", "n", "create host", "create dev", "ratio", "e2e-n", "e2e host", "e2e rows", "ratio", "solve_lps",
                 "lower s", "share", "kernels ms", "MB", "GB/s", "peak")]
    print("\n".join(lines), flush=True)
    e2e = {}
    for name, make, counts in (("config 4 257x769", config4_members, (128, 1024)), ("mixed 33x65/77", mixed_members, (256, 1024))):
        for n in counts:
            L, sense, is_max = make(n, 3)
            M, B, A, AB = host_arrays(L, sense)

            def create_host():
                mb = lp.MultiDeviceBatch.from_arrays(M, B, args.devices)
                return mb, (lp.MultiDeviceBatch.from_arrays(A, AB, args.devices) if A is not None else None)
            tch, _ = timed(create_host, args.reps)
            tcd, (main, art) = timed(lambda: lp.MultiDeviceBatch.from_lps(L, sense, args.devices), args.reps)
            G, gb = main.download(n - 1)
            assert np.array_equal(G.view(np.uint64), M[n - 1].view(np.uint64)) and np.array_equal(gb, B[n - 1])
            # the assembly kernels alone
            ms, k = ctypes.c_double(0), ctypes.c_int64(0)
            lib.mi355x_batch_lps_timing(1, None, None)
            lp.MultiDeviceBatch.from_lps(L, sense, args.devices)          # (warm)
            lib.mi355x_batch_lps_timing(1, None, None)
            for _ in range(args.reps):
                lp.MultiDeviceBatch.from_lps(L, sense, args.devices)
            lib.mi355x_batch_lps_timing(0, ctypes.byref(ms), ctypes.byref(k))
            kern_ms = ms.value / args.reps
            ld = lambda c: (c + 15) // 16 * 16
            written = n * ((main.rows * ld(main.cols) + main.rows - 1) + ((art.rows * ld(art.cols) + art.rows - 1) if art else 0)) * 8
            rate = written / (kern_ms * 1e-3)
            del main, art
            # end to end, from Problem objects
            ne = max(2, min(n, args.e2e_terms // (L.shape[1] * L.shape[2])))
            if (name, ne) not in e2e:                                       # (a count already timed at this shape: its figures)
                ps = [lc.problem_of_rows(lp, L[q], sense[q], is_max) for q in range(ne)]
                teh, host = timed(lambda: lp.solve_problems(ps, errorp=False, max_pivots=CAP), args.reps)
                ted, rows = timed(lambda: lp.solve_problems(ps, errorp=False, max_pivots=CAP, from_rows=True), args.reps)
                tl, (alone, _) = timed(lambda: lp.group_lowered_rows(ps), args.reps)
                assert not alone and all(same(a, b) for a, b in zip(rows, host))
                tea, res = timed(lambda: lp.solve_lps(L[:ne], sense[:ne], is_max=is_max, devices=args.devices, max_pivots=CAP), args.reps)
                for q, t in enumerate(host):
                    if not isinstance(t, Exception):
                        assert res[0][q] == 0 and res[2][q, -1] == t.matrix[-1, -1]
                e2e[(name, ne)] = (teh, ted, tl, tea)
                del ps, host, rows
            teh, ted, tl, tea = e2e[(name, ne)]
            line = "%-22s %6d %11.4f %11.4f %7.1f %6d %10.4f %10.4f %7.1f %10.4f %9.4f %6.2f %10.3f %9.1f %8.0f %6.3f" % (
                name, n, tch, tcd, tch / tcd, ne, teh, ted, teh / ted, tea, tl, tl / ted, kern_ms, written / 1e6, rate / 1e9,
                rate / HBM_PEAK)
            lines.append(line)
            print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
