#!/usr/bin/env python
"""What building GLOBAL-form single-float batches on the device (mi355x_sbatch_create_lps_global,
mi355x_sbatch_create_nodes_global) achieves against the routes of the parent commit, timed in the same run; recorded,
not gated.  Every figure is the median of --reps runs after a warm-up, with the minimum and the maximum, unless the
line says otherwise.  The baseline of a table is never the new route itself.

  (a) create alone   SingleBatch.from_lps(rows, form="global")  against  build_tableau_single per member +
                     SingleBatch.from_arrays(tableaux, form="global").  build_tableau_single is Python per
                     coefficient: it is timed on --built members (no warm-up, median over them) and multiplied by the
                     member count -- the line says "x N"; the upload is timed on the whole batch (the built members
                     repeated).  write: the write pass alone by HIP events (mi355x_sbatch_lps_global_timing), its bytes
                     -- both tableaux stored once, the members' rows read once -- over its time as a share of 8 TB/s.
  (b) the list route solve_problems_single_from_rows(ps, beyond_lds=True)  against  solve_problems_single(ps,
                     beyond_lds=True) from Problem objects at 256 x 512; `lower` is group_lowered_rows_single(ps) alone.
  (c) a whole search mi355x_simplex_solver(p, precision="single", branch_and_bound=True, bb_width=W, beyond_lds=True)
                     against beyond_lds=False (node by node), on a problem whose nodes are beyond the LDS budget.

    python tools/slps_global_rate.py [--reps 5] [--out profiles/slps_global_rate.txt]
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
F32 = np.float32
N_ART = 6
PEAK = 8e12                                                  # bytes per second


def rows_of(n, m, distinct, two_phase):
    """-> (L distinct x (m + 1) x (n + 1) float32, sense distinct x m): synth.tableau's numbers as problem rows, every
    fourth row a `>=` row with both sides negated (flipped back into `<=`); two_phase: the last 6 rows artificial."""
    Ls, ss = [], []
    for k in range(distinct):
        M, _ = lp.synth.tableau(n, m, lp.synth.seed_for(9, 4321 + k))
        M = M.astype(F32)
        L = np.concatenate([M[:, :n], M[:, -1:]], axis=1)
        sense = np.zeros(m, dtype=np.int32)
        L[:m - N_ART:4] *= F32(-1)
        sense[:m - N_ART:4] = 1
        if two_phase:
            L[m - N_ART:m, -1] *= F32(0.01)
            sense[m - N_ART:m - N_ART // 2] = 1
            L[m - N_ART // 2:m] *= F32(-1)
        Ls.append(L)
        ss.append(sense)
    return np.stack(Ls), np.stack(ss)


def problems_of(L, sense):
    ops = ("<=", ">=", "=")
    n = L.shape[2] - 1
    names = ["x%d" % j for j in range(n)]
    out = []
    for Lq, sq in zip(L, sense):
        cons = [(ops[s], list(zip(names, row[:n])), row[n]) for row, s in zip(Lq[:-1], sq)]
        out.append(lp.Problem(type="max", vars=names, objective_var="w", objective_func=list(zip(names, -Lq[-1, :n])),
                              constraints=cons))
    return out


def repeat(a, count):
    return np.concatenate([a] * (count // a.shape[0] + 1))[:count]


def timed(fn, reps):
    """-> ((median, min, max) seconds after one warm-up, the last result)."""
    ts, out = [], None
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if k:
            ts.append(time.perf_counter() - t0)
    return (statistics.median(ts), min(ts), max(ts)), out


def ms(t):
    return "%9.2f [%8.2f, %8.2f]" % tuple(x * 1e3 for x in t)


def close(*batches):
    for b in batches:
        if b is not None:
            b.close()


def write_pass_ms():
    r, w, o = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    lp.capi.check(lp.capi.lib().mi355x_sbatch_lps_global_timing(1, ctypes.byref(r), ctypes.byref(w), ctypes.byref(o)),
                  "mi355x_sbatch_lps_global_timing")
    return r.value, w.value, o.value


def bb_problem(rows=200, seed=3):
    """Three integer variables (z free), `rows` constraint rows of which all but five never bind: every node tableau
    is beyond the LDS budget."""
    rng = np.random.default_rng(seed)

    def quarter(lo, hi):
        k = int(rng.integers(4 * lo, 4 * hi))
        return k // 4 if k % 4 == 0 else F32(k / 4)
    names = ["x", "y", "z"]
    cons = [("<=", [(v, quarter(1, 5)) for v in names], quarter(8, 20)) for _ in range(3)]
    cons += [("<=", [("z", 1)], F32(2.5)), ("<=", [("z", -1)], F32(1.5))]
    cons += [("<=", [("x", 1), ("y", 1)], 100 + i) for i in range(rows - len(cons))]
    return lp.Problem(type="max", vars=names, objective_var="w", objective_func=[(v, quarter(1, 6)) for v in names],
                      var_bounds=[("z", (None, None))], constraints=cons, integer_vars=names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--built", type=int, default=2, help="members build_tableau_single is timed on, per shape and form")
    ap.add_argument("--list-members", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("global-form single-float batches built on the device against the parent commit's routes, same run")
    say("(median [min, max] of %d after a warm-up; ms)" % args.reps)
    say()
    loses = []
    lib = lp.capi.lib()
    lib.mi355x_sbatch_lps_global_timing(1, None, None, None)

    # ---- (a) create alone
    say("(a) create alone")
    say("   m x n        form  N     | host: build_tableau_single  + from_arrays(global)            total | from_lps(global)"
        "              ratio  upload/  | write pass ms    GB     share of 8 TB/s")
    for (m, n), counts, built_n in (((256, 512), (64, 256, 1024), args.built), ((1024, 2048), (8, 64), 1)):
        for two_phase in (False, True):
            if (m, n) == (1024, 2048) and two_phase:
                continue
            form = "two" if two_phase else "one"
            Ld, sd = rows_of(n, m, built_n, two_phase)
            ps = problems_of(Ld, sd)
            if m <= 256:                                     # (no member would leave the device route)
                assert lp.group_lowered_rows_single(ps * 2)[0] == {}
            per, tabs = [], []
            for p in ps:                                     # Python per coefficient: once per member, no warm-up
                t0 = time.perf_counter()
                t = lp.build_tableau_single(p)
                per.append(time.perf_counter() - t0)
                tabs.append(t if isinstance(t, list) else [t])
            t_build = statistics.median(per)
            stacks = [(np.stack([t[w].matrix for t in tabs]), np.stack([t[w].basis_columns for t in tabs]))
                      for w in range(len(tabs[0]))]
            for N in counts:
                L, sense = repeat(Ld, N), repeat(sd, N)
                host = [(repeat(Ms, N), repeat(bs, N)) for Ms, bs in stacks]
                tu, _ = timed(lambda: close(*[lp.SingleBatch.from_arrays(Ms, bs, form="global") for Ms, bs in host]), args.reps)
                writes = []

                def create_rows():
                    made = lp.SingleBatch.from_lps(L, sense, form="global")
                    writes.append(write_pass_ms()[1])
                    return made
                tr, made = timed(lambda: close(*create_rows()), args.reps)
                main_b, art_b = lp.SingleBatch.from_lps(L, sense, form="global")
                for q in (0, N - 1):                         # the same members, bit for bit
                    for sb, (Ms, bs) in zip((art_b, main_b) if art_b else (main_b,), host):
                        G, gb = sb.download(q)
                        assert np.array_equal(G.view(np.uint32), Ms[q].view(np.uint32)) and np.array_equal(gb, bs[q])
                ld_m, ld_a = main_b.info()["ld"], (art_b.info()["ld"] if art_b else 0)
                close(main_b, art_b)
                nbytes = 4 * N * ((m + 1) * ld_m + m * ld_a + (m + 1) * (n + 1))
                w = statistics.median(writes[1:])
                total = t_build * N + tu[0]
                say("   %-12s %-5s %-5d | %9.1f x %-5d = %9.1f  + %s = %10.1f | %s %8.1f %8.2f  | %9.3f %8.3f %8.1f %%"
                    % ("%d x %d" % (m, n), form, N, t_build * 1e3, N, t_build * N * 1e3, ms(tu), total * 1e3, ms(tr),
                       total / tr[0], tu[0] / tr[0], w, nbytes / 1e9, 100.0 * nbytes / (w * 1e-3) / PEAK))
                if tr[0] >= tu[0]:
                    loses.append("(a) %d x %d %s N=%d against the upload alone" % (m, n, form, N))
                if tr[0] >= total:
                    loses.append("(a) %d x %d %s N=%d" % (m, n, form, N))
    say("   (build_tableau_single: median per member over the members built -- %d at 256 x 512, 1 at 1024 x 2048 -- times N;"
        % args.built)
    say("    ratio: host total over from_lps; upload/: from_arrays alone over from_lps)")
    say()

    # ---- (b) the list route
    say("(b) the list route at 256 x 512, %d members, GLOBAL_BATCH_MIN_MEMBERS as shipped" % args.list_members)
    say("   form | solve_problems_single(beyond_lds)   | from rows (beyond_lds)              ratio | lower alone"
        "                         share of from rows")
    for two_phase in (False, True):
        ps = problems_of(*rows_of(512, 256, args.list_members, two_phase))
        host, groups = lp.group_lowered_rows_single(ps)
        assert host == {} and len(groups) == 1
        forms = []
        real = lp.SingleBatch.from_lps.__func__

        def spy(cls, *a, **kw):
            forms.append(kw.get("form", "lds"))
            return real(cls, *a, **kw)
        lp.SingleBatch.from_lps = classmethod(spy)
        try:
            th, rh = timed(lambda: lp.single.solve_problems_single(ps, errorp=False, beyond_lds=True), args.reps)
            tr, rr = timed(lambda: lp.solve_problems_single_from_rows(ps, errorp=False, beyond_lds=True), args.reps)
        finally:
            lp.SingleBatch.from_lps = classmethod(real)
        assert forms[-2:] == ["lds", "global"], forms
        tl, _ = timed(lambda: lp.group_lowered_rows_single(ps), args.reps)
        assert all(type(a) is type(b) and (isinstance(a, Exception) or
                                           np.array_equal(a.matrix.view(np.uint32), b.matrix.view(np.uint32)))
                   for a, b in zip(rh, rr))
        say("   %-4s | %s | %s %8.2f | %s   %.2f" % ("two" if two_phase else "one", ms(th), ms(tr), th[0] / tr[0], ms(tl),
                                                     tl[0] / tr[0]))
        if tr[0] >= th[0]:
            loses.append("(b) 256 x 512 %s" % ("two" if two_phase else "one"))
    say()

    # ---- (c) a whole search
    p = bb_problem()
    say("(c) a whole search: 200 rows over three integer variables (node tableaux 201 + d x 205 + d), "
        "GLOBAL_BATCH_MIN_MEMBERS as shipped")
    say("   bb_width | beyond_lds=False (node by node)     | beyond_lds=True                     ratio | nodes  in global batches  one by one")
    for width in (8, 64):
        def search(beyond):
            s = lp.single_bb.SingleBranchAndBound(p, width=width, max_pivots=2000, beyond_lds=beyond)
            t = s.run()
            return s, t
        t0, (s0, a) = timed(lambda: search(False), args.reps)
        t1, (s1, b) = timed(lambda: search(True), args.reps)
        assert len(s0.trace()) == len(s1.trace()) and np.array_equal(a.matrix.view(np.uint32), b.matrix.view(np.uint32))
        assert all(x[:5] == y[:5] and (x[5] == y[5] or (x[5] != x[5] and y[5] != y[5])) for x, y in zip(s0.trace(), s1.trace()))
        st = s1.stats()
        say("   %-8d | %s | %s %8.2f | %5d  %17d  %10d" % (width, ms(t0), ms(t1), t0[0] / t1[0], st["solved"],
                                                           st["global_batched"], st["one_by_one"]))
        if t1[0] >= t0[0]:
            loses.append("(c) bb_width %d" % width)
    say()
    say("where the device route loses (not faster than the baseline): %s" % (", ".join(loses) if loses else "nowhere"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
