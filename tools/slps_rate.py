#!/usr/bin/env python
"""What building single-float batches on the device from problem rows (mi355x_sbatch_create_lps) achieves against
the host-built route of the same commit, recorded, not gated.  Every figure is a median of --reps runs after a
warm-up.  Shapes m x n: those of profiles/sbatch_rate.txt, each also in a two-phase form (the last 6 rows
artificial: three written `>=`, three as `<=` rows with both sides negated).  In both forms every fourth of the other
rows is a `>=` row with both sides negated, which the flip turns back into `<=`.

  create    SingleBatch.from_arrays(host-built float32 tableaux, upload included; the tableaux themselves are made
            outside the timed region)  |  SingleBatch.from_lps(rows)
  arrays    from_arrays + solve + readback  |  solve_lps_single(rows): arrays in, light read-back out
  e2e       solve_problems_single(ps)  |  solve_problems_single_from_rows(ps); `lower` is
            group_lowered_rows_single(ps) alone, `share` its part of the from-rows time.  On the first members only,
            as many as hold --e2e-terms coefficients: the Problem objects cost Python per coefficient on both routes.

    python tools/slps_rate.py [--reps 5] [--out profiles/slps_rate.txt]
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
DISTINCT = 64
N_ART = 6          # (a 96 x 300 member with 7 artificial columns is the last one inside the LDS budget)


def rows_of(n, m, count, two_phase):
    """-> (L count x (m + 1) x (n + 1) float32, sense count x m): synth.tableau's numbers as problem rows."""
    Ls, ss = [], []
    for k in range(min(count, DISTINCT)):
        M, _ = lp.synth.tableau(n, m, lp.synth.seed_for(9, 4321 + k))
        M = M.astype(F32)
        L = np.concatenate([M[:, :n], M[:, -1:]], axis=1)
        sense = np.zeros(m, dtype=np.int32)
        L[:m - N_ART:4] *= F32(-1)                            # `>=` with both sides negated: flipped back into `<=`
        sense[:m - N_ART:4] = 1
        if two_phase:
            L[m - N_ART:m, -1] *= F32(0.01)                   # A x >= b / 100: feasible next to the `<=` rows
            sense[m - N_ART:m - N_ART // 2] = 1
            L[m - N_ART // 2:m] *= F32(-1)                    # `<=` with both sides negated: flipped into `>=`
        Ls.append(L)
        ss.append(sense)
    return (np.stack([Ls[k % len(Ls)] for k in range(count)]), np.stack([ss[k % len(ss)] for k in range(count)]))


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


def host_tableaux(ps):
    """The stacked float32 tableaux and bases build_tableau_single makes: [(matrices, bases)], artificial first."""
    tabs = [lp.build_tableau_single(p) for p in ps]
    pairs = [t if isinstance(t, list) else [t] for t in tabs]
    return [(np.stack([p[w].matrix for p in pairs]), np.stack([p[w].basis_columns for p in pairs]))
            for w in range(len(pairs[0]))]


def timed(fn, reps):
    ts, out = [], None
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if k:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def close(*batches):
    for b in batches:
        if b is not None:
            b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e-terms", type=int, default=200000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["single-float batches from problem rows against the host-built route (median of %d after a warm-up)" % args.reps, ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    loses = []
    say("   m x n      form    N      | create ms: host-built   from rows   ratio | arrays ms: host-built   from rows   ratio")
    e2e = []
    for m, n in ((24, 40), (61, 97), (96, 300)):
        for two_phase in (False, True):
            form = "two" if two_phase else "one"
            built = {}
            for N in (256, 1024):
                L, sense = rows_of(n, m, N, two_phase)
                k = min(N, DISTINCT)
                if not built:
                    built["tabs"] = host_tableaux(problems_of(L[:k], sense[:k]))
                stacks = [(np.concatenate([Ms] * (N // k)), np.concatenate([bs] * (N // k))) for Ms, bs in built["tabs"]]

                def create_host():
                    close(*[lp.SingleBatch.from_arrays(Ms, bs) for Ms, bs in stacks])

                def create_rows():
                    close(*lp.SingleBatch.from_lps(L, sense))

                def arrays_host():
                    made = [lp.SingleBatch.from_arrays(Ms, bs) for Ms, bs in stacks]
                    st, _ = made[0].solve_two_phase(made[1], True) if two_phase else made[0].solve(True)
                    out = lp.single_bb.readback(made[-1])
                    close(*made)
                    return st, out

                tch, _ = timed(create_host, args.reps)
                tcr, _ = timed(create_rows, args.reps)
                tah, (st_h, out_h) = timed(arrays_host, args.reps)
                tar, out_r = timed(lambda: lp.solve_lps_single(L, sense), args.reps)
                assert np.array_equal(st_h, out_r[0]) and all(np.array_equal(a.view(np.uint8), b.view(np.uint8))
                                                              for a, b in zip(out_h, out_r[2:]))
                say("   %-10s %-7s %-6d | %21.3f %11.3f %7.2f | %21.3f %11.3f %7.2f"
                    % ("%d x %d" % (m, n), form, N, tch * 1e3, tcr * 1e3, tch / tcr, tah * 1e3, tar * 1e3, tah / tar))
                for leg, a, b in (("create", tch, tcr), ("arrays", tah, tar)):
                    if b >= a:
                        loses.append("%s %d x %d %s N=%d" % (leg, m, n, form, N))
                ke = min(N, max(2, args.e2e_terms // (m * n)))
                if (m, n, two_phase, ke) not in [x[:4] for x in e2e]:
                    ps = problems_of(*rows_of(n, m, ke, two_phase))
                    host, groups = lp.group_lowered_rows_single(ps)
                    assert host == {} and len(groups) == 1
                    teh, rh = timed(lambda: lp.single.solve_problems_single(ps, errorp=False), args.reps)
                    ter, rr = timed(lambda: lp.solve_problems_single_from_rows(ps, errorp=False), args.reps)
                    tlo, _ = timed(lambda: lp.group_lowered_rows_single(ps), args.reps)
                    assert all(type(a) is type(b) and (isinstance(a, Exception) or
                                                       np.array_equal(a.matrix.view(np.uint32), b.matrix.view(np.uint32)))
                               for a, b in zip(rh, rr))
                    e2e.append((m, n, two_phase, ke, teh, ter, tlo))
                    if ter >= teh:
                        loses.append("e2e %d x %d %s N=%d" % (m, n, form, ke))
    say("")
    say("   m x n      form    members | e2e ms: solve_problems_single   from rows   ratio | lower ms   share of from rows")
    for m, n, two_phase, ke, teh, ter, tlo in e2e:
        say("   %-10s %-7s %-7d | %29.1f %11.1f %7.2f | %8.1f   %.2f"
            % ("%d x %d" % (m, n), "two" if two_phase else "one", ke, teh * 1e3, ter * 1e3, teh / ter, tlo * 1e3, tlo / ter))
    say("")
    say("where the device route loses (not faster than the host-built one): %s" % (", ".join(loses) if loses else "nowhere"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
