"""Shared by the tests of the device-built double-precision batches (mi355x_multibatch_create_lps): a seeded
generator of small problems, the plain numpy statement of what k_blp_rows / k_assemble / k_art_objective
write (linear-programming_amd/csrc/kernels_batch_lps.inc) -- pinned to build_tableau by
tests/test_batch_lps_host.py -- and members given as arrays that have a known outcome."""
import random

import numpy as np

OPS = ("<=", ">=", "=")
KINDS = ("plain", "lower", "upper+", "upper-", "both+", "both-", "free")
# coefficients: small integers, a zero, and decimals whose sums round (0.1 + 0.2 != 0.3)
COEFS = (-3, -2, -1, 0, 1, 2, 3, 0.1, 0.2, 0.7, -0.3, 1.5)


def _bounds(kind, rng):
    if kind == "plain":
        return None
    if kind == "lower":
        return (rng.choice((1, 2.5, -1.5, 0.1)), None)
    if kind == "upper+":
        return (None, rng.choice((0, 2, 3.5)))
    if kind == "upper-":
        return (None, rng.choice((-1, -2.5)))
    if kind == "both+":
        return (rng.choice((-1, 0.5, 1, 0.1)), rng.choice((2, 4.5)))
    if kind == "both-":
        return (rng.choice((-6, -4.5)), rng.choice((-1, -2.5)))
    return (None, None)


def problem(lp, seed):
    """A small problem and the kinds of its variables.  Over the seeds: `<=`, `>=` and `=` rows; negative
    right-hand sides and ones that become negative only through an offset; zero coefficients (also in negated
    rows); free, upper-bounded-only and doubly bounded variables with ub >= 0 and ub < 0; non-zero lower bounds; a
    non-zero objective constant (an objective coefficient on a variable with an offset)."""
    rng = random.Random(seed)
    n = rng.randint(2, 4)
    names = ["x%d" % i for i in range(n)]
    tame = rng.random() < 0.4                            # mostly single-phase: `<=` rows, right-hand sides >= 3
    kinds = [rng.choice(("plain", "plain", "both+", "free") if tame else KINDS) for _ in names]
    var_bounds = [(v, _bounds(k, rng)) for v, k in zip(names, kinds) if k != "plain"]
    cons = []
    for _ in range(rng.randint(1, 4)):
        expr = [(v, rng.choice(COEFS)) for v in names if rng.random() < 0.8] or [(names[0], 1)]
        # a small right-hand side next to offsets of either sign: some stay positive, some are negative from the
        # start, some become negative only when coef * offset is subtracted
        if tame:
            cons.append(("<=", expr, rng.choice((3, 7.5, 12))))
        else:
            cons.append((rng.choice(OPS), expr, rng.choice((-2, -0.5, 0, 0.25, 1, 3, 7.5))))
    obj = [(v, rng.choice((-2, -1, 0.5, 1, 3))) for v in names]
    p = lp.Problem(type=rng.choice(("max", "min")), vars=names, objective_var="w", objective_func=obj,
                   var_bounds=var_bounds, constraints=cons)
    return p, set(kinds)


def assemble(L, sense):
    """A member in column space (L: (m + 1) x (ncv + 1) float64, sense: m) -> (main matrix, main basis, artificial
    matrix, artificial basis), the last two None without an artificial row: the kernels' statement, entry by
    entry."""
    L = np.asarray(L, dtype=np.float64)
    m, ncv = L.shape[0] - 1, L.shape[1] - 1
    flip = [bool(L[i, ncv] < 0.0) for i in range(m)]
    op = [2 if int(s) == 2 else (1 - int(s) if f else int(s)) for s, f in zip(sense, flip)]
    n_slack = sum(o != 2 for o in op)
    cols = ncv + n_slack + 1
    M = np.zeros((m + 1, cols))
    basis = np.zeros(m, dtype=np.int64)
    k = 0
    for i in range(m):
        row = -L[i] if flip[i] else L[i]
        M[i, :ncv], M[i, cols - 1] = row[:ncv], row[ncv]
        M[i, ncv:cols - 1] = -0.0 if flip[i] else 0.0
        if op[i] != 2:
            M[i, ncv + k] = 1.0 if op[i] == 0 else -1.0
        basis[i] = ncv + k if op[i] == 0 else cols
        k += op[i] != 2
    M[m, :ncv], M[m, cols - 1] = L[m, :ncv], L[m, ncv]
    art_rows = [i for i in range(m) if op[i] != 0]
    if not art_rows:
        return M, basis, None, None
    n_art = len(art_rows)
    A = np.zeros((m + 1, cols + n_art))
    abasis = basis.copy()
    A[:m, :cols - 1], A[:m, -1] = M[:m, :cols - 1], M[:m, cols - 1]
    for i in art_rows:
        rank = sum(1 for j in art_rows if j > i)
        A[i, cols - 1 + rank] = 1.0
        abasis[i] = cols - 1 + rank
    for c in list(range(cols - 1)) + [cols + n_art - 1]:
        s = np.float64(0.0)
        for i in art_rows:                                                # increasing row order, one rounding each
            s = s + A[i, c]
        A[m, c] = s
    return M, basis, A, abasis


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_tableaux(lp, p):
    """(main matrix, main basis, artificial matrix, artificial basis, mapping) from build_tableau."""
    tabs = lp.build_tableau(p)
    art, main = tabs if isinstance(tabs, list) else (None, tabs)
    return (main._matrix, main._basis, art._matrix if art else None, art._basis if art else None, main.var_mapping)


def random_rows(n, m, ncv, seed, pattern):
    """n members in column space whose rows follow pattern(i) -> (sense, right-hand side negative?), so that they
    form one group; coefficients from COEFS (zeros included), inexact sums in the artificial objective row."""
    rng = random.Random(seed)
    L = np.zeros((n, m + 1, ncv + 1))
    sense = np.zeros((n, m), dtype=np.int32)
    for q in range(n):
        for i in range(m + 1):
            L[q, i] = [rng.choice(COEFS) + rng.choice((0, 0.1, 0.01)) for _ in range(ncv + 1)]
            if i < m:
                sense[q, i], neg = pattern(i)
                L[q, i, ncv] = -abs(L[q, i, ncv]) - 0.5 if neg else abs(L[q, i, ncv])
    return L, sense


def single_phase_members(n, m, ncv, seed):
    """All-`<=` members of  max c . x,  A x <= b  with A > 0, b > 0, c > 0 (bounded, an optimum) -- but member 1 (n > 1),
    whose column 0 is <= 0 in every row: unbounded."""
    rng = np.random.default_rng(seed)
    L = np.zeros((n, m + 1, ncv + 1))
    L[:, :m, :ncv] = rng.uniform(0.1, 1.0, (n, m, ncv))
    L[:, :m, ncv] = rng.uniform(1.0, 2.0, (n, m))
    L[:, m, :ncv] = -rng.uniform(0.5, 1.5, (n, ncv))
    if n > 1:
        L[1, :m, 0] = -L[1, :m, 0]
    return L, np.zeros((n, m), dtype=np.int32)


def two_phase_members(n, ncv, seed):
    """Members of  min c . x  (c > 0: bounded) with the rows `<=`, `>=`, `=`, `>=` written with a negative right-hand
    side (so negated into `<=`), and `<=` written with a negative right-hand side (negated into `>=`): x = 1 is
    feasible.  Member 1 is infeasible (row 0 says sum x <= 1, row 1 sum x >= 3); member 2 is unbounded (its
    column 0 has cost -1 and no row holds it back).  is_max False."""
    rng = np.random.default_rng(seed)
    m = 5
    L = np.zeros((n, m + 1, ncv + 1))
    a = rng.uniform(0.1, 1.0, (n, m, ncv))
    a[2, :, 0] = 0.0
    s = a.sum(axis=2)
    L[:, 0, :ncv], L[:, 0, ncv] = a[:, 0], s[:, 0] + 1.0                  # a.x <= a.1 + 1
    L[:, 1, :ncv], L[:, 1, ncv] = a[:, 1], s[:, 1] - 0.05                 # a.x >= a.1 - 0.05  (> 0)
    L[:, 2, :ncv], L[:, 2, ncv] = a[:, 2], s[:, 2]                        # a.x  = a.1
    L[:, 3, :ncv], L[:, 3, ncv] = -a[:, 3], -s[:, 3] - 1.0                # -a.x >= -a.1 - 1   (negated: `<=`)
    L[:, 4, :ncv], L[:, 4, ncv] = -a[:, 4], -s[:, 4] + 0.05               # -a.x <= -a.1 + 0.05 (negated: `>=`)
    L[:, m, :ncv] = -rng.uniform(0.5, 1.5, (n, ncv))                      # the objective row: -c
    sense = np.tile(np.array([0, 1, 2, 1, 0], dtype=np.int32), (n, 1))
    L[1, 0, :ncv], L[1, 0, ncv] = 1.0, 1.0
    L[1, 1, :ncv], L[1, 1, ncv] = 1.0, 3.0
    L[2, 0, 0] = -1.0
    L[2, m, 0] = 1.0
    return L, sense


def problem_of_rows(lp, L, sense, is_max):
    """The lp.Problem (variables >= 0, no bounds, no constant) a member in column space states."""
    m, ncv = L.shape[0] - 1, L.shape[1] - 1
    names = ["x%d" % j for j in range(ncv)]
    cons = [(OPS[int(sense[i])], [(v, float(L[i, j])) for j, v in enumerate(names)], float(L[i, ncv])) for i in range(m)]
    assert L[m, ncv] == 0
    return lp.Problem(type="max" if is_max else "min", vars=names, objective_var="w",
                      objective_func=[(v, float(-L[m, j])) for j, v in enumerate(names)], constraints=cons)
