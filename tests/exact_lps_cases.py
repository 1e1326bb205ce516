"""Shared by the tests of the device-built exact batches (mi355x_xbatch_create_lps): the Python-int statement
of what k_xb_assemble_lps writes (linear-programming_amd/csrc/kernels_exact_lps.inc) -- pinned to
exact_cases.start_state(build_tableau(exact=True)) by tests/test_exact_lps_host.py, as exact_bb.node_tableaux
states k_xbb_assemble -- and generators of members given as arrays."""
import random
from fractions import Fraction
from math import gcd

import numpy as np

from tests import exact_cases as ec


def assemble(num, den, sense):
    """A member in column space (num, den: (m + 1) x (ncv + 1), sense: m) -> (D main, main rows, main basis,
    D art, art rows, art basis), every entry a Python int; the last three None without an artificial row.
    The integer rule of the kernel: L_i the rows' LCMs, P = prod_{i<m} L_i, D main = P * L_m; S_c the column sums
    of the artificial rows at scale P, D art = P * (P / gcd(P, S_0, S_1, ...))."""
    num = [[int(x) for x in row] for row in num]
    den = [[int(x) for x in row] for row in den]
    m, ncv = len(num) - 1, len(num[0]) - 1
    L = []
    for row in den:
        l = 1
        for d in row:
            l = l // gcd(l, d) * d
        L.append(l)
    flip = [num[r][ncv] < 0 for r in range(m)]
    op = [2 if int(s) == 2 else (1 - int(s) if f else int(s)) for s, f in zip(sense, flip)]
    n_slack = sum(o != 2 for o in op)
    num_cols = ncv + n_slack + 1
    P = 1
    for l in L[:m]:
        P *= l
    Dm = P * L[m]

    def entry(D, r, c):
        x = D // den[r][c] * num[r][c]
        return -x if r < m and flip[r] else x

    def rows_at(D, extra):
        out, k = [], 0
        for r in range(m):
            slack = [0] * n_slack
            if op[r] != 2:
                slack[k] = D if op[r] == 0 else -D
                k += 1
            out.append([entry(D, r, c) for c in range(ncv)] + slack + [0] * extra + [entry(D, r, ncv)])
        return out
    M = rows_at(Dm, 0)
    M.append([entry(Dm, m, c) for c in range(ncv)] + [0] * n_slack + [entry(Dm, m, ncv)])
    basis, k = [], 0
    for r in range(m):
        basis.append(ncv + k if op[r] == 0 else num_cols)
        k += op[r] != 2
    art_rows = [r for r in range(m) if op[r] != 0]
    if not art_rows:
        return Dm, M, basis, None, None, None
    n_art = len(art_rows)
    S = [sum(entry(P, r, c) for r in art_rows) for c in range(ncv + 1)]
    g = P
    for s in S:
        g = gcd(g, s)
    La = P // g
    Da = P * La
    A = rows_at(Da, n_art)
    abasis = list(basis)
    for k, r in enumerate(reversed(art_rows)):                            # push order, :257, :261, :296-300
        A[r][num_cols - 1 + k] = Da
        abasis[r] = num_cols - 1 + k
    last = [0] * (num_cols + n_art)
    for c in list(range(num_cols - 1)) + [num_cols + n_art - 1]:
        last[c] = sum(A[r][c] for r in art_rows)
    assert last[:ncv] + last[-1:] == [s * La for s in S]
    A.append(last)
    return Dm, M, basis, Da, A, abasis


def host_states(lp, problem):
    """((T0, D0, basis) main, the same of the artificial tableau or None) from build_tableau(exact=True) and
    exact_cases.start_state."""
    tabs = lp.build_tableau(problem, exact=True)
    art, main = tabs if isinstance(tabs, list) else (None, tabs)
    out = []
    for t in (main, art):
        if t is None:
            out.append(None)
            continue
        T, D = ec.start_state(t._matrix.tolist())
        out.append((T, D, t._basis.tolist()))
    return tuple(out)


def reduction_problem(lp):
    """x/2 + y/3 >= 1 and x/2 + 2y/3 >= 1 under max -x - y: P = 36, the column sums at that scale are 36, 36 and
    72, so the artificial objective row is integral and the artificial tableau starts from D = 36, not 36 * 6."""
    F = Fraction
    return lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", -1), ("y", -1)],
                      constraints=[(">=", [("x", F(1, 2)), ("y", F(1, 3))], 1),
                                   (">=", [("x", F(1, 2)), ("y", F(2, 3))], 1)])


def dense_slack_problem(lp, n, seed):
    """An n x n all-`<=` max LP with small non-negative integers: no artificial row."""
    T, _ = ec.slack_tableau(n, n, seed)
    names = ["x%d" % i for i in range(n)]
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, int(-T[n, j])) for j, v in enumerate(names)],
                      constraints=[("<=", [(v, int(T[i, j])) for j, v in enumerate(names)], int(T[i, -1])) for i in range(n)])


def array_members(n, m, ncv, seed, pattern, dens=(1,), frac_rows=None, lo=-4, hi=6):
    """n members in column space whose rows all follow `pattern(i) -> (sense, right-hand side negative?)`, so
    that they form one group: coefficients in [lo, hi] over denominators from `dens` (rows in frac_rows only;
    None: every row), reduced.  (num, den, sense) as create_lps takes them."""
    rng = random.Random(seed)
    num = np.zeros((n, m + 1, ncv + 1), dtype=np.int64)
    den = np.ones((n, m + 1, ncv + 1), dtype=np.int64)
    sense = np.zeros((n, m), dtype=np.int32)
    for q in range(n):
        for i in range(m + 1):
            fr = frac_rows is None or i in frac_rows
            for c in range(ncv + 1):
                x = Fraction(rng.randint(lo, hi), rng.choice(dens) if fr else 1)
                if i < m and c == ncv:
                    s, neg = pattern(i)
                    sense[q, i] = s
                    x = -abs(x) - 1 if neg else abs(x)
                num[q, i, c], den[q, i, c] = x.numerator, x.denominator
    return num, den, sense


def feasible_members(n, ncv, seed, pattern, dens=(1, 2, 3)):
    """array_members whose members have an optimum as min problems: x = 1 satisfies every row (a negative
    right-hand side comes from negative coefficients), and the objective row -c has c >= 0 over x >= 0."""
    rng = random.Random(seed)
    m = 0
    while True:
        try:
            pattern(m)
        except IndexError:
            break
        m += 1
    num = np.zeros((n, m + 1, ncv + 1), dtype=np.int64)
    den = np.ones((n, m + 1, ncv + 1), dtype=np.int64)
    sense = np.zeros((n, m), dtype=np.int32)
    for q in range(n):
        for i in range(m + 1):
            s, neg = pattern(i) if i < m else (0, True)                   # (the objective row: -c)
            row = [Fraction(rng.randint(-5, -1) if neg else rng.randint(0, 5), rng.choice(dens)) for _ in range(ncv)]
            if i < m:
                sense[q, i] = s
                row.append(sum(row) + (1 if s == 0 else -1 if s == 1 else 0))
                if s == 1 and not neg:
                    row[-1] = max(row[-1], Fraction(0))
            else:
                row.append(Fraction(0))
            for c, x in enumerate(row):
                num[q, i, c], den[q, i, c] = x.numerator, x.denominator
    return num, den, sense


def problem_of_arrays(lp, num, den, sense, is_max=True):
    """The lp.Problem (variables >= 0, no bounds) a member in column space states."""
    m, ncv = num.shape[0] - 1, num.shape[1] - 1
    names = ["x%d" % j for j in range(ncv)]
    F = lambda r, c: Fraction(int(num[r, c]), int(den[r, c]))
    cons = [(("<=", ">=", "=")[int(sense[r])], [(v, F(r, j)) for j, v in enumerate(names)], F(r, ncv)) for r in range(m)]
    assert num[m, ncv] == 0
    return lp.Problem(type="max" if is_max else "min", vars=names, objective_var="w",
                      objective_func=[(v, -F(m, j)) for j, v in enumerate(names)], constraints=cons)
