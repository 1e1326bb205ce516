"""Shared by the exact-mode tests: a seeded generator of random rational LPs, the problem in the
oracle's dict form, the oracle's outcome, and a pure-Python model of the fraction-free (Bareiss)
arithmetic the exact kernels implement (linear-programming_amd/csrc/kernels_exact.inc)."""
import random
from fractions import Fraction
from math import gcd

import oracle.rational_ref as rr


def _coef(rng):
    if rng.random() < 0.5:
        return rng.randint(-6, 6)
    return Fraction(rng.randint(-12, 12), rng.randint(1, 10))


def random_problem(lp, seed):
    """A random LP with integer and p/q coefficients, all three senses, bounds, free variables,
    negative right-hand sides and (often) a redundant equality row, which leaves an artificial
    variable basic at the end of phase 1 (a drive-out)."""
    rng = random.Random(seed)
    big = seed % 20 == 0
    n = rng.randint(8, 20) if big else rng.randint(2, 6)
    m = rng.randint(4, 20) if big else rng.randint(1, 6)
    names = ["x%d" % i for i in range(n)]
    cons = []
    for _ in range(m):
        op = rng.choice(["<=", "<=", ">=", "="])
        expr = [(v, _coef(rng)) for v in names if rng.random() < 0.7] or [(names[0], 1)]
        rhs = _coef(rng) if rng.random() < 0.3 else abs(Fraction(_coef(rng))) + rng.randint(0, 8)
        cons.append((op, expr, rhs))
    if rng.random() < 0.35:                       # a redundant equality: k times an existing row
        base = cons[rng.randrange(len(cons))]
        k = Fraction(rng.choice([1, 2, 3, -1, -2]), rng.choice([1, 1, 2, 3]))
        if base[0] == "=":
            cons.append(("=", [(v, c * k) for v, c in base[1]], base[2] * k))
        else:
            cons.append(("=", list(base[1]), base[2]))
            cons.append(("=", [(v, c * k) for v, c in base[1]], base[2] * k))
    bounds = []
    for v in names:
        r = rng.random()
        if r < 0.1:
            bounds.append((v, (None, None)))                                  # free
        elif r < 0.2:
            lo = rng.randint(-3, 2)
            bounds.append((v, (lo, lo + abs(Fraction(_coef(rng))) + 1)))
        elif r < 0.27:
            bounds.append((v, (None, rng.randint(-2, 5))))
        elif r < 0.34:
            bounds.append((v, (Fraction(rng.randint(-4, 4), rng.randint(1, 3)), None)))
    obj = [(v, _coef(rng)) for v in names]
    return lp.Problem(type=rng.choice(["max", "min"]), vars=names, objective_var="w",
                      objective_func=obj, var_bounds=bounds, constraints=cons)


def divergent_problem(lp, seed):
    """An all-<= max LP with coefficients k/3, k/7 or k/10 (ties that rounding can break)."""
    rng = random.Random(seed)
    n, m = rng.randint(3, 7), rng.randint(3, 7)
    q = rng.choice([3, 7, 10])
    names = ["x%d" % i for i in range(n)]
    cons = [("<=", [(v, Fraction(rng.randint(0, 9), q)) for v in names], Fraction(rng.randint(1, 20), q))
            for _ in range(m)]
    obj = [(v, Fraction(rng.randint(0, 9), q)) for v in names]
    return lp.Problem(type="max", vars=names, objective_var="w", objective_func=obj, constraints=cons)


def to_dict(p):
    """lp.Problem -> the oracle's problem dict."""
    return {"type": p.type, "vars": list(p.vars), "objective_var": p.objective_var,
            "objective": [[v, c] for v, c in p.objective_func],
            "bounds": [[v, lb, ub] for v, (lb, ub) in p.var_bounds],
            "constraints": [[op, [[v, c] for v, c in e], rhs] for op, e, rhs in p.constraints]}


def oracle_outcome(tabs):
    """(status, trace, final main tableau or None) of the Fraction oracle on build_tableau's result."""
    trace = []
    try:
        t = rr.solve_any(tabs, trace)
        return "optimal", trace, t
    except rr.Unbounded:
        return "unbounded", trace, None
    except rr.Infeasible:
        return "infeasible", trace, None
    except RuntimeError as e:
        return ("art_nonzero" if "non-zero" in str(e) else "art_stuck"), trace, None


# ---- the fraction-free model ------------------------------------------------------------------
def _lcm(a, b):
    return a // gcd(a, b) * b


def start_state(matrix):
    """(T0, D0): L_i = LCM of row i's denominators, the objective row's folded into the first
    constraint row's, D0 = prod L_i, T0 = D0 * t0."""
    R = len(matrix)
    L = [1] * R
    for i, row in enumerate(matrix):
        for x in row:
            L[i] = _lcm(L[i], Fraction(x).denominator)
    m = R - 1
    if m > 0:
        L[0] *= L[m]
        D = 1
        for i in range(m):
            D *= L[i]
    else:
        D = L[0]
    T = [[int(Fraction(x) * D) for x in row] for row in matrix]
    assert all(Fraction(x) * D == T[i][j] for i, row in enumerate(matrix) for j, x in enumerate(row))
    return T, D


class Model:
    """The Bareiss state (T, D) of one tableau and the kernels' steps on it."""

    def __init__(self, matrix, basis, var_count):
        self.T, self.D = start_state(matrix)
        self.basis = list(basis)
        self.nv = var_count
        self.stats = {"inexact": 0, "negative_pivots": 0, "driveouts": 0, "max_bits": 0}
        self.track(self.T, [self.D])

    def track(self, rows, extra=()):
        """max_bits: the width (sign bit included) the largest value stored so far needs."""
        vals = [abs(int(x)) for row in rows for x in row] + [abs(int(x)) for x in extra]
        self.stats["max_bits"] = max([self.stats["max_bits"]] + [v.bit_length() + 1 for v in vals])

    def _div(self, N):
        q, r = divmod(N, self.D)
        if r:
            self.stats["inexact"] += 1
        return q

    def pivot(self, e, r):
        p = self.T[r][e]
        s = -1 if p < 0 else 1
        if p < 0:
            self.stats["negative_pivots"] += 1
        prow = self.T[r]
        out = []
        for i, row in enumerate(self.T):
            if i == r:
                out.append([s * x for x in prow])
            else:
                c = s * row[e]
                out.append([self._div(x * abs(p) - c * y) for x, y in zip(row, prow)])
        self.T, self.D = out, abs(p)
        self.basis[r] = e
        self.track(out, [self.D])

    def matrix(self):
        return [[Fraction(x, self.D) for x in row] for row in self.T]

    def price(self, is_max):
        obj = self.T[-1]
        if self.nv == 0:
            return None
        best = 0
        for j in range(1, self.nv):
            if (obj[j] < obj[best]) if is_max else (obj[j] > obj[best]):
                best = j
        return best if ((obj[best] < 0) if is_max else (obj[best] > 0)) else None

    def ratio(self, e):
        best = None
        for i in range(len(self.T) - 1):
            a = self.T[i][e]
            if a > 0 and (best is None or self.T[i][self.nv] * self.T[best][e] < self.T[best][self.nv] * a):
                best = i
        return best

    def solve(self, is_max, trace):
        while True:
            e = self.price(is_max)
            if e is None:
                return "optimal"
            r = self.ratio(e)
            if r is None:
                return "unbounded"
            trace.append((e, r))
            self.pivot(e, r)


def model_solve(tabs):
    """(status, trace, final Model or None, stats) of the fraction-free model on rational_ref's
    build_tableau result (a Tableau or an (art, main) pair)."""
    trace = []
    if not isinstance(tabs, tuple):
        t = Model(tabs.matrix, tabs.basis, tabs.var_count)
        st = t.solve(tabs.is_max, trace)
        return st, trace, (t if st == "optimal" else None), t.stats
    art_t, main_t = tabs
    a = Model(art_t.matrix, art_t.basis, art_t.var_count)
    st = a.solve(False, trace)
    if st != "optimal":
        return st, trace, None, a.stats
    if a.T[-1][a.nv] != 0:
        return "infeasible", trace, None, a.stats
    nv, m = main_t.var_count, main_t.constraint_count
    for i in range(m):
        if a.basis[i] >= nv:
            if a.T[i][a.nv] != 0:
                return "art_nonzero", trace, None, a.stats
            j = next((j for j in range(nv) if a.T[i][j] != 0 and j not in a.basis), None)
            if j is None:
                return "art_stuck", trace, None, a.stats
            a.stats["driveouts"] += 1
            a.pivot(j, i)
    # hand-over: the constraint rows and D times L_c, the objective row D * c - sum c[b_i] T_i
    c = [Fraction(x) for x in main_t.matrix[m]]
    lc = 1
    for x in c:
        lc = _lcm(lc, x.denominator)
    src = list(range(nv)) + [a.nv]
    mm = Model.__new__(Model)
    mm.nv, mm.basis, mm.stats = nv, list(a.basis), a.stats
    mm.D = a.D * lc
    mm.T = [[a.T[i][s] * lc for s in src] for i in range(m)]
    obj = []
    for k, s in enumerate(src):
        v = a.D * (c[k] * lc) - sum(c[a.basis[i]] * lc * a.T[i][s] for i in range(m))
        assert v.denominator == 1
        obj.append(int(v))
    mm.T.append(obj)
    mm.track(mm.T, [mm.D, lc] + [c[a.basis[i]] * lc for i in range(m)] + [x * lc for x in c])
    st = mm.solve(main_t.is_max, trace)
    return st, trace, (mm if st == "optimal" else None), mm.stats


def wide_problem(lp, seed, e):
    """A 4x4 all-<= max LP with coefficients between 2^e and 2^(e+1): its fraction-free entries
    outgrow 64 bits (e = 40) or 128 bits (e = 60) within two pivots."""
    rng = random.Random(seed)
    names = ["x%d" % i for i in range(4)]
    cons = [("<=", [(v, rng.randint(1 << e, 1 << (e + 1))) for v in names], rng.randint(1 << e, 1 << (e + 1)))
            for _ in range(4)]
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, rng.randint(1, 1 << e)) for v in names], constraints=cons)


def beale(lp):
    """Beale's LP with Fraction coefficients: the rational simplex cycles on it with period 6."""
    F = Fraction
    names = ["x1", "x2", "x3", "x4"]
    return lp.Problem(type="max", vars=names, objective_var="z",
                      objective_func=[("x1", F(3, 4)), ("x2", F(-20)), ("x3", F(1, 2)), ("x4", F(-6))],
                      constraints=[("<=", [("x1", F(1, 4)), ("x2", F(-8)), ("x3", F(-1)), ("x4", F(9))], F(0)),
                                   ("<=", [("x1", F(1, 2)), ("x2", F(-12)), ("x3", F(-1, 2)), ("x4", F(3))], F(0)),
                                   ("<=", [("x3", F(1))], F(1))])
