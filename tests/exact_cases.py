"""Shared by the exact-mode tests: a seeded generator of random rational LPs, the problem in the
oracle's dict form, the oracle's outcome, and a pure-Python model of the fraction-free (Bareiss)
arithmetic the exact kernels implement (linear-programming_amd/csrc/kernels_exact.inc)."""
import random
from fractions import Fraction
from math import gcd

import numpy as np

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


def new_stats():
    return {"inexact": 0, "negative_pivots": 0, "driveouts": 0, "max_bits": 0, "pivots": 0, "over64": None}


def note_bits(stats, stage, bits):
    """max_bits, and where it first exceeded 64: over64 = (stage, index of the pivot whose result did it,
    counted over both phases and the drive-outs; for the hand-over: the pivots applied before it)."""
    stats["max_bits"] = max(stats["max_bits"], bits)
    if stats["max_bits"] > 64 and stats["over64"] is None:
        stats["over64"] = (stage, stats["pivots"])


class Model:
    """The Bareiss state (T, D) of one tableau and the kernels' steps on it."""

    stage = "phase1"

    def __init__(self, matrix, basis, var_count):
        self.T, self.D = start_state(matrix)
        self.basis = list(basis)
        self.nv = var_count
        self.stats = new_stats()
        self.track(self.T, [self.D])

    @classmethod
    def from_state(cls, T, D, basis, var_count, stats=None, stage="phase1", extra=()):
        """A model that starts from integer rows T and their common denominator D."""
        t = cls.__new__(cls)
        t.T, t.D, t.basis, t.nv = [list(row) for row in T], D, list(basis), var_count
        t.stats, t.stage = (new_stats() if stats is None else stats), stage
        t.track(t.T, [t.D] + list(extra))
        return t

    def rows(self):
        """T as lists of Python ints."""
        return self.T

    def track(self, rows, extra=()):
        """max_bits: the width (sign bit included) the largest value stored so far needs."""
        vals = [abs(int(x)) for row in rows for x in row] + [abs(int(x)) for x in extra]
        note_bits(self.stats, self.stage, max([0] + [v.bit_length() + 1 for v in vals]))

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
        self.stats["pivots"] += 1

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

    def solve(self, is_max, trace, max_pivots=0):
        """Pivots until the tableau is optimal or unbounded, or ("max_pivots") max_pivots > 0 were made."""
        k = 0
        while True:
            if max_pivots and k >= max_pivots:
                return "max_pivots"
            k += 1
            e = self.price(is_max)
            if e is None:
                return "optimal"
            r = self.ratio(e)
            if r is None:
                return "unbounded"
            trace.append((e, r))
            self.pivot(e, r)


def model_solve(tabs, cls=None, keep=None, phase2_pivots=0, total_pivots=0):
    """(status, trace, final model or None, stats) of the fraction-free model (cls: Model or VecModel) on
    rational_ref's build_tableau result (a Tableau or an (art, main) pair).  keep: a dict that receives
    the artificial model ("art") and the trace's length at the end of phase 1 ("n1").  phase2_pivots > 0
    caps phase 2 of a two-phase solve: status "max_pivots", the main model as it stands; total_pivots > 0
    caps it at what a call of that many pivots leaves for it after phase 1 and the drive-outs (which must
    fit the call).  keep also receives "driveout_pivots": per drive-out (column, row, every eligible column
    -- non-zero and non-basic -- of the row at that moment)."""
    cls = cls or Model
    trace = []
    if not isinstance(tabs, tuple):
        t = cls(tabs.matrix, tabs.basis, tabs.var_count)
        st = t.solve(tabs.is_max, trace)
        return st, trace, (t if st == "optimal" else None), t.stats
    art_t, main_t = tabs
    a = cls(art_t.matrix, art_t.basis, art_t.var_count)
    st = a.solve(False, trace)
    if keep is not None:
        keep["art"], keep["n1"] = a, len(trace)
    if st != "optimal":
        return st, trace, None, a.stats
    if a.rows()[-1][a.nv] != 0:
        return "infeasible", trace, None, a.stats
    nv, m = main_t.var_count, main_t.constraint_count
    a.stage = "driveout"
    for i in range(m):
        if a.basis[i] >= nv:
            row = a.rows()[i]
            if row[a.nv] != 0:
                return "art_nonzero", trace, None, a.stats
            eligible = [j for j in range(nv) if row[j] != 0 and j not in a.basis]
            if not eligible:
                return "art_stuck", trace, None, a.stats
            j = eligible[0]
            if keep is not None:
                keep.setdefault("driveout_pivots", []).append((j, i, eligible))
            a.stats["driveouts"] += 1
            a.pivot(j, i)
    # hand-over: the constraint rows and D times L_c, the objective row D * c - sum c[b_i] T_i
    c = [Fraction(x) for x in main_t.matrix[m]]
    lc = 1
    for x in c:
        lc = _lcm(lc, x.denominator)
    src = list(range(nv)) + [a.nv]
    AT = a.rows()
    T = [[AT[i][s] * lc for s in src] for i in range(m)]
    w = [c[a.basis[i]] * lc for i in range(m)]
    cl = [x * lc for x in c]
    assert all(x.denominator == 1 for x in w + cl)
    w, cl = [int(x) for x in w], [int(x) for x in cl]
    T.append([a.D * cl[k] - sum(w[i] * AT[i][s] for i in range(m) if w[i]) for k, s in enumerate(src)])
    mm = cls.from_state(T, a.D * lc, a.basis, nv, stats=a.stats, stage="handover", extra=[lc] + w + cl)
    mm.stage = "phase2"
    if total_pivots:
        phase2_pivots = total_pivots - len(trace) - a.stats["driveouts"]
        assert phase2_pivots > 0
    st = mm.solve(main_t.is_max, trace, phase2_pivots)
    return st, trace, (mm if st in ("optimal", "max_pivots") else None), mm.stats


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


# ---- the same model on a numpy matrix, for tableaux of many workgroups ----------------------------
class VecModel:
    """Model's rules (price / ratio / pivot, the same ties) with the rank-1 update done by numpy: int64
    while every intermediate of a pivot provably stays below 2^62, Python ints (dtype object) beyond.
    tests/test_exact_host.py pins it to Model, and so to oracle/rational_ref.py."""
    stage = "phase1"

    def __init__(self, matrix, basis, var_count):
        T, D = start_state(matrix)
        self._init(T, D, basis, var_count, None, "phase1", ())

    @classmethod
    def from_state(cls, T, D, basis, var_count, stats=None, stage="phase1", extra=()):
        t = cls.__new__(cls)
        t._init(T, D, basis, var_count, stats, stage, extra)
        return t

    def _init(self, T, D, basis, var_count, stats, stage, extra):
        if isinstance(T, np.ndarray) and T.dtype == np.int64:
            self.T = T.copy()
        else:
            self.T = np.array(T, dtype=object)
            if self._maxabs() < 1 << 62:
                self.T = self.T.astype(np.int64)
        self.D, self.basis, self.nv = int(D), [int(b) for b in basis], int(var_count)
        self.stats, self.stage = (new_stats() if stats is None else stats), stage
        self.track(extra)

    def _maxabs(self):
        if self.T.dtype == object:
            return max(abs(x) for x in self.T.flat)
        return max(int(self.T.max()), -int(self.T.min()))

    def track(self, extra=()):
        vals = [self._maxabs(), self.D] + [abs(int(x)) for x in extra]
        note_bits(self.stats, self.stage, max(v.bit_length() + 1 for v in vals))

    def rows(self):
        return self.T.tolist()

    def price(self, is_max):
        if self.nv == 0:
            return None
        obj = self.T[-1, :self.nv]
        best = int(np.argmin(obj) if is_max else np.argmax(obj))         # (the first of equal values)
        return best if ((obj[best] < 0) if is_max else (obj[best] > 0)) else None

    def ratio(self, e):
        col, rhs = self.T[:-1, e], self.T[:-1, self.nv]
        best = ba = br = None
        for i in np.nonzero(col > 0)[0].tolist():
            a, r = int(col[i]), int(rhs[i])
            if best is None or r * ba < br * a:
                best, ba, br = i, a, r
        return best

    def pivot(self, e, r):
        T = self.T
        p = int(T[r, e])
        s, ap = (-1 if p < 0 else 1), abs(p)
        if p < 0:
            self.stats["negative_pivots"] += 1
        if T.dtype != object and (2 * self._maxabs() ** 2 >= 1 << 62 or self.D >= 1 << 62):
            T = T.astype(object)
        prow = T[r].copy()
        c = s * T[:, e]
        N = T * ap
        N -= np.multiply.outer(c, prow)
        if self.D != 1:
            Q = N // self.D
            self.stats["inexact"] += int(((N - Q * self.D) != 0).sum())
        else:
            Q = N
        Q[r] = s * prow
        self.T, self.D = Q, ap
        self.basis[r] = e
        self.track()
        self.stats["pivots"] += 1

    solve = Model.solve


def slack_tableau(m, n, seed, entries=(0, 3), rhs=(1, 9), obj=(1, 3), density=1.0):
    """A seeded slack-form start [A | I | b] over the objective row -c, as int64: m rows of n variables
    with small non-negative entries, so that exact ties in pricing and in the ratio test are the rule and
    the fraction-free entries (minors of A) stay narrow; density < 1 zeroes entries of A at random, so that
    different variables meet different rows.  (T ((m + 1) x (n + m + 1)), basis)."""
    rng = np.random.default_rng(seed)
    T = np.zeros((m + 1, n + m + 1), dtype=np.int64)
    T[:m, :n] = rng.integers(entries[0], entries[1] + 1, size=(m, n))
    if density < 1.0:
        T[:m, :n] *= rng.random(size=(m, n)) < density
    T[np.arange(m), n + np.arange(m)] = 1
    T[:m, -1] = rng.integers(rhs[0], rhs[1] + 1, size=m)
    T[m, :n] = -rng.integers(obj[0], obj[1] + 1, size=n)
    return T, np.arange(n, n + m, dtype=np.int64)


def mixed_problem(lp, n, m_le, m_ge, m_eq, seed, paired=2):
    """A feasible all-integer LP with <=, >= and = rows (small entries; x = 1 is feasible) and `paired`
    rows that stand twice, as a . x <= b and further down as a . x = b: the two tie in every ratio test,
    the slack of the first leaves, and the artificial variable of the second stays basic at zero over a
    row that is not zero -- it has to be driven out after phase 1."""
    rng = random.Random(seed)
    names = ["x%d" % i for i in range(n)]
    cons, twice = [], []
    for _ in range(paired):
        a = [rng.randint(0, 3) for _ in names]
        cons.append(("<=", list(zip(names, a)), sum(a)))
        twice.append(("=", list(zip(names, a)), sum(a)))
    for op, count in (("<=", m_le), (">=", m_ge), ("=", m_eq)):
        for _ in range(count):
            a = [rng.randint(0, 3) for _ in names]
            tot = sum(a)
            rhs = tot + rng.randint(1, 6) if op == "<=" else (max(tot - rng.randint(1, 6), 0) if op == ">=" else tot)
            cons.append((op, list(zip(names, a)), rhs))
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, rng.randint(1, 3)) for v in names], constraints=cons + twice)


def wide_mixed_problem(lp, seed, e):
    """wide_problem with a >= and an = row among its four (x = 1 is feasible): a two-phase job whose
    fraction-free entries outgrow 64 bits on the way -- where, depends on e and the seed."""
    rng = random.Random(seed)
    names = ["x%d" % i for i in range(4)]
    cons = []
    for op in ("<=", ">=", "=", "<="):
        a = [rng.randint(1 << e, 1 << (e + 1)) for _ in names]
        d = rng.randint(1 << e, 1 << (e + 1))
        cons.append((op, list(zip(names, a)), sum(a) + (d if op == "<=" else -d if op == ">=" else 0)))
    return lp.Problem(type="max", vars=names, objective_var="w",
                      objective_func=[(v, rng.randint(1, 1 << e)) for v in names], constraints=cons)


# ---- k_x_select's two reductions, thread for thread ------------------------------------------------
def select_tree(n, better, equal, tie_clause=True, threads=256):
    """The index k_x_select's reduction pattern picks among 0 .. n-1.  better(a, b): candidate a strictly
    beats b (b = -1: none yet; a candidate that may not take part beats nothing); equal(a, b): a tie.
    Every thread scans tid, tid + threads, ... and keeps the first best; a tree over the threads' keeps then
    takes the other element when it is strictly better or, with tie_clause, equal with a lower index.
    Without tie_clause (a kernel that lost the clause) the element at the lower thread position survives a
    tie, whatever its index."""
    keep = [-1] * threads
    for t in range(threads):
        for j in range(t, n, threads):
            if better(j, keep[t]):
                keep[t] = j
    s = threads // 2
    while s:
        for t in range(s):
            o = t + s
            if keep[o] >= 0 and (keep[t] < 0 or better(keep[o], keep[t]) or
                                 (tie_clause and equal(keep[o], keep[t]) and keep[o] < keep[t])):
                keep[t] = keep[o]
        s //= 2
    return keep[0]


def select_price(obj, is_max, tie_clause=True):
    """The pricing reduction over the objective entries obj[0 .. nv): the index at the tree's root (the
    kernel then tests its sign)."""
    obj = [int(x) for x in obj]

    def better(a, b):
        return b < 0 or (obj[a] < obj[b] if is_max else obj[a] > obj[b])
    return select_tree(len(obj), better, lambda a, b: obj[a] == obj[b], tie_clause)


def select_ratio(col, rhs, tie_clause=True):
    """The ratio-test reduction over rows with col > 0, cross-multiplied; -1: no row."""
    col, rhs = [int(x) for x in col], [int(x) for x in rhs]

    def better(a, b):
        if col[a] <= 0:
            return False
        return b < 0 or rhs[a] * col[b] < rhs[b] * col[a]
    return select_tree(len(col), better, lambda a, b: rhs[a] * col[b] == rhs[b] * col[a], tie_clause)
