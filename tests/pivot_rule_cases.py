"""Shared by the pivot-rule tests: the three rules of mi355x_xtab_set_pivot_rule restated on the fraction-free
models of tests/exact_cases.py, and the inputs the tests run.

Rule 0 ("dantzig") is exact_cases.Model / VecModel as they stand.  Rule 1 ("bland") prices the lowest column
whose objective entry has the entering sign and breaks ties of the strict minimum ratio by the lowest basis
column.  Rule 2 ("dantzig-bland") is rule 0 until a selected pivot is degenerate (its row's right-hand side is
0 at selection), then rule 1 until one is not.  `stalled` is a class attribute, so a model made with
from_state -- the main model of model_solve's hand-over -- starts with the flag clear, and the drive-outs,
which call pivot() alone, neither read nor write it."""
from fractions import Fraction

import numpy as np

from tests import exact_cases as ec

RULES = ("dantzig", "bland", "dantzig-bland")
PERIOD = [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (5, 1)]
BEALE_TRACE = [(0, 0), (1, 1), (2, 0), (3, 1), (0, 2), (4, 1)]
CHVATAL_TRACE = [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (0, 1), (2, 2)]


def _bland_price(obj, nv, is_max):
    for j in range(nv):
        if (obj[j] < 0) if is_max else (obj[j] > 0):
            return j
    return None


def _bland_ratio(col, rhs, key):
    """The row of the strict minimum rhs / col over col > 0; ties go to the lowest key(i)."""
    best = None
    for i in range(len(col)):
        a = int(col[i])
        if a <= 0:
            continue
        if best is None:
            best = i
            continue
        lhs, rhs_ = int(rhs[i]) * int(col[best]), int(rhs[best]) * a
        if lhs < rhs_ or (lhs == rhs_ and key(i) < key(best)):
            best = i
    return best


class _Rules:
    """price / ratio of a rule over a model's own (rule 0); mixed in before Model or VecModel."""
    stalled = False
    bland_always = False                      # rule 1
    switching = False                         # rule 2
    row_key = False                           # the wrong tie key: the row index instead of basis[i]

    def _obj(self):
        return [int(x) for x in self.T[-1][:self.nv]]

    def _bland_now(self):
        return self.bland_always or (self.switching and self.stalled)

    def price(self, is_max):
        if not self._bland_now():
            return super().price(is_max)
        return _bland_price(self._obj(), self.nv, is_max)

    def ratio(self, e):
        if not self._bland_now():
            r = super().ratio(e)
        else:
            T = self.T
            m = len(T) - 1
            if isinstance(T, np.ndarray):
                col, rhs = T[:m, e].tolist(), T[:m, self.nv].tolist()
            else:
                col, rhs = [row[e] for row in T[:m]], [row[self.nv] for row in T[:m]]
            r = _bland_ratio(col, rhs, (lambda i: i) if self.row_key else (lambda i: self.basis[i]))
        if r is not None:                                     # the flag: set by each selected pivot
            self.stalled = int(self.T[r][self.nv]) == 0
        return r


class BlandModel(_Rules, ec.Model):
    bland_always = True


class DantzigBlandModel(_Rules, ec.Model):
    switching = True


class RowKeyBlandModel(_Rules, ec.Model):
    bland_always = row_key = True


class BlandVec(_Rules, ec.VecModel):
    bland_always = True


class DantzigBlandVec(_Rules, ec.VecModel):
    switching = True


class RowKeyBlandVec(_Rules, ec.VecModel):
    bland_always = row_key = True


MODELS = {"dantzig": ec.Model, "bland": BlandModel, "dantzig-bland": DantzigBlandModel, "row-key": RowKeyBlandModel}
VEC_MODELS = {"dantzig": ec.VecModel, "bland": BlandVec, "dantzig-bland": DantzigBlandVec, "row-key": RowKeyBlandVec}


def chvatal(lp):
    """Chvatal's cycling LP (Linear Programming, 1983, p. 31) in Fractions: period 6 under the default rule."""
    F = Fraction
    names = ["x1", "x2", "x3", "x4"]
    return lp.Problem(type="max", vars=names, objective_var="z",
                      objective_func=[("x1", F(10)), ("x2", F(-57)), ("x3", F(-9)), ("x4", F(-24))],
                      constraints=[("<=", [("x1", F(1, 2)), ("x2", F(-11, 2)), ("x3", F(-5, 2)), ("x4", F(9))], F(0)),
                                   ("<=", [("x1", F(1, 2)), ("x2", F(-3, 2)), ("x3", F(-1, 2)), ("x4", F(1))], F(0)),
                                   ("<=", [("x1", F(1))], F(1))])


CYCLING = {"beale": (ec.beale, BEALE_TRACE, Fraction(5, 4)), "chvatal": (chvatal, CHVATAL_TRACE, Fraction(1))}


def solve_tabs(tabs, rule, max_pivots, vec=False, keep=None):
    """model_solve under a rule with a finite cap on either phase: (status, trace, final model, stats)."""
    cls = (VEC_MODELS if vec else MODELS)[rule]
    if not isinstance(tabs, tuple):
        t = cls(tabs.matrix, tabs.basis, tabs.var_count)
        trace = []
        st = t.solve(tabs.is_max, trace, max_pivots)
        return st, trace, t, t.stats
    return ec.model_solve(tabs, cls=cls, keep=keep, phase2_pivots=max_pivots)


def solve_state(T, basis, rule, max_pivots, is_max=True):
    """A VecModel of the rule on an integer start state (D = 1): (status, trace, model)."""
    m = VEC_MODELS[rule].from_state(T, 1, basis, T.shape[1] - 1)
    trace = []
    st = m.solve(is_max, trace, max_pivots)
    return st, trace, m


def degenerate_count(T, basis, trace):
    """How many pivots of a trace, replayed from the start state, are degenerate."""
    return sum(degenerate_flags(T, basis, trace))


WIDE_SLACK = dict(m=40, n=300, seed=1, rhs=(0, 2), density=0.5)          # 41 x 341: 340 priced columns
TALL_SLACK = dict(m=300, n=40, seed=0, rhs=(0, 2), density=0.5)          # 301 x 341: 300 ratio rows


def slack(m, n, seed, **kw):
    return ec.slack_tableau(m, n, seed, **kw)


def beale_variants(lp):
    """Beale's LP (cycles under the default rule) and three bounded LPs of its shape that do not."""
    F = Fraction
    names = ["x1", "x2", "x3", "x4"]

    def bounded(rows, rhs, obj):
        return lp.Problem(type="max", vars=names, objective_var="z", objective_func=list(zip(names, obj)),
                          constraints=[("<=", list(zip(names, a)), b) for a, b in zip(rows, rhs)])
    return [ec.beale(lp),
            bounded([[1, 2, 1, 1], [2, 1, 3, 1], [1, 1, 1, 2]], [10, 12, 9], [3, 2, 4, 1]),
            bounded([[F(1, 2), 1, 2, 1], [1, F(1, 3), 1, 3], [2, 2, 1, 1]], [7, 8, F(21, 2)], [1, 5, 2, F(3, 2)]),
            chvatal(lp)]


RESTART_CAP = 6


def restart_state():
    """A 64-bit start for rule 2 under a cap of RESTART_CAP pivots: zero right-hand sides but two and signed
    entries up to 2^20, so that the first pivots are degenerate and the entries outgrow 64 bits on the way."""
    rng = np.random.default_rng(4)
    m, n = 6, 8
    T = np.zeros((m + 1, n + m + 1), dtype=np.int64)
    T[:m, :n] = rng.integers(-(1 << 20), 1 << 20, size=(m, n))
    T[np.arange(m), n + np.arange(m)] = 1
    T[m - 2:m, -1] = rng.integers(1, 1 << 20, size=2)
    T[m, :n] = -rng.integers(1, 1 << 20, size=n)
    return T, np.arange(n, n + m, dtype=np.int64)


def degenerate_flags(T, basis, trace):
    """Per pivot of a trace, replayed from the start state: was it degenerate?"""
    m = ec.VecModel.from_state(T, 1, basis, T.shape[1] - 1)
    out = []
    for e, r in trace:
        out.append(int(m.T[r, m.nv]) == 0)
        m.pivot(e, r)
    return out


def handover_start(tabs, rule):
    """(T, D, basis) the main model of model_solve starts from under `rule`: what from_state receives."""
    seen = {}

    class Spy(MODELS[rule]):
        @classmethod
        def from_state(cls, T, D, basis, var_count, **kw):
            seen["start"] = ([list(r) for r in T], D, list(basis))
            return super().from_state(T, D, basis, var_count, **kw)
    ec.model_solve(tabs, cls=Spy, phase2_pivots=1)
    return seen["start"]
