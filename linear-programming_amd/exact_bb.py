"""Exact branch-and-bound (opt-in: ``mi355x_simplex_solver(p, exact=True, branch_and_bound=True)``).

The reference's integer solver (simplex-solver, src/simplex.lisp:462-542) tests integrality with
`integerp` (:475-480), which only a rational tableau can satisfy: on rationals it is a real
branch-and-bound.  `search` is that loop as a replay over speculatively solved nodes, with the policy of
csrc/host_bb.inc and the same argument for exactness: every entry the reference pushes is popped and
solved; a node's result depends only on its own rows; pruning is monotone.  So the replay sees the
same results in the same order for every width.  Integrality is ``denominator == 1``, the bounds are
floor / ceil of Fractions, the comparator is `<` (max) / `>` (min) on Fractions.

`DeviceRounds` is the `solve_round` of the GPU: the root goes through the one-problem exact route;
every other node is grouped by (depth, artificial rows), built on the device from the base problem's
general form and its node rows (mi355x_xbatch_create_nodes: k_xbb_assemble), solved as one batch of
exact tableaux in bounded calls, and read back with one light copy per batch (mi355x_xbatch_readback).
"""
import ctypes
import math
from fractions import Fraction

import numpy as np

from . import capi
from .conditions import InfeasibleProblemError, SolverError
from .exact import ExactTableau, XBatch, _declined, _int128, _num_den, _ptr, batch_in_chunks, pivot_rule_code

# outcomes of a trace row: the values of MI_BB_* (mi355x_simplex_solver_bb_trace)
BB_INFEASIBLE, BB_PRUNED, BB_BRANCHED, BB_INCUMBENT, BB_NOT_BETTER, BB_FAILED = range(6)
_I64_MAX = (1 << 63) - 1


class _Node:
    __slots__ = ("parent", "row", "depth", "solved", "status", "obj", "values", "viol", "child", "trace_index")

    def __init__(self, parent=-1, row=None, depth=0):
        self.parent, self.row, self.depth = parent, row, depth        # row: (var, sense, bound) that made it
        self.solved, self.status, self.obj, self.values, self.viol = False, None, None, None, None
        self.child, self.trace_index = [None, None], -1


class SearchResult:
    """status: MI_OPTIMAL (an incumbent), MI_INFEASIBLE (no integral point), MI_MAX_PIVOTS (the node cap), or
    what ended the search -- a node LP's status, or the exception of a declined node.  objective / values:
    the incumbent's, as `solve_round` returned them.  trace: the rows of mi355x_simplex_solver_bb_trace with
    variable names -- (parent trace index, var or None, sense, float(bound), outcome, float(objective) or
    NaN); objectives: the same objectives as Fractions (None where a row has none)."""

    def __init__(self):
        self.status, self.objective, self.values = None, None, None
        self.trace, self.objectives = [], []
        self.n_solved = self.max_depth = 0

    def stats(self):
        return {"processed": len(self.trace), "solved": self.n_solved, "max_depth": self.max_depth}


def _fractional(v):
    return v.denominator != 1


def search(problem, solve_round, width=1, max_nodes=0, fractional=_fractional, floor=math.floor, ceil=math.ceil):
    """simplex-solver (src/simplex.lisp:506-542).  solve_round(list of entries) -> per entry (status,
    objective, values): an entry is a tuple of rows (var, sense 0 `<=` / 1 `>=`, bound), newest first;
    values[var] is the variable's Fraction.  Up to `width` node LPs per round.
    fractional(v): the integrality test's negation (:474-479), floor / ceil: the branching bounds (:465-472) --
    the defaults are the rational search's; single_bb.py passes the float32 readings."""
    is_max = problem.type == "max"

    def better(inc, v):                                               # the comparator, :515
        return inc < v if is_max else inc > v
    nodes, stack, res = [_Node()], [0], SearchResult()
    best = None

    def prunable(n):
        return n.viol is not None and best is not None and not better(nodes[best].obj, n.obj)

    def child(i, which):                                              # gen-entries, :465-472
        n = nodes[i]
        if n.child[which] is None:
            v = n.values[n.viol]
            bound = floor(v) if which == 0 else ceil(v)
            nodes.append(_Node(i, (n.viol, which, bound), n.depth + 1))
            n.child[which] = len(nodes) - 1
        return n.child[which]

    def collect(i, out):                                              # the speculation policy of host_bb.inc
        if len(out) >= width:
            return
        n = nodes[i]
        if not n.solved:
            out.append(i)
            return
        if n.status != capi.MI_OPTIMAL or n.viol is None or prunable(n):
            return
        collect(child(i, 0), out)
        collect(child(i, 1), out)

    def entry(i):
        rows = []
        while nodes[i].parent >= 0:
            rows.append(nodes[i].row)
            i = nodes[i].parent
        return tuple(rows)

    def finished(status):
        res.status = status
        if best is not None:
            res.objective, res.values = nodes[best].obj, nodes[best].values
        return res

    while stack:                                                      # :517-539
        if max_nodes and len(res.trace) >= max_nodes:
            return finished(capi.MI_MAX_PIVOTS)
        i = stack[-1]
        if not nodes[i].solved:
            ids = []
            for s in reversed(stack):
                collect(s, ids)
            for k, (status, obj, values) in zip(ids, solve_round([entry(k) for k in ids])):
                n = nodes[k]
                n.solved, n.status = True, status
                res.n_solved += 1
                if status == capi.MI_OPTIMAL:
                    n.obj, n.values = obj, values
                    n.viol = next((v for v in problem.integer_vars if fractional(values[v])), None)   # :474-479
            continue
        stack.pop()
        n = nodes[i]
        n.trace_index = len(res.trace)
        res.max_depth = max(res.max_depth, n.depth)
        var, sense, bound = n.row if n.row else (None, 0, 0)
        parent = nodes[n.parent].trace_index if n.parent >= 0 else -1

        def row(outcome):
            res.trace.append((parent, var, sense, float(bound), outcome, float("nan") if n.obj is None else float(n.obj)))
            res.objectives.append(n.obj)
        if n.status == capi.MI_INFEASIBLE:                            # build-and-solve -> :infeasible
            row(BB_INFEASIBLE)
            continue
        if n.status != capi.MI_OPTIMAL:                               # any other condition ends the solve
            row(BB_FAILED)
            return finished(n.status)
        if prunable(n):
            n.values = None
            row(BB_PRUNED)
        elif n.viol is not None:                                      # (append (gen-entries tab entry) stack)
            ge, le = child(i, 1), child(i, 0)
            stack.extend((ge, le))
            n.values = None                                           # (both children exist: its batch may go)
            row(BB_BRANCHED)
        elif best is None or better(nodes[best].obj, n.obj):
            if best is not None:
                nodes[best].values = None                             # (a beaten incumbent lets its batch go)
            best = i
            row(BB_INCUMBENT)
        else:
            n.values = None
            row(BB_NOT_BETTER)
    return finished(capi.MI_OPTIMAL if best is not None else capi.MI_INFEASIBLE)     # :540-542


# ------------------------------------------------------------------ the base problem, once per search
class GeneralForm:
    """The base problem's general form on Fractions (build_tableau(general=True)) and what places a node
    row in it: host_problem.cpp's build(general=true)."""

    def __init__(self, problem, device=0):
        from .simplex import build_tableau
        t = build_tableau(problem, problem, device=device, exact=True, general=True)
        self.problem, self.matrix, self.basis, self.mapping = problem, t._matrix, t._basis, t.var_mapping
        bounds = dict(problem.var_bounds)
        self.nb = sum(1 for v in problem.vars if v in bounds and None not in bounds[v])
        self.ncv = sum(2 if self.mapping[v][0] == "signed" else 1 for v in problem.vars)
        self.index = {v: i for i, v in enumerate(problem.vars)}
        self.kind = [("positive", "negative", "signed").index(self.mapping[v][0]) for v in problem.vars]
        self.col = [self.mapping[v][1] for v in problem.vars]
        self.offset = [Fraction(0) if self.mapping[v][0] == "signed" else self.mapping[v][2] for v in problem.vars]
        self.n_art = int((self.basis == self.matrix.shape[1]).sum())
        # the integer scale (capi_exact_bb.inc): the product of the rows' LCMs -- the objective row's folded in,
        # as every exact handle starts -- times the LCM of the offsets' denominators
        lcm = lambda xs: math.lcm(*[x.denominator for x in xs]) if len(xs) else 1
        L = [lcm(list(row)) for row in self.matrix]
        self.Db = math.prod(L) * lcm(self.offset)

    def row_artificial(self, var, sense, bound):
        """Does the node row need an artificial variable?  (bound - offset < 0 flips its sense, :243-252)"""
        return (1 - sense if bound - self.offset[self.index[var]] < 0 else sense) == 1


def node_tableaux(g, entry):
    """The node's tableaux from the general form and its rows, at ONE integer scale Db: (Db, main rows,
    main basis, artificial rows or None, artificial basis or None), every entry a Python int.  The host
    statement of what k_xbb_assemble writes (csrc/kernels_exact_bb.inc)."""
    B, d, Db = g.matrix, len(entry), g.Db
    rows_b, cols_b = B.shape
    m, num_cols, at = rows_b - 1 + d, cols_b + d, g.ncv + g.nb

    def base_row(r):
        src = [int(x * Db) for x in B[r]]
        return src[:at] + [0] * d + src[at:]
    M, basis = [], []
    for R in range(m):
        if g.nb <= R < g.nb + d:
            var, sense, bound = entry[R - g.nb]
            v = g.index[var]
            row = [0] * num_cols
            row[g.col[v]] = -Db if g.kind[v] == 1 else Db
            if g.kind[v] == 2:
                row[g.col[v] + 1] = -Db
            row[-1] = int(bound * Db - g.offset[v] * Db)
            if row[-1] < 0:
                row, sense = [-x for x in row], 1 - sense
            row[g.ncv + R] = Db if sense == 0 else -Db
            M.append(row)
            basis.append(g.ncv + R if sense == 0 else num_cols)
        else:
            r = R if R < g.nb else R - d
            b = int(g.basis[r])
            M.append(base_row(r))
            basis.append(num_cols if b == cols_b else (b + d if b >= at else b))
    M.append(base_row(rows_b - 1))
    art_rows = [R for R in range(m) if basis[R] == num_cols]
    if not art_rows:
        return Db, M, basis, None, None
    n_art = len(art_rows)
    A = [row[:-1] + [0] * n_art + row[-1:] for row in M[:m]]
    abasis = list(basis)
    for k, R in enumerate(reversed(art_rows)):                        # push order, :257, :261, :296-300
        A[R][num_cols - 1 + k] = Db
        abasis[R] = num_cols - 1 + k
    last = [0] * (num_cols + n_art)
    for c in list(range(num_cols - 1)) + [num_cols + n_art - 1]:
        last[c] = sum(A[R][c] for R in art_rows)
    A.append(last)
    return Db, M, basis, A, abasis


class Base:
    """mi355x_xbb_base: the general form on the device."""

    def __init__(self, g, device=0):
        self.g, self.handle = g, None
        num, den = _num_den(g.matrix)
        off = np.empty((len(g.offset), 1), dtype=object)
        off[:, 0] = g.offset
        onum, oden = _num_den(off)
        kind = np.array(g.kind, dtype=np.int32)
        col = np.array(g.col, dtype=np.int64)
        basis = np.ascontiguousarray(g.basis, dtype=np.int64)
        h = ctypes.c_void_p()
        rc = capi.lib().mi355x_xbb_base_create(ctypes.byref(h), num.shape[0], num.shape[1], _ptr(num), _ptr(den),
                                               _ptr(basis) if basis.size else None, g.ncv, g.nb, len(g.kind), _ptr(kind),
                                               _ptr(col), _ptr(onum), _ptr(oden), device)
        if rc == capi.MI_EXACT_OVERFLOW:
            raise _declined(("overflow", "128 bits"))
        capi.check(rc, "mi355x_xbb_base_create")
        self.handle = h

    def create_nodes(self, entries, min_bits=0, pivot_rule="dantzig"):
        """mi355x_xbatch_create_nodes for entries of one depth and one number of artificial rows:
        (main XBatch, artificial XBatch or None), both with pivot_rule set."""
        g, n, d = self.g, len(entries), len(entries[0])
        flat = [r for e in entries for r in e]
        if any(abs(b) > _I64_MAX for _, _, b in flat):
            raise _declined(("bound", "64 bits"))
        var = np.array([g.index[v] for v, _, _ in flat], dtype=np.int64)
        sense = np.array([s for _, s, _ in flat], dtype=np.int32)
        bound = np.array([int(b) for _, _, b in flat], dtype=np.int64)
        hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
        rc = capi.lib().mi355x_xbatch_create_nodes(ctypes.byref(hm), ctypes.byref(ha), self.handle, n, d, _ptr(var),
                                                   _ptr(sense), _ptr(bound), int(min_bits))
        if rc == capi.MI_UNSUPPORTED:
            raise _declined(("batch", "shape", g.matrix.shape[0] + d, g.matrix.shape[1] + d))
        capi.check(rc, "mi355x_xbatch_create_nodes")
        rows, cols = g.matrix.shape[0] + d, g.matrix.shape[1] + d
        n_art = g.n_art + sum(g.row_artificial(*r) for r in entries[0])
        main = XBatch.from_handle(hm, n, rows, cols)
        art = XBatch.from_handle(ha, n, rows, cols + n_art) if ha else None          # (owned from here on)
        main.set_pivot_rule(pivot_rule)
        if art:
            art.set_pivot_rule(pivot_rule)
        return main, art

    def close(self):
        h, self.handle = self.handle, None
        if h:
            capi.lib().mi355x_xbb_base_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def readback(xb):
    """mi355x_xbatch_readback: per member (D, right-hand sides, objective row, basis) as Python ints / an
    int64 array, or None for a member past 128 bits."""
    R, C, n = xb.rows, xb.cols, xb.n_lps
    vals = np.empty((n, 1 + R + C, 2), dtype=np.int64)
    basis = np.empty((n, max(R - 1, 0)), dtype=np.int64)
    st = np.empty(n, dtype=np.int32)
    capi.check(capi.lib().mi355x_xbatch_readback(xb.handle, _ptr(vals), _ptr(basis) if basis.size else None, _ptr(st)),
               "mi355x_xbatch_readback")
    out = []
    for q in range(n):
        if st[q] != capi.MI_OK:
            out.append(None)
            continue
        ints = [_int128(lo, hi) for lo, hi in vals[q].tolist()]
        out.append((ints[0], ints[1:1 + R], ints[1 + R:], basis[q]))
    return out


class LightSolution:
    """What tableau-objective-value and tableau-variable read of one solved member (src/simplex.lisp:74-107),
    with the batch it lives in: values[var] is the variable's Fraction."""

    def __init__(self, g, light, batch, q):
        self.g, (self.D, self.rhs, self.obj_row, self.basis), self.batch, self.q = g, light, batch, q
        self.objective = Fraction(self.obj_row[-1], self.D)

    def _basic(self, col):
        pos = np.nonzero(self.basis == col)[0]                        # `position`: the first match
        return Fraction(self.rhs[int(pos[0])], self.D) if pos.size else Fraction(0)

    def __getitem__(self, var):
        mp = self.g.mapping[var]
        if mp[0] == "positive":
            return mp[2] + self._basic(mp[1])
        if mp[0] == "negative":
            return mp[2] - self._basic(mp[1])
        return self._basic(mp[1]) - self._basic(mp[1] + 1)

    def tableau(self):
        """The member downloaded in full, as the solved ExactTableau of the node."""
        g, (R, C) = self.g, (self.batch.rows, self.batch.cols)
        t = ExactTableau.__new__(ExactTableau)                        # (its matrix comes with the first read)
        t.problem = t.instance_problem = g.problem
        t.var_count, t.constraint_count, t.var_mapping = C - 1, R - 1, g.mapping
        t.device = t.min_bits = t.n_pivots = 0
        t.phase1 = t._handle = None
        t._matrix, t._basis = np.empty((R, C), dtype=object), np.empty(R - 1, dtype=np.int64)
        t._batch, t._stale = (self.batch, self.q), True
        return t


class DeviceRounds:
    """The `solve_round` of the GPU (see the module's docstring)."""

    def __init__(self, problem, device=0, max_pivots=0, min_bits=0, chunk=None, pivot_rule="dantzig"):
        self.problem, self.device, self.max_pivots, self.min_bits, self.chunk = problem, device, max_pivots, min_bits, chunk
        pivot_rule_code(pivot_rule)
        self.pivot_rule = pivot_rule                                  # of the root and of every node batch
        self.g = self.base = None
        self.root = None                                              # the root's solved ExactTableau
        self.declined = 0                                             # nodes that came back declined

    def _root(self):
        from .exact import n_solve_exact
        from .simplex import build_tableau, tableau_objective_value, tableau_variable
        try:
            tabs = build_tableau(self.problem, self.problem, device=self.device, exact=True, min_bits=self.min_bits)
            t = n_solve_exact(tabs, max_pivots=self.max_pivots, chunk=self.chunk, pivot_rule=self.pivot_rule)
        except SolverError as e:
            return _status_of(e), None, None
        self.root = t
        return capi.MI_OPTIMAL, tableau_objective_value(t), {v: tableau_variable(t, v) for v in self.problem.vars}

    def __call__(self, entries):
        out = [None] * len(entries)
        groups = {}
        for k, e in enumerate(entries):
            if not e:
                out[k] = self._root()
                continue
            if self.base is None:
                self.g = GeneralForm(self.problem, self.device)
                self.base = Base(self.g, self.device)
            groups.setdefault((len(e), sum(self.g.row_artificial(*r) for r in e)), []).append(k)
        is_max = self.problem.type == "max"
        for ks in groups.values():
            try:
                main, art = self.base.create_nodes([entries[k] for k in ks], self.min_bits, self.pivot_rule)
            except SolverError as e:                                  # a shape or a bound the batch declines
                for k in ks:
                    out[k] = (e, None, None)
                self.declined += len(ks)
                continue
            st, _ = batch_in_chunks(art or main, main if art else None, is_max, self.max_pivots, self.chunk)
            light = readback(main)
            for q, k in enumerate(ks):
                if st[q] == capi.MI_EXACT_OVERFLOW or (st[q] == capi.MI_OPTIMAL and light[q] is None):
                    out[k] = (_declined(("overflow", "128 bits")), None, None)
                    self.declined += 1
                elif st[q] == capi.MI_OPTIMAL:
                    s = LightSolution(self.g, light[q], main, q)
                    out[k] = (capi.MI_OPTIMAL, s.objective, s)
                else:
                    out[k] = (int(st[q]), None, None)
        return out


def _status_of(e):
    """A solve's exception as the status the search replays (a declined one stays the exception)."""
    from .conditions import UnboundedProblemError
    if isinstance(e, UnboundedProblemError):
        return capi.MI_UNBOUNDED
    if isinstance(e, InfeasibleProblemError):
        return capi.MI_INFEASIBLE
    return e


class ExactBranchAndBound:
    """One exact search on the GPU: run() -> the incumbent's solved ExactTableau, or raises the reference's
    errors; trace() / stats() as native.BranchAndBound, `result.objectives` the trace's objectives as Fractions."""

    def __init__(self, problem, width=1, device=0, max_pivots=0, max_nodes=0, min_bits=0, chunk=None, pivot_rule="dantzig"):
        self.problem, self.width, self.max_nodes = problem, int(width), int(max_nodes)
        self.rounds = DeviceRounds(problem, device=device, max_pivots=max_pivots, min_bits=min_bits, chunk=chunk,
                                   pivot_rule=pivot_rule)
        self.result = None

    def run(self):
        from .simplex import _raise_for
        if self.width < 1:
            raise ValueError("bb_width must be >= 1")
        r = self.result = search(self.problem, self.rounds, self.width, self.max_nodes)
        if isinstance(r.status, Exception):
            raise r.status
        if r.status == capi.MI_MAX_PIVOTS and self.max_nodes and len(r.trace) >= self.max_nodes:
            raise SolverError("node cap reached (max_nodes=%d)" % self.max_nodes)
        _raise_for(r.status)
        return r.values.tableau() if isinstance(r.values, LightSolution) else self.rounds.root

    def trace(self):
        return list(self.result.trace)

    def stats(self):
        return dict(self.result.stats(), declined=self.rounds.declined)


def solve_branch_and_bound_exact(problem, width=1, device=0, max_pivots=0, max_nodes=0, min_bits=0, chunk=None,
                                 pivot_rule="dantzig"):
    """simplex-solver with integer variables (src/simplex.lisp:506-542) on a problem whose numbers are all
    rational: the incumbent as a solved ExactTableau (its read-back in Fractions).  pivot_rule: of the root's
    solve and of every node batch (exact.py)."""
    return ExactBranchAndBound(problem, width, device, max_pivots, max_nodes, min_bits, chunk, pivot_rule).run()
