"""Single-float branch-and-bound (opt-in: ``mi355x_simplex_solver(p, precision="single", branch_and_bound=True)``).

The reference's integer solver (simplex-solver, src/simplex.lisp:462-542) on a problem written with single-floats
runs in single-float arithmetic with single-float-epsilon thresholds.  This is that search: ``exact_bb.search`` --
the one copy of the loop, a replay over speculatively solved nodes whose result does not depend on the width --
with the float32 readings of the integrality test and the branching bounds:

    integral     v == floor(v) on the np.float32 that tableau-variable returns (the f32 reading of `integerp`,
                 as the double path reads it in f64); int_tolerance > 0 counts |v - round(v)| <= int_tolerance *
                 single-float-epsilon, computed in float32, as integral instead
    bounds       floor(v) and ceiling(v) as exact Python integers, what Lisp's `floor` / `ceiling` return.  They are
                 not numbers of the user's: a binary32 holds each exactly, and check_single_problem's |x| <= 2**24
                 rule is for the base problem, which is checked once
    comparator   `<` (max) / `>` (min) on np.float32 objective values; a NaN compares false

A node's tableaux are what build_tableau_single makes of `entry ++ problem constraints` under Lisp's contagion, bit
for bit.  ``DeviceRounds`` solves the root through build_tableau_single + n_solve_tableau and groups every other
node by (depth, artificial rows); a group is written by the device from the base problem's float32 general form and
its node rows (mi355x_sbatch_create_nodes: k_sbb_assemble), solved as one batch or a pair of batches in bounded
calls, and read back with one light copy (mi355x_sbatch_readback).  Three facts about Lisp's contagion decide that
the float32 assembly is Lisp's build:

    a  a node row's right-hand side bound - 1 * offset has two binary32 operands, so the exact-integer route and
       the float route round the same exact difference once; a node row negated for a negative right-hand side
       negates integer zeros: +0.0, never -0.0, in its other columns
    b  the columns inserted into base rows are integer zeros: +0.0 even in a base row that build-tableau negated
    c  the artificial objective row is a column sum in increasing row order in which integers stay exact among
       themselves; a float32 running sum is the same while every integer partial sum is exact, which holds while
       the absolute values of a column's integer entries sum to at most 2**24 -- the guard
       (GeneralFormSingle.device_ok).  A group that fails it is built on the host (lowering.build with SINGLE) and
       goes through SingleBatch.from_arrays; a shape beyond the batch's LDS budget goes node by node through
       SingleTableau -- or, with beyond_lds=True and at least single.global_batch_min_members nodes in the group,
       as ONE global-form batch or pair, device-built (mi355x_sbatch_create_nodes_global) or host-built alike.
"""
import ctypes
import math

import numpy as np

from . import capi, lists
from .capi import _ptr
from .conditions import SolverError, UnsupportedConstraintError
from .exact_bb import _I64_MAX, _status_of, search
from .lowering import assemble, build, lower
from .problem import Problem
from .single import (EPSILON_SINGLE, LDS_BUDGET, SINGLE, SingleBatch, SingleTableau, build_tableau_single,
                     check_single_problem, global_batch_min_members, single_lds_bytes, solve_status)
from .simplex import tableau_objective_value, tableau_variable

F32 = np.float32
_EXACT_INTS = 2 ** 24


# ------------------------------------------------------------------ the float32 readings
def fractional(int_tolerance=0):
    """The negation of the integrality test on an np.float32 (module docstring)."""
    tol = F32(F32(int_tolerance) * EPSILON_SINGLE)

    def test(v):
        v = F32(v)
        if int_tolerance > 0:
            return not (abs(F32(v - np.round(v))) <= tol)
        return not (v == np.floor(v))
    return test


def floor(v):
    return math.floor(float(v))


def ceil(v):
    return math.ceil(float(v))


def node_problem(problem, entry):
    """The node's problem: constraints = entry ++ problem-constraints (src/simplex.lisp:465-472, :520)."""
    rows = [("<=" if sense == 0 else ">=", [(var, 1)], int(bound)) for var, sense, bound in entry]
    return Problem(type=problem.type, vars=list(problem.vars), objective_var=problem.objective_var,
                   objective_func=list(problem.objective_func), integer_vars=list(problem.integer_vars),
                   var_bounds=list(problem.var_bounds), constraints=rows + list(problem.constraints))


def host_tableaux(problem, entry, fp_tolerance=1024, device=0):
    """build-tableau of the node problem on the host: a SingleTableau or [art, main].  The base problem's numbers
    were checked once; the bounds are exact integers Lisp made itself."""
    def make(inst, M, basis, mapping):
        return SingleTableau(problem, inst, M, basis, M.shape[1] - 1, M.shape[0] - 1, mapping, fp_tolerance, device)
    return build(problem, node_problem(problem, entry), SINGLE, make)


# ------------------------------------------------------------------ the base problem, once per search
class GeneralFormSingle:
    """The base problem's general form in float32 (lowering.build's steps with SINGLE, general=True), what places
    a node row in it, and the guard of fact c."""

    def __init__(self, problem):
        check_single_problem(problem)
        L, ncv, constraints, mapping = lower(problem, SINGLE, problem, room=True)
        M, basis, _, _ = assemble(L, ncv, constraints, SINGLE, True, general=True)
        # which entries Lisp holds as integers is known only before the coercion to float32
        self.col_int_sum = [sum(abs(x.v) for x in M[:-1, c] if type(x.v) is int) for c in range(M.shape[1])]
        self.problem, self.matrix, self.basis, self.mapping = problem, SINGLE.matrix(M), basis, SINGLE.mapping(mapping)
        bounds = dict(problem.var_bounds)
        self.nb = sum(1 for v in problem.vars if v in bounds and None not in bounds[v])
        self.ncv = ncv
        self.index = {v: i for i, v in enumerate(problem.vars)}
        self.kind = [("positive", "negative", "signed").index(self.mapping[v][0]) for v in problem.vars]
        self.col = [self.mapping[v][1] for v in problem.vars]
        self.offset = [F32(0) if self.mapping[v][0] == "signed" else F32(self.mapping[v][2]) for v in problem.vars]
        self.n_art = int((self.basis == self.matrix.shape[1]).sum())

    def row_rhs(self, var, bound):
        """float(bound) - offset: one float32 subtraction (fact a)."""
        v = self.index[var]
        return F32(bound) if self.kind[v] == 2 else F32(F32(bound) - self.offset[v])

    def row_artificial(self, var, sense, bound):
        """Does the node row need an artificial variable?  (a negative right-hand side flips its sense, :243-252)"""
        return (1 - sense if self.row_rhs(var, bound) < 0 else sense) == 1

    def device_ok(self, entry):
        """The guard: with this node's rows, do the integer entries of every column sum to at most 2**24 in
        absolute value?  A node row adds 1 in its variable's column(s) and |rhs| in the last column, counted
        whenever the right-hand side is integer-valued (the rule of mi355x_sbatch_create_nodes)."""
        total = list(self.col_int_sum)
        for var, _, bound in entry:
            v = self.index[var]
            total[self.col[v]] += 1
            if self.kind[v] == 2:
                total[self.col[v] + 1] += 1
            r = abs(float(self.row_rhs(var, bound)))
            if r == math.floor(r):
                total[-1] += r
        return all(t <= _EXACT_INTS for t in total)


def node_tableaux_single(g, entry):
    """The node's tableaux from the float32 general form and its rows: (main matrix, main basis, artificial matrix
    or None, artificial basis or None).  The host statement of what k_sbb_assemble writes
    (csrc/kernels_single_bb.inc), in float32 operation for operation."""
    B, d = g.matrix, len(entry)
    rows_b, cols_b = B.shape
    m, num_cols, at = rows_b - 1 + d, cols_b + d, g.ncv + g.nb
    M = np.zeros((m + 1, num_cols), dtype=F32)                            # (+0.0 everywhere: facts a and b)
    basis = np.zeros(m, dtype=np.int64)

    def base_row(r):
        return np.concatenate([B[r, :at], np.zeros(d, dtype=F32), B[r, at:]])
    for R in range(m):
        if g.nb <= R < g.nb + d:
            var, sense, bound = entry[R - g.nb]
            v = g.index[var]
            rhs = g.row_rhs(var, bound)
            flip = bool(rhs < 0)
            if flip:
                rhs, sense = F32(-rhs), 1 - sense
            M[R, g.col[v]] = F32(-1 if (g.kind[v] == 1) != flip else 1)
            if g.kind[v] == 2:
                M[R, g.col[v] + 1] = F32(1 if flip else -1)
            M[R, g.ncv + R] = F32(1 if sense == 0 else -1)
            M[R, -1] = rhs
            basis[R] = g.ncv + R if sense == 0 else num_cols
        else:
            r = R if R < g.nb else R - d
            b = int(g.basis[r])
            M[R] = base_row(r)
            basis[R] = num_cols if b == cols_b else (b + d if b >= at else b)
    M[m] = base_row(rows_b - 1)
    art_rows = [R for R in range(m) if basis[R] == num_cols]
    if not art_rows:
        return M, basis, None, None
    n_art = len(art_rows)
    A = np.zeros((m + 1, num_cols + n_art), dtype=F32)
    A[:m, :num_cols - 1], A[:m, -1] = M[:m, :num_cols - 1], M[:m, -1]
    for c in list(range(num_cols - 1)) + [num_cols + n_art - 1]:         # increasing rows, from 0.0 (:302-316)
        acc = F32(0)
        for R in art_rows:
            acc = F32(acc + A[R, c])
        A[m, c] = acc
    abasis = basis.copy()
    for k, R in enumerate(reversed(art_rows)):                            # push order, :257, :261, :296-300
        A[R, num_cols - 1 + k] = F32(1)
        abasis[R] = num_cols - 1 + k
    return M, basis, A, abasis


class Base:
    """mi355x_sbb_base: the float32 general form on the device."""

    def __init__(self, g, device=0):
        self.g, self.handle, self._sense_said = g, None, False
        M = np.ascontiguousarray(g.matrix, dtype=F32)
        basis = np.ascontiguousarray(g.basis, dtype=np.int64)
        kind, col = np.array(g.kind, dtype=np.int32), np.array(g.col, dtype=np.int64)
        off = np.array(g.offset, dtype=F32)
        sums = np.array([min(float(s), 2.0 ** 63) for s in g.col_int_sum], dtype=np.float64)
        h = ctypes.c_void_p()
        capi.check(capi.lib().mi355x_sbb_base_create(ctypes.byref(h), M.shape[0], M.shape[1], _ptr(M),
                                                     _ptr(basis) if basis.size else None, g.ncv, g.nb, len(g.kind),
                                                     _ptr(kind), _ptr(col), _ptr(off), _ptr(sums), int(device)),
                   "mi355x_sbb_base_create")
        self.handle = h

    def create_nodes(self, entries, form="lds"):
        """mi355x_sbatch_create_nodes for entries of one depth and one number of artificial rows: (main
        SingleBatch, artificial SingleBatch or None).  A bound beyond 64 bits is declined; a group the library
        declines (the guard, the LDS budget) raises capi.Mi355xError with code MI_UNSUPPORTED.  form="global":
        mi355x_sbatch_create_nodes_global, the same tableaux as members of global-form batches -- every shape whose
        pivot row and column snapshot fit the budget."""
        if form not in ("lds", "global"):
            raise ValueError("form=%r: \"lds\" (default) or \"global\"" % (form,))
        g, n, d = self.g, len(entries), len(entries[0])
        flat = [r for e in entries for r in e]
        if any(abs(b) > _I64_MAX for _, _, b in flat):
            raise UnsupportedConstraintError(("single", "bound", "64 bits"), "mi355x-simplex")
        var = np.array([g.index[v] for v, _, _ in flat], dtype=np.int64)
        sense = np.array([s for _, s, _ in flat], dtype=np.int32)
        bound = np.array([int(b) for _, _, b in flat], dtype=np.int64)
        hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
        name = "mi355x_sbatch_create_nodes_global" if form == "global" else "mi355x_sbatch_create_nodes"
        capi.check(getattr(capi.lib(), name)(ctypes.byref(hm), ctypes.byref(ha), self.handle, n, d, _ptr(var),
                                             _ptr(sense), _ptr(bound)), name)
        rows, cols = g.matrix.shape[0] + d, g.matrix.shape[1] + d
        n_art = g.n_art + sum(g.row_artificial(*r) for r in entries[0])
        main = SingleBatch(hm, n, rows, cols)
        return main, (SingleBatch(ha, n, rows, cols + n_art) if ha else None)

    def create_nodes_ragged(self, entries):
        """mi355x_sbatch_create_nodes_ragged for entries of ANY depths: (main SingleBatch, artificial SingleBatch or
        None), both ragged.  Either no node has artificial rows or every node has at least one (the counts may
        differ): the library declines a mixture with MI_BAD_ARG.  The guard, the assembly's LDS and the batch's budget
        decline with MI_UNSUPPORTED, the node named; a bound beyond 64 bits is declined as in create_nodes."""
        g, n = self.g, len(entries)
        flat = [r for e in entries for r in e]
        if any(abs(b) > _I64_MAX for _, _, b in flat):
            raise UnsupportedConstraintError(("single", "bound", "64 bits"), "mi355x-simplex")
        depth = np.array([len(e) for e in entries], dtype=np.int64)
        var = np.array([g.index[v] for v, _, _ in flat], dtype=np.int64)
        sense = np.array([s for _, s, _ in flat], dtype=np.int32)
        bound = np.array([int(b) for _, _, b in flat], dtype=np.int64)
        if not self._sense_said:                                          # (a form-4 handle carries the sense per member)
            capi.check(capi.lib().mi355x_sbb_base_set_sense(self.handle, 1 if g.problem.type == "max" else 0),
                       "mi355x_sbb_base_set_sense")
            self._sense_said = True
        hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
        capi.check(capi.lib().mi355x_sbatch_create_nodes_ragged(ctypes.byref(hm), ctypes.byref(ha), self.handle, n,
                                                                _ptr(depth), _ptr(var), _ptr(sense), _ptr(bound)),
                   "mi355x_sbatch_create_nodes_ragged")
        rows, cols = g.matrix.shape[0] + depth, g.matrix.shape[1] + depth
        acols = cols + g.n_art + np.array([sum(g.row_artificial(*r) for r in e) for e in entries], dtype=np.int64)
        big, abig = int(np.argmax(rows * cols)), int(np.argmax(rows * acols))
        return (SingleBatch(hm, n, rows[big], cols[big], ragged=True),
                SingleBatch(ha, n, rows[abig], acols[abig], ragged=True) if ha else None)

    def close(self):
        h, self.handle = self.handle, None
        if h:
            capi.lib().mi355x_sbb_base_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def readback(sb):
    """mi355x_sbatch_readback: (rhs[n, rows], objective rows[n, cols], bases[n, rows - 1]).  On a ragged batch
    (sb.ragged) mi355x_sbatch_readback_ragged, one gather and one copy as well: three lists of per-member arrays."""
    if sb.ragged:
        shapes = [sb.member_shape(q) for q in range(sb.n_lps)]
        r = np.cumsum([0] + [s["rows"] for s in shapes])
        c = np.cumsum([0] + [s["cols"] for s in shapes])
        rhs, obj = np.empty(int(r[-1]), dtype=F32), np.empty(int(c[-1]), dtype=F32)
        basis = np.empty(int(r[-1]) - sb.n_lps, dtype=np.int64)
        capi.check(capi.lib().mi355x_sbatch_readback_ragged(sb._handle, _ptr(rhs), _ptr(obj),
                                                            _ptr(basis) if basis.size else None),
                   "mi355x_sbatch_readback_ragged")
        n = range(sb.n_lps)
        return ([rhs[r[q]:r[q + 1]] for q in n], [obj[c[q]:c[q + 1]] for q in n],
                [basis[r[q] - q:r[q + 1] - q - 1] for q in n])
    rhs, obj = np.empty((sb.n_lps, sb.rows), dtype=F32), np.empty((sb.n_lps, sb.cols), dtype=F32)
    basis = np.empty((sb.n_lps, max(sb.rows - 1, 0)), dtype=np.int64)
    capi.check(capi.lib().mi355x_sbatch_readback(sb._handle, _ptr(rhs), _ptr(obj), _ptr(basis) if basis.size else None),
               "mi355x_sbatch_readback")
    return rhs, obj, basis


class LightSolution:
    """What tableau-objective-value and tableau-variable read of one solved member (src/simplex.lisp:74-107), with
    the batch it lives in: values[var] is the variable's np.float32, through simplex.tableau_variable's arithmetic
    (this object answers what that function asks of a tableau)."""
    ns = SINGLE

    def __init__(self, g, fp_tolerance, device, rhs, obj_row, basis, batch, q):
        self.g, self.fp_tolerance, self.device, self.batch, self.q = g, fp_tolerance, device, batch, q
        self.instance_problem, self.var_mapping, self.var_count = g.problem, g.mapping, len(obj_row) - 1
        self._light = (obj_row, rhs, basis)
        self.objective = tableau_objective_value(self)

    def _readback(self):
        return self._light

    def __getitem__(self, var):
        return tableau_variable(self, var)

    def tableau(self):
        """The member downloaded in full, as the solved SingleTableau of the node."""
        M, b = self.batch.download(self.q)
        return SingleTableau(self.g.problem, self.g.problem, M, b, M.shape[1] - 1, M.shape[0] - 1, self.g.mapping,
                             self.fp_tolerance, self.device)


class TableauSolution:
    """The same answers from a node's own solved SingleTableau (the root, and nodes solved one by one)."""

    def __init__(self, t, problem):
        self.t = t
        self.objective = tableau_objective_value(t)
        self._values = {v: tableau_variable(t, v) for v in problem.vars}

    def __getitem__(self, var):
        return self._values[var]

    def tableau(self):
        return self.t


#: mixed_shapes=True: the fewest nodes of a round that make a device-built ragged batch (or pair): a batch of one
#: node gains nothing, so two.  What was measured on whole searches is in DESIGN 4.6n.
RAGGED_NODES_MIN = 2


class DeviceRounds:
    """The `solve_round` of the GPU (see the module's docstring)."""

    def __init__(self, problem, fp_tolerance=1024, device=0, max_pivots=0, chunk=None, beyond_lds=False,
                 mixed_shapes=False):
        self.problem, self.fp_tolerance, self.device = problem, fp_tolerance, device
        self.max_pivots, self.chunk, self.beyond_lds = max_pivots, chunk, bool(beyond_lds)
        self.mixed_shapes = bool(mixed_shapes)
        self.ragged_batched = 0                                           # nodes solved in device-built ragged batches
        self.n_creates = self.n_create_rounds = 0                         # batches (or pairs) created; rounds that created any
        self.g = self.base = None
        self.host_built = self.one_by_one = self.declined = 0             # nodes that left the device-built route
        self.global_batched = 0                                           # nodes solved in global-form batches

    def _alone(self, tabs):
        """One node through its own SingleTableau(s)."""
        try:
            rc, _ = solve_status(tabs, max_pivots=self.max_pivots, chunk=self.chunk)
        except SolverError as e:
            return e, None, None
        if rc != capi.MI_OPTIMAL:
            return int(rc), None, None
        s = TableauSolution(tabs[1] if isinstance(tabs, list) else tabs, self.problem)
        return capi.MI_OPTIMAL, s.objective, s

    def _root(self):
        try:
            tabs = build_tableau_single(self.problem, fp_tolerance_factor=self.fp_tolerance, device=self.device)
        except SolverError as e:
            return _status_of(e), None, None
        return self._alone(tabs)

    def _batches(self, entries, form="lds"):
        """(main, art or None) for a group in that form, or None when the form does not hold the shape."""
        kw = {"form": form} if form != "lds" else {}                      # (the default: the calls as they were)
        if all(self.g.device_ok(e) for e in entries):
            try:
                return self.base.create_nodes(entries, **kw)
            except capi.Mi355xError as e:
                if e.code != capi.MI_UNSUPPORTED:
                    raise
                return None
        built = [host_tableaux(self.problem, e, self.fp_tolerance, self.device) for e in entries]
        two = isinstance(built[0], list)
        made = []
        try:
            for tabs in ([t[1] for t in built], [t[0] for t in built]) if two else (built,):
                made.append(SingleBatch.from_arrays(np.stack([t.matrix for t in tabs]),
                                                    np.stack([t.basis_columns for t in tabs]), device=self.device,
                                                    **kw))
        except capi.Mi355xError as e:
            for b in made:
                b.close()
            if e.code != capi.MI_UNSUPPORTED:
                raise
            return None
        self.host_built += len(entries)
        return made[0], (made[1] if two else None)

    def _solved(self, ks, st, main, out):
        """The members of a solved main batch into their slots: one light read-back."""
        rhs, obj, basis = readback(main)
        for q, k in enumerate(ks):
            if st[q] == capi.MI_OPTIMAL:
                s = LightSolution(self.g, self.fp_tolerance, self.device, rhs[q], obj[q], basis[q], main, q)
                out[k] = (capi.MI_OPTIMAL, s.objective, s)
            else:
                out[k] = (int(st[q]), None, None)

    def _in_chunks(self, main, art):
        is_max, f = self.problem.type == "max", self.fp_tolerance
        first = art or main
        st, _ = lists.batch_in_chunks(
            lambda cap: (False,) + (art.solve_two_phase(main, is_max, f, cap) if art else main.solve(is_max, f, cap)),
            first.rows, first.cols, self.max_pivots, self.chunk)
        if art:
            art.close()
        return st

    def _take_ragged(self, entries, groups, out):
        """mixed_shapes=True: the entries of `groups` that pass the guard and fit the LDS budget leave their (depth,
        artificial rows) groups and go as ONE device-built ragged batch (no artificial rows) and ONE ragged pair, each
        of RAGGED_NODES_MIN or more nodes, with one read-back each."""
        g, sets = self.g, ([], [])
        for (d, n_art), ks in groups.items():
            a = g.n_art + n_art
            if single_lds_bytes(g.matrix.shape[0] + d, g.matrix.shape[1] + d + a) > LDS_BUDGET:
                continue
            for k in ks:
                if g.device_ok(entries[k]) and all(abs(b) <= _I64_MAX for _, _, b in entries[k]):
                    sets[1 if a else 0].append(k)
        for ks in sets:
            if len(ks) < RAGGED_NODES_MIN:
                continue
            ks.sort()
            try:
                main, art = self.base.create_nodes_ragged([entries[k] for k in ks])
            except capi.Mi355xError as e:                                 # declined all the same: the groups keep them
                if e.code != capi.MI_UNSUPPORTED:
                    raise
                continue
            taken = set(ks)
            for key in list(groups):
                groups[key] = [k for k in groups[key] if k not in taken]
                if not groups[key]:
                    del groups[key]
            self.n_creates += 1
            self.ragged_batched += len(ks)
            self._solved(ks, self._in_chunks(main, art), main, out)

    def __call__(self, entries):
        out = [None] * len(entries)
        groups = {}
        created = self.n_creates
        for k, e in enumerate(entries):
            if not e:
                out[k] = self._root()
                continue
            if self.base is None:
                self.g = GeneralFormSingle(self.problem)
                self.base = Base(self.g, self.device)
            groups.setdefault((len(e), sum(self.g.row_artificial(*r) for r in e)), []).append(k)
        f = self.fp_tolerance
        if self.mixed_shapes and groups:
            self._take_ragged(entries, groups, out)
        for (d, n_art), ks in groups.items():
            try:
                made = self._batches([entries[k] for k in ks])
                # beyond the LDS budget, opt-in: ONE global-form batch (or pair) when the group is large enough
                if made is None and self.beyond_lds and len(ks) >= global_batch_min_members(
                        self.g.matrix.shape[0] + d, self.g.matrix.shape[1] + d + self.g.n_art + n_art):
                    made = self._batches([entries[k] for k in ks], form="global")
                    if made is not None:
                        self.global_batched += len(ks)
            except SolverError as e:                                      # a bound the batch declines
                for k in ks:
                    out[k] = (e, None, None)
                self.declined += len(ks)
                continue
            if made is None:                                              # beyond the LDS budget: node by node
                self.one_by_one += len(ks)
                for k in ks:
                    out[k] = self._alone(host_tableaux(self.problem, entries[k], f, self.device))
                continue
            main, art = made
            self.n_creates += 1
            self._solved(ks, self._in_chunks(main, art), main, out)
        self.n_create_rounds += self.n_creates > created
        return out


class SingleBranchAndBound:
    """One single-float search on the GPU: run() -> the incumbent's solved SingleTableau, or raises the reference's
    errors; trace() / stats() as ExactBranchAndBound, `result.objectives` the trace's objectives as np.float32."""

    def __init__(self, problem, width=1, fp_tolerance=1024, int_tolerance=0, device=0, max_pivots=0, max_nodes=0,
                 chunk=None, beyond_lds=False, mixed_shapes=False):
        self.problem, self.width, self.max_nodes, self.int_tolerance = problem, int(width), int(max_nodes), int_tolerance
        self.rounds = DeviceRounds(problem, fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots, chunk=chunk,
                                   **({"beyond_lds": True} if beyond_lds else {}),
                                   **({"mixed_shapes": True} if mixed_shapes else {}))
        self.result = None

    def run(self):
        from .simplex import _raise_for
        if self.width < 1:
            raise ValueError("bb_width must be >= 1")
        r = self.result = search(self.problem, self.rounds, self.width, self.max_nodes,
                                 fractional=fractional(self.int_tolerance), floor=floor, ceil=ceil)
        if self.rounds.base is not None:
            self.rounds.base.close()
        if isinstance(r.status, Exception):
            raise r.status
        if r.status == capi.MI_MAX_PIVOTS and self.max_nodes and len(r.trace) >= self.max_nodes:
            raise SolverError("node cap reached (max_nodes=%d)" % self.max_nodes)
        _raise_for(r.status)
        return r.values.tableau()

    def trace(self):
        return list(self.result.trace)

    def stats(self):
        return dict(self.result.stats(), declined=self.rounds.declined, host_built=self.rounds.host_built,
                    one_by_one=self.rounds.one_by_one, global_batched=self.rounds.global_batched,
                    ragged_batched=self.rounds.ragged_batched)


def solve_branch_and_bound_single(problem, width=1, fp_tolerance=1024, int_tolerance=0, device=0, max_pivots=0,
                                  max_nodes=0, chunk=None, beyond_lds=False, mixed_shapes=False):
    """simplex-solver with integer variables (src/simplex.lisp:506-542) on a problem of integers and single-floats:
    the incumbent as a solved SingleTableau (its read-back in np.float32).  beyond_lds=True (opt-in): a node group
    the LDS batches decline that has at least single.global_batch_min_members nodes goes as ONE global-form batch or
    pair instead of node by node; the search is the same, bit for bit.  mixed_shapes=True (opt-in): the nodes of a
    round are not grouped by depth and artificial rows -- those that pass the guard and fit the LDS budget go as ONE
    device-built ragged batch and ONE ragged pair (two or more nodes each); the search is the same, bit for bit."""
    return SingleBranchAndBound(problem, width, fp_tolerance, int_tolerance, device, max_pivots, max_nodes, chunk,
                                beyond_lds, mixed_shapes).run()
