"""Exact rational solves (opt-in: ``mi355x_simplex_solver(problem, exact=True)``).

The reference solves a problem whose numbers are all rational in exact arithmetic: fp=, fp< and
fp> dispatch on `rational` to =, < and > (src/utils.lisp:84-124) and its tableau holds ratios.  Here
build-tableau runs on Fractions (simplex.build_tableau(exact=True)) and the tableau crosses the
boundary as numerators and denominators (mi355x_xtab_create).  On the GPU it is a fraction-free
integer tableau T with one common denominator D (kernels_exact.inc); every pivot, the two-phase
hand-over and the read-back are exact, so the pivot sequence, the basis and every entry are the
reference's own.  Values are 64-bit integers, or 128-bit ones once 64 bits overflow; a problem
whose entries outgrow 128 bits is declined with unsupported-constraint-error -- or, with
``exact_max_bits=256`` (opt-in), solved again at 256 bits on the single-tableau path and declined
only past those.

A list of problems (``mi355x_solve_problems(problems, exact=True)``) is grouped by tableau shape and
sense; a group of two or more is one batch of exact tableaux (mi355x_xbatch_*, one workgroup per
member: kernels_exact_batch.inc), and every member comes back as the solved ExactTableau the
one-problem route returns.

``pivot_rule`` (opt-in, every exact solve): "dantzig" is the reference's choice of column and row, which has
no anti-cycling rule -- on rationals a cycle never ends; "bland" and "dantzig-bland" end on every input
(mi355x_xtab_set_pivot_rule, include/mi355x_simplex.h).
"""
import ctypes
from fractions import Fraction

import numpy as np

from . import capi, lists
from .capi import _ptr
from .conditions import UnsupportedConstraintError
from .lowering import EXACT
from .simplex import TableauStruct

_I64_MAX = (1 << 63) - 1


def _declined(what):
    return UnsupportedConstraintError(("exact",) + tuple(what), "mi355x-simplex")


PIVOT_RULES = {"dantzig": capi.MI_RULE_DANTZIG, "bland": capi.MI_RULE_BLAND, "dantzig-bland": capi.MI_RULE_DANTZIG_BLAND}


def pivot_rule_code(name):
    """MI_RULE_* of a rule's name; ValueError for any other."""
    if not isinstance(name, str) or name not in PIVOT_RULES:
        raise ValueError("pivot_rule %r: must be one of %s" % (name, ", ".join(repr(k) for k in PIVOT_RULES)))
    return PIVOT_RULES[name]


def _check_widths(min_bits, max_bits):
    """The (min_bits, max_bits) pairs mi355x_xtab_create_wide takes."""
    if max_bits not in (128, 256) or min_bits not in (0, 64, 128, 256) or min_bits > max_bits:
        raise ValueError("exact widths: min_bits %r must be 0, 64, 128 or 256 and at most max_bits %r (128 or 256)"
                         % (min_bits, max_bits))


def check(rc, where, max_bits=128):
    """capi.check, with MI_EXACT_OVERFLOW as the condition a caller can act on (fall back to the
    reference's solver); max_bits: the limit of the handle that overflowed."""
    if rc == capi.MI_EXACT_OVERFLOW:
        raise _declined(("overflow", "%d bits" % max_bits))
    if rc == capi.MI_UNSUPPORTED:
        raise _declined(("start", "basis columns are not unit columns"))
    return capi.check(rc, where)


def _int128(lo, hi):
    return (int(hi) << 64) | (int(lo) & 0xFFFFFFFFFFFFFFFF)


def _int_of_limbs(limbs):
    """Little-endian 64-bit limbs, two's complement: the top limb carries the sign."""
    v = int(limbs[-1])
    for x in reversed(limbs[:-1]):
        v = (v << 64) | (int(x) & 0xFFFFFFFFFFFFFFFF)
    return v


def _num_den(matrix):
    """An object matrix of Fractions as the int64 numerators and denominators that cross the boundary."""
    flat = list(matrix.flat)
    for x in flat:
        if abs(x.numerator) > _I64_MAX or x.denominator > _I64_MAX:
            raise _declined(("coefficient", str(x)))
    num = np.array([x.numerator for x in flat], dtype=np.int64).reshape(matrix.shape)
    den = np.array([x.denominator for x in flat], dtype=np.int64).reshape(matrix.shape)
    return num, den


class ExactTableau(TableauStruct):
    """The `tableau` struct (src/simplex.lisp:48-58) with rational entries, behind an exact device
    handle.  `.matrix` is an object array of Fractions (downloaded T / D), `.basis_columns` an int64
    array; `pivot_trace()` and `bits` as for Tableau."""
    exact = True
    ns, _entry = EXACT, "xtab"
    pivot_rule = "dantzig"                 # set_pivot_rule; the handle gets it when it is made

    def __init__(self, problem, instance_problem, matrix, basis_columns, var_count, constraint_count,
                 var_mapping, device=0, min_bits=0, max_bits=128, pivot_rule="dantzig"):
        self._struct(problem, instance_problem, var_count, constraint_count, var_mapping, device)
        self.min_bits = int(min_bits)
        self.max_bits = int(max_bits)            # the widest width its solves may escalate to: 128 or 256
        _check_widths(self.min_bits, self.max_bits)
        pivot_rule_code(pivot_rule)
        self.pivot_rule = pivot_rule
        self.n_pivots = 0
        self.phase1 = None                 # the artificial tableau of a two-phase solve
        self._handle = None
        self._batch = None                 # (XBatch, member index): a member solved in a batch
        M = np.empty((self.constraint_count + 1, self.var_count + 1), dtype=object)
        M[:, :] = [[x if type(x) is Fraction else Fraction(x) for x in row] for row in matrix]
        self._matrix = M
        self._basis = np.ascontiguousarray(basis_columns, dtype=np.int64)
        self._stale = False

    @property
    def _h(self):
        if self._handle is None:
            num, den = _num_den(self._matrix)
            h = ctypes.c_void_p()
            basis = _ptr(self._basis) if self._basis.size else None
            if self.max_bits == 128:
                rc = capi.lib().mi355x_xtab_create(ctypes.byref(h), num.shape[0], num.shape[1], _ptr(num), _ptr(den),
                                                   basis, self.device, self.min_bits)
            else:
                rc = capi.lib().mi355x_xtab_create_wide(ctypes.byref(h), num.shape[0], num.shape[1], _ptr(num),
                                                        _ptr(den), basis, self.device, self.min_bits, self.max_bits)
            check(rc, "mi355x_xtab_create", self.max_bits)
            self._handle = h
            if self.pivot_rule != "dantzig":
                capi.check(capi.lib().mi355x_xtab_set_pivot_rule(h, pivot_rule_code(self.pivot_rule)),
                           "mi355x_xtab_set_pivot_rule")
        return self._handle

    def set_pivot_rule(self, name):
        """mi355x_xtab_set_pivot_rule: before the tableau's first pivot (both tableaux of a two-phase pair)."""
        code = pivot_rule_code(name)
        if self._handle is not None:
            capi.check(capi.lib().mi355x_xtab_set_pivot_rule(self._handle, code), "mi355x_xtab_set_pivot_rule")
        self.pivot_rule = name

    def raw(self):
        """(T as Python ints, D, basis) as the device holds them."""
        R, C = self._matrix.shape
        b = np.empty(max(R - 1, 0), dtype=np.int64)
        if not self._batch and self.bits == 256:
            T = np.empty(R * C * 4, dtype=np.int64)
            D = np.empty(4, dtype=np.int64)
            check(capi.lib().mi355x_xtab_download_limbs(self._h, 4, _ptr(T), _ptr(D), _ptr(b) if b.size else None),
                  "mi355x_xtab_download_limbs", self.max_bits)
            vals = [_int_of_limbs(T[4 * k:4 * k + 4]) for k in range(R * C)]
            return np.array(vals, dtype=object).reshape(R, C), _int_of_limbs(D), b
        T = np.empty(R * C * 2, dtype=np.int64)
        D = np.empty(2, dtype=np.int64)
        if self._batch:
            xb, q = self._batch
            check(capi.lib().mi355x_xbatch_download(xb.handle, q, _ptr(T), _ptr(D), _ptr(b) if b.size else None),
                  "mi355x_xbatch_download")
        else:
            check(capi.lib().mi355x_xtab_download(self._h, _ptr(T), _ptr(D), _ptr(b) if b.size else None),
                  "mi355x_xtab_download", self.max_bits)
        vals = [_int128(T[2 * k], T[2 * k + 1]) for k in range(R * C)]
        return np.array(vals, dtype=object).reshape(R, C), _int128(D[0], D[1]), b

    def _refresh(self):
        if self._stale:
            T, D, b = self.raw()
            M = np.empty(T.shape, dtype=object)
            for (i, j), x in np.ndenumerate(T):
                M[i, j] = Fraction(x, D)
            self._matrix, self._basis, self._stale = M, b, False

    @property
    def bits(self):
        """The width the device uses for this tableau: 64, 128 or 256."""
        b = ctypes.c_int(0)
        if self._batch:
            check(capi.lib().mi355x_xbatch_bits(self._batch[0].handle, self._batch[1], ctypes.byref(b)), "mi355x_xbatch_bits")
            return int(b.value)
        check(capi.lib().mi355x_xtab_bits(self._h, ctypes.byref(b)), "mi355x_xtab_bits")
        return int(b.value)

    def pivot_trace(self, cap=1 << 18):
        """(entering column, row) of every pivot the solve loops made on this tableau (a member solved in
        a batch: the first capi.XBATCH_TRACE_CAP of them)."""
        n = ctypes.c_int64(0)
        if self._batch:
            cap = min(cap, capi.XBATCH_TRACE_CAP)
        ec = np.empty(cap, dtype=np.int64)
        cr = np.empty(cap, dtype=np.int64)
        if self._batch:
            check(capi.lib().mi355x_xbatch_trace(self._batch[0].handle, self._batch[1], _ptr(ec), _ptr(cr), cap,
                                                 ctypes.byref(n)), "mi355x_xbatch_trace")
        else:
            check(capi.lib().mi355x_xtab_trace(self._h, _ptr(ec), _ptr(cr), cap, ctypes.byref(n)), "mi355x_xtab_trace")
        k = min(n.value, cap)
        return np.stack([ec[:k], cr[:k]], axis=1)


def cancel_solve(tableau):
    """mi355x_xtab_cancel on a tableau (or both of a two-phase pair) that a solve runs on in another thread."""
    for t in (tableau if isinstance(tableau, (list, tuple)) else [tableau]):
        check(capi.lib().mi355x_xtab_cancel(t._h), "mi355x_xtab_cancel")


def n_solve_exact(tabs, max_pivots=0, chunk=None, pivot_rule=None):
    """n-solve-tableau (src/simplex.lisp:399-461) on an ExactTableau or a list [art, main], in bounded
    calls (the glue's solve-in-chunks).  Returns the solved (main) tableau; raises as n_solve_tableau.
    pivot_rule: set on the tableau (on both of a pair) first; None leaves them as they are."""
    from .simplex import _raise_for
    if pivot_rule is not None:
        for t in (tabs if isinstance(tabs, (list, tuple)) else [tabs]):
            t.set_pivot_rule(pivot_rule)
    L = capi.lib()
    n = ctypes.c_int64(0)
    if isinstance(tabs, (list, tuple)):
        art, main = tabs
        npv = (ctypes.c_int64 * 2)()
        done = [0, 0]

        def call(cap):
            rc = check(L.mi355x_xtab_solve_two_phase(art._h, main._h, int(main.is_max), int(cap), npv),
                       "mi355x_xtab_solve_two_phase", art.max_bits)
            done[0] += int(npv[0])
            done[1] += int(npv[1])
            return rc, int(npv[0]) + int(npv[1])
        try:
            rc, _ = lists.solve_in_chunks(call, art.constraint_count + 1, art.var_count + 1, int(max_pivots), chunk=chunk)
        finally:
            art._touch()
            main._touch()
        main.n_pivots = tuple(done)
        main.phase1 = art
        _raise_for(rc)
        return main

    def call(cap):
        rc = check(L.mi355x_xtab_solve(tabs._h, int(tabs.is_max), int(cap), ctypes.byref(n)), "mi355x_xtab_solve",
                   tabs.max_bits)
        return rc, int(n.value)
    try:
        rc, total = lists.solve_in_chunks(call, tabs.constraint_count + 1, tabs.var_count + 1, int(max_pivots), chunk=chunk)
    finally:
        tabs._touch()
    tabs.n_pivots = total
    _raise_for(rc)
    return tabs


def rational_number(x):
    """An exact number of the reference's `rational` type: an int (not a bool) or a Fraction."""
    return (isinstance(x, int) and not isinstance(x, bool)) or isinstance(x, Fraction)


def rational_problem(problem):
    """Every number of the problem is rational (no float anywhere)."""
    ok = all(rational_number(c) for _, c in problem.objective_func)
    ok = ok and all((lb is None or rational_number(lb)) and (ub is None or rational_number(ub))
                    for _, (lb, ub) in problem.var_bounds)
    return ok and all(all(rational_number(c) for _, c in e) and rational_number(rhs)
                      for _, e, rhs in problem.constraints)


def solve_exact(problem, device=0, max_pivots=0, min_bits=0, chunk=None, exact_max_bits=128, pivot_rule="dantzig"):
    """The exact route of mi355x_simplex_solver: build-tableau in Fractions, then the exact solve
    (exact_max_bits: 128, or 256 to let it escalate to 256-bit tableaux; pivot_rule: the module's docstring)."""
    from .simplex import build_tableau
    pivot_rule_code(pivot_rule)
    tabs = build_tableau(problem, problem, device=device, exact=True, min_bits=min_bits, max_bits=exact_max_bits)
    return n_solve_exact(tabs, max_pivots=max_pivots, chunk=chunk, pivot_rule=pivot_rule)


# ------------------------------------------------------------------ many problems at once
class XBatch:
    """A mi355x_xbatch handle: the start tableaux of `tabs` (ExactTableaus of one shape) back to back.
    Members solved in it keep it alive; the last one to go destroys it."""

    def __init__(self, tabs, device=0, min_bits=0, pivot_rule="dantzig"):
        pivot_rule_code(pivot_rule)
        self.handle = None
        self.n_lps = len(tabs)
        self.rows, self.cols = tabs[0]._matrix.shape
        pairs = [_num_den(t._matrix) for t in tabs]
        num = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
        den = np.ascontiguousarray(np.stack([p[1] for p in pairs]))
        basis = np.ascontiguousarray(np.stack([t._basis for t in tabs]), dtype=np.int64)
        self._create(num, den, basis, device, min_bits)
        self.set_pivot_rule(pivot_rule)

    @classmethod
    def from_states(cls, num, den, basis, device=0, min_bits=0, pivot_rule="dantzig"):
        """A batch of start states given as arrays: numerators and denominators (n x rows x cols, int64)
        and the bases (n x (rows - 1))."""
        pivot_rule_code(pivot_rule)
        xb = cls.__new__(cls)
        xb.handle = None
        num = np.ascontiguousarray(num, dtype=np.int64)
        xb.n_lps, xb.rows, xb.cols = num.shape
        xb._create(num, np.ascontiguousarray(den, dtype=np.int64), np.ascontiguousarray(basis, dtype=np.int64),
                   device, min_bits)
        xb.set_pivot_rule(pivot_rule)
        return xb

    @classmethod
    def from_handle(cls, handle, n_lps, rows, cols, pivot_rule="dantzig"):
        """A batch the library made itself (mi355x_xbatch_create_nodes)."""
        xb = cls.__new__(cls)
        xb.handle, xb.n_lps, xb.rows, xb.cols = handle, int(n_lps), int(rows), int(cols)
        xb.set_pivot_rule(pivot_rule)
        return xb

    pivot_rule = "dantzig"

    def set_pivot_rule(self, name):
        """mi355x_xbatch_set_pivot_rule: before the batch's first pivot (both batches of a two-phase pair)."""
        code = pivot_rule_code(name)
        if code != capi.MI_RULE_DANTZIG or self.pivot_rule != "dantzig":
            capi.check(capi.lib().mi355x_xbatch_set_pivot_rule(self.handle, code), "mi355x_xbatch_set_pivot_rule")
        self.pivot_rule = name

    def _create(self, num, den, basis, device, min_bits):
        h = ctypes.c_void_p()
        rc = capi.lib().mi355x_xbatch_create(ctypes.byref(h), self.n_lps, self.rows, self.cols, _ptr(num), _ptr(den),
                                             _ptr(basis) if basis.size else None, device, int(min_bits))
        if rc == capi.MI_UNSUPPORTED:
            raise _declined(("batch", "shape", self.rows, self.cols))
        capi.check(rc, "mi355x_xbatch_create")
        self.handle = h

    def solve(self, is_max, max_pivots=0):
        """mi355x_xbatch_solve: (call status, per-member statuses, pivots of this call)."""
        st = np.empty(self.n_lps, dtype=np.int32)
        npv = np.zeros(self.n_lps, dtype=np.int64)
        rc = capi.check(capi.lib().mi355x_xbatch_solve(self.handle, int(is_max), int(max_pivots), _ptr(st), _ptr(npv)),
                        "mi355x_xbatch_solve")
        return rc, st, npv

    def solve_two_phase(self, main, main_is_max, max_pivots=0):
        """mi355x_xbatch_solve_two_phase with self as the artificial batch: (call status, statuses,
        pivots of this call as an (n, 2) array)."""
        st = np.empty(self.n_lps, dtype=np.int32)
        npv = np.zeros((self.n_lps, 2), dtype=np.int64)
        rc = capi.check(capi.lib().mi355x_xbatch_solve_two_phase(self.handle, main.handle, int(main_is_max),
                                                                 int(max_pivots), _ptr(st), _ptr(npv)),
                        "mi355x_xbatch_solve_two_phase")
        return rc, st, npv

    def cancel(self):
        capi.check(capi.lib().mi355x_xbatch_cancel(self.handle), "mi355x_xbatch_cancel")

    def close(self):
        h, self.handle = self.handle, None
        if h:
            capi.lib().mi355x_xbatch_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def overflowed_128(result):
    """A member's result is the condition a batch (or a 128-bit handle) declines an overflow with."""
    return isinstance(result, UnsupportedConstraintError) and tuple(result.constraint) == ("exact", "overflow", "128 bits")


def group_exact_problems(problems, device=0, min_bits=0):
    """The grouping of mi355x_solve_problems(exact=True), host only.  Returns (alone, groups, groups2,
    failed): `alone` the indices that go through mi355x_simplex_solver one by one (integer members,
    members with a float anywhere, members alone in their group), `groups` {(shape, is_max): [(k, tab)]}
    the single-phase groups of two or more, `groups2` {(art shape, main shape, is_max): [(k, art, main)]}
    the two-phase ones, `failed` {k: the SolverError build-tableau raised}."""
    from .conditions import SolverError
    from .simplex import build_tableau
    alone, groups, groups2, failed = [], {}, {}, {}
    for k, p in enumerate(problems):
        if p.integer_vars or not rational_problem(p):
            alone.append(k)
            continue
        try:
            tabs = build_tableau(p, p, device=device, exact=True, min_bits=min_bits)
        except SolverError as e:                       # e.g. the unbounded no-constraint special case
            failed[k] = e
            continue
        lists.file_by_shape(groups, groups2, k, tabs)
    alone += lists.pop_singletons(groups) + lists.pop_singletons(groups2)
    return sorted(alone), groups, groups2, failed


def _member_error(st):
    """The exception of a member's final status (None: it has a solution)."""
    from .conditions import SolverError
    from .simplex import _raise_for
    try:
        check(int(st), "mi355x_xbatch_solve")
        _raise_for(int(st))
    except SolverError as e:
        return e
    return None


def batch_in_chunks(xa, xm, is_max, max_pivots=0, chunk=None):
    """A batch (xm None) or a two-phase pair of batches in bounded calls (the glue's solve-in-chunks):
    -> (final member statuses, pivots per member -- (n, 2) for a pair)."""
    def call(cap):
        rc, st, npv = xa.solve_two_phase(xm, is_max, cap) if xm else xa.solve(is_max, cap)
        return rc == capi.MI_CANCELLED, st, npv                # (a cancelled call ends the loop: cancel())
    return lists.batch_in_chunks(call, xa.rows, xa.cols, max_pivots, chunk)


def solve_exact_batch(members, is_max, device=0, max_pivots=0, min_bits=0, chunk=None, pivot_rule="dantzig"):
    """One group of mi355x_solve_problems(exact=True) in bounded calls (the glue's solve-in-chunks):
    members are ExactTableaus (single phase) or (art, main) pairs of one shape.  Returns per member the
    solved (main) tableau or the exception of its outcome; raises the declined condition when the shape
    does not fit a batch."""
    two = isinstance(members[0], (list, tuple))
    first = [m[0] for m in members] if two else list(members)
    xa = XBatch(first, device=device, min_bits=min_bits, pivot_rule=pivot_rule)
    try:
        xm = XBatch([m[1] for m in members], device=device, min_bits=min_bits, pivot_rule=pivot_rule) if two else None
    except Exception:
        xa.close()                                     # (its device memory goes at once)
        raise
    st, total = batch_in_chunks(xa, xm, is_max, max_pivots, chunk)
    out = []
    for q, m in enumerate(members):
        e = _member_error(capi.MI_CANCELLED if st[q] == capi.MI_RUNNING else st[q])
        if e is not None:
            out.append(e)
            continue
        t = m[1] if two else m
        t._batch, t._stale = (xm if two else xa, q), True
        if two:
            m[0]._batch, m[0]._stale = (xa, q), True
            t.phase1 = m[0]
        t.n_pivots = lists.member_pivots(total, q)
        out.append(t)
    return out


def solve_problems_exact(problems, fp_tolerance=1024, device=0, max_pivots=0, errorp=True, native=False, min_bits=0,
                         chunk=None, exact_max_bits=128, pivot_rule="dantzig", device_build=False):
    """mi355x_solve_problems(exact=True): see there.  pivot_rule goes to every batch and to every member solved
    alone, the 256-bit re-solve included; a member with a float declines a rule other than "dantzig".  exact_max_bits=256: the batches stay at their 64 / 128
    bits, and a member a batch declines for overflowing them is solved again, alone, on the single-tableau
    path with 256 bits allowed; its result (or its condition) takes its slot, the other members are untouched.
    device_build=True (opt-in): the members are lowered to rows of numerators and denominators and their tableaux
    built on the device (exact_lps.py); members alone in their group, members exact_lps.lower_problem does not
    take, groups the batch declines and members that end past 128 bits go through the route above, whose
    outcomes, exceptions and errorp these are."""
    from .simplex import mi355x_simplex_solver
    _check_widths(min_bits, exact_max_bits)
    if device_build:
        from .exact_lps import solve_problems_device_built
        pivot_rule_code(pivot_rule)

        def host_route(ps):
            return solve_problems_exact(ps, fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots, errorp=False,
                                        native=native, min_bits=min_bits, chunk=chunk, exact_max_bits=exact_max_bits,
                                        pivot_rule=pivot_rule)
        return lists.finish(solve_problems_device_built(problems, host_route, device=device, max_pivots=max_pivots,
                                                        min_bits=min(min_bits, 128), chunk=chunk,
                                                        pivot_rule=pivot_rule), errorp)
    rule_kw = {} if pivot_rule_code(pivot_rule) == capi.MI_RULE_DANTZIG else {"pivot_rule": pivot_rule}   # (the default: the calls as they were)
    results = [None] * len(problems)
    batch_bits = min(min_bits, 128)                    # (a batch member is at most 128 bits wide)
    ones, groups, groups2, failed = group_exact_problems(problems, device=device, min_bits=batch_bits)

    def alone(k):
        return mi355x_simplex_solver(problems[k], fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots,
                                     native=native, exact=True, exact_bits=min_bits, exact_max_bits=exact_max_bits,
                                     chunk=chunk, **rule_kw)

    def batch(ks, members, is_max):
        try:
            lists.place(results, ks, solve_exact_batch(members, is_max, device, max_pivots, batch_bits, chunk, **rule_kw))
        except UnsupportedConstraintError:              # a shape the batch declines
            lists.one_by_one(results, ks, alone)
            return
        if exact_max_bits > 128:
            lists.one_by_one(results, [k for k in ks if overflowed_128(results[k])], alone)

    lists.place(results, failed, failed.values())
    lists.one_by_one(results, ones, alone)
    for (_, is_max), members in groups.items():
        batch([k for k, _ in members], [t for _, t in members], is_max)
    for (_, _, is_max), members in groups2.items():
        batch([k for k, _, _ in members], [(a, t) for _, a, t in members], is_max)
    return lists.finish(results, errorp)
