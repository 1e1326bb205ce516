"""Exact rational solves (opt-in: ``mi355x_simplex_solver(problem, exact=True)``).

The reference solves a problem whose numbers are all rational in exact arithmetic: fp=, fp< and
fp> dispatch on `rational` to =, < and > (src/utils.lisp:84-124) and its tableau holds ratios.  Here
build-tableau runs on Fractions (simplex.build_tableau(exact=True)) and the tableau crosses the
boundary as numerators and denominators (mi355x_xtab_create).  On the GPU it is a fraction-free
integer tableau T with one common denominator D (kernels_exact.inc); every pivot, the two-phase
hand-over and the read-back are exact, so the pivot sequence, the basis and every entry are the
reference's own.  Values are 64-bit integers, or 128-bit ones once 64 bits overflow; a problem
whose entries outgrow 128 bits is declined with unsupported-constraint-error.
"""
import ctypes
from fractions import Fraction

import numpy as np

from . import capi
from .conditions import UnsupportedConstraintError

_I64_MAX = (1 << 63) - 1


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _declined(what):
    return UnsupportedConstraintError(("exact",) + tuple(what), "mi355x-simplex")


def check(rc, where):
    """capi.check, with MI_EXACT_OVERFLOW as the condition a caller can act on (fall back to the
    reference's solver)."""
    if rc == capi.MI_EXACT_OVERFLOW:
        raise _declined(("overflow", "128 bits"))
    if rc == capi.MI_UNSUPPORTED:
        raise _declined(("start", "basis columns are not unit columns"))
    return capi.check(rc, where)


def _int128(lo, hi):
    return (int(hi) << 64) | (int(lo) & 0xFFFFFFFFFFFFFFFF)


class ExactTableau:
    """The `tableau` struct (src/simplex.lisp:48-58) with rational entries, behind an exact device
    handle.  `.matrix` is an object array of Fractions (downloaded T / D), `.basis_columns` an int64
    array; `pivot_trace()` and `bits` as for Tableau."""
    exact = True

    def __init__(self, problem, instance_problem, matrix, basis_columns, var_count, constraint_count,
                 var_mapping, device=0, min_bits=0):
        self.problem = problem
        self.instance_problem = instance_problem
        self.var_count = int(var_count)
        self.constraint_count = int(constraint_count)
        self.var_mapping = var_mapping
        self.device = device
        self.min_bits = int(min_bits)
        self.n_pivots = 0
        self.phase1 = None                 # the artificial tableau of a two-phase solve
        self._handle = None
        M = np.empty((self.constraint_count + 1, self.var_count + 1), dtype=object)
        M[:, :] = [[Fraction(x) for x in row] for row in matrix]
        self._matrix = M
        self._basis = np.ascontiguousarray(basis_columns, dtype=np.int64)
        self._stale = False

    @property
    def _h(self):
        if self._handle is None:
            num = np.empty(self._matrix.shape, dtype=np.int64)
            den = np.empty(self._matrix.shape, dtype=np.int64)
            for (i, j), x in np.ndenumerate(self._matrix):
                if abs(x.numerator) > _I64_MAX or x.denominator > _I64_MAX:
                    raise _declined(("coefficient", str(x)))
                num[i, j], den[i, j] = x.numerator, x.denominator
            h = ctypes.c_void_p()
            check(capi.lib().mi355x_xtab_create(ctypes.byref(h), num.shape[0], num.shape[1], _ptr(num), _ptr(den),
                                                _ptr(self._basis) if self._basis.size else None, self.device,
                                                self.min_bits), "mi355x_xtab_create")
            self._handle = h
        return self._handle

    def _touch(self):
        self._stale = True

    def raw(self):
        """(T as Python ints, D, basis) as the device holds them."""
        R, C = self._matrix.shape
        T = np.empty(R * C * 2, dtype=np.int64)
        D = np.empty(2, dtype=np.int64)
        b = np.empty(max(R - 1, 0), dtype=np.int64)
        check(capi.lib().mi355x_xtab_download(self._h, _ptr(T), _ptr(D), _ptr(b) if b.size else None),
              "mi355x_xtab_download")
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
    def matrix(self):
        """tableau-matrix: Fractions."""
        self._refresh()
        return self._matrix

    @property
    def basis_columns(self):
        """tableau-basis-columns."""
        self._refresh()
        return self._basis

    def _readback(self):
        M = self.matrix
        return M[-1], M[:, -1], self.basis_columns

    @property
    def is_max(self):
        return self.instance_problem.type == "max"

    @property
    def bits(self):
        """The width the device uses for this tableau: 64 or 128."""
        b = ctypes.c_int(0)
        check(capi.lib().mi355x_xtab_bits(self._h, ctypes.byref(b)), "mi355x_xtab_bits")
        return int(b.value)

    def pivot_trace(self, cap=1 << 18):
        """(entering column, row) of every pivot the solve loops made on this tableau."""
        n = ctypes.c_int64(0)
        ec = np.empty(cap, dtype=np.int64)
        cr = np.empty(cap, dtype=np.int64)
        check(capi.lib().mi355x_xtab_trace(self._h, _ptr(ec), _ptr(cr), cap, ctypes.byref(n)), "mi355x_xtab_trace")
        k = min(n.value, cap)
        return np.stack([ec[:k], cr[:k]], axis=1)

    def __del__(self):
        h = getattr(self, "_handle", None)
        self._handle = None
        if h:
            try:
                capi.lib().mi355x_xtab_destroy(h)
            except Exception:
                pass


def cancel_solve(tableau):
    """mi355x_xtab_cancel on a tableau (or both of a two-phase pair) that a solve runs on in another thread."""
    for t in (tableau if isinstance(tableau, (list, tuple)) else [tableau]):
        check(capi.lib().mi355x_xtab_cancel(t._h), "mi355x_xtab_cancel")


def n_solve_exact(tabs, max_pivots=0, chunk=None):
    """n-solve-tableau (src/simplex.lisp:399-461) on an ExactTableau or a list [art, main], in bounded
    calls (the glue's solve-in-chunks).  Returns the solved (main) tableau; raises as n_solve_tableau."""
    from .simplex import _raise_for, _solve_in_chunks
    L = capi.lib()
    n = ctypes.c_int64(0)
    if isinstance(tabs, (list, tuple)):
        art, main = tabs
        npv = (ctypes.c_int64 * 2)()
        done = [0, 0]

        def call(cap):
            rc = check(L.mi355x_xtab_solve_two_phase(art._h, main._h, int(main.is_max), int(cap), npv),
                       "mi355x_xtab_solve_two_phase")
            done[0] += int(npv[0])
            done[1] += int(npv[1])
            return rc, int(npv[0]) + int(npv[1])
        try:
            rc, _ = _solve_in_chunks(call, art.constraint_count + 1, art.var_count + 1, int(max_pivots), chunk=chunk)
        finally:
            art._touch()
            main._touch()
        main.n_pivots = tuple(done)
        main.phase1 = art
        _raise_for(rc)
        return main

    def call(cap):
        rc = check(L.mi355x_xtab_solve(tabs._h, int(tabs.is_max), int(cap), ctypes.byref(n)), "mi355x_xtab_solve")
        return rc, int(n.value)
    try:
        rc, total = _solve_in_chunks(call, tabs.constraint_count + 1, tabs.var_count + 1, int(max_pivots), chunk=chunk)
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


def solve_exact(problem, device=0, max_pivots=0, min_bits=0, chunk=None):
    """The exact route of mi355x_simplex_solver: build-tableau in Fractions, then the exact solve."""
    from .simplex import build_tableau
    tabs = build_tableau(problem, problem, device=device, exact=True, min_bits=min_bits)
    return n_solve_exact(tabs, max_pivots=max_pivots, chunk=chunk)
