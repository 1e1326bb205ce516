"""Single-float solves: the reference's single-float path (src/utils.lisp:84-124 with
single-float-epsilon) over the mi355x_stab_* entries of the C ABI.

Common Lisp reads ``0.5`` as a single-float, and the reference then solves in single-float arithmetic
with single-float thresholds.  ``solve_single`` / ``mi355x_simplex_solver(problem, precision="single")``
is that path: build-tableau -- lowering.py's, the one copy every precision runs -- on a number system with
Lisp's contagion (SINGLE: integers stay exact Python ints among themselves, an int becomes float32 when it
meets a float, every float operation is an explicit ``np.float32`` operation), the solve in IEEE binary32
on the GPU (kernels_single.inc), the read-back (simplex.tableau_variable and the others) in float32.

Which problems qualify: every number is an integer with |x| <= 2**24 or a float whose value a binary32
holds exactly (``np.float32``, or a Python float with ``float(np.float32(x)) == x``).  Anything else -- a
double that is not a float32 value, a Fraction, a larger integer -- is DECLINED, never rounded silently:
``UnsupportedConstraintError(("single", x), "mi355x-simplex")``.

Integer problems are declined here (``solve_single``); ``precision="single", branch_and_bound=True`` solves them
with the reference's branch-and-bound in single-float arithmetic (single_bb.py).

Known departure (stated the way the double path states its own): integer-only sub-expressions that the
reference would keep as exact ratios through a pivot are floats here from the start -- the tableau that
crosses the boundary is all float32.
"""
import ctypes

import numpy as np

from . import capi, lists
from .capi import _ptr
from .conditions import UnsupportedConstraintError
from .lowering import NumberSystem, build
from .simplex import (TableauStruct, find_entering_column, find_pivoting_row, n_pivot_row,      # noqa: F401
                      tableau_objective_value, tableau_reduced_cost, tableau_variable)

#: SBCL's single-float-epsilon = 2^-24 (1 + 2^-23)
EPSILON_SINGLE = np.float32(2.0 ** -24 * (1 + 2.0 ** -23))


def thresholds(factor=1024):
    """(pricing, ratio eligibility, phase-1 feasibility) thresholds, computed in float32 from the factor:
    (f/8) eps_s, 0 + (f/2) eps_s, f eps_s."""
    f = np.float32(factor)
    return (np.float32(np.float32(f / np.float32(8)) * EPSILON_SINGLE),
            np.float32(np.float32(0) + np.float32(np.float32(f / np.float32(2)) * EPSILON_SINGLE)),
            np.float32(f * EPSILON_SINGLE))


# ------------------------------------------------------------------ which numbers qualify
def single_number(x):
    """True when x is an integer with |x| <= 2**24 or a float whose value a binary32 holds exactly."""
    if isinstance(x, (bool, np.bool_)):
        return False
    if isinstance(x, (int, np.integer)):
        return abs(int(x)) <= 2 ** 24
    if isinstance(x, np.float32):
        return True
    if isinstance(x, (float, np.floating)):
        with np.errstate(over="ignore"):
            return float(np.float32(x)) == float(x)
    return False


def check_single_problem(problem):
    """Declines the first number of the problem that does not qualify."""
    def check(x):
        if not single_number(x):
            raise UnsupportedConstraintError(("single", x), "mi355x-simplex")
    for _, c in problem.objective_func:
        check(c)
    for _, (lb, ub) in problem.var_bounds:
        for b in (lb, ub):
            if b is not None:
                check(b)
    for _, e, rhs in problem.constraints:
        for _, c in e:
            check(c)
        check(rhs)


# ------------------------------------------------------------------ Lisp's contagion on (int | float32)
class _Lisp:
    """A qualifying number as Lisp holds it while build-tableau computes: v is an exact int or a single-float.
    The operators are Lisp's contagion: two ints stay an exact int, anything else is a float32 operation."""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v

    def __add__(self, other):
        a, b = self.v, other.v
        return _Lisp(a + b if type(a) is int and type(b) is int else np.float32(a) + np.float32(b))

    def __sub__(self, other):
        a, b = self.v, other.v
        return _Lisp(a - b if type(a) is int and type(b) is int else np.float32(a) - np.float32(b))

    def __mul__(self, other):
        a, b = self.v, other.v
        return _Lisp(a * b if type(a) is int and type(b) is int else np.float32(a) * np.float32(b))

    def __neg__(self):
        return _Lisp(-self.v)

    def __lt__(self, number):
        return self.v < number


def _read(x):
    return _Lisp(int(x) if isinstance(x, (int, np.integer)) else np.float32(x))


def _to_f32(M):
    """A finished matrix, coerced to float32 entry by entry."""
    return np.array([np.float32(x.v) for x in M.flat], dtype=np.float32).reshape(M.shape)


def _zeros(shape):
    M = np.empty(shape, dtype=object)
    M.fill(SINGLE.zero)
    return M


#: the number system of the single-float build (lowering.py) and read-back: no _Lisp leaves the build -- matrices
#: go out as float32 arrays, a mapping's offsets as the int or np.float32 they hold
SINGLE = NumberSystem(_read, _zeros, value=np.float32, offset=np.float32, matrix=_to_f32,
                      mapping=lambda d: {var: mp[:2] + tuple(x.v for x in mp[2:]) for var, mp in d.items()})


# ------------------------------------------------------------------ the tableau
class SingleTableau(TableauStruct):
    """The `tableau` struct (src/simplex.lisp:48-58) with a single-float matrix, behind a mi355x_stab; its
    read-back (simplex.tableau_variable and the others) is in np.float32."""
    ns, _entry = SINGLE, "stab"

    def __init__(self, problem, instance_problem, matrix, basis_columns, var_count, constraint_count,
                 var_mapping, fp_tolerance_factor=1024, device=0):
        matrix = np.asarray(matrix)
        if matrix.dtype != np.float32:
            raise TypeError("a SingleTableau takes a float32 matrix, not %s" % (matrix.dtype,))
        self._struct(problem, instance_problem, var_count, constraint_count, var_mapping, device,
                     np.ascontiguousarray(matrix), basis_columns)
        self.fp_tolerance_factor = fp_tolerance_factor
        self.n_pivots = 0

    @property
    def _h(self):
        """The device handle (uploads the host arrays on first use; no CPU fallback)."""
        if self._handle is None:
            h = ctypes.c_void_p()
            capi.check(capi.lib().mi355x_stab_create(
                ctypes.byref(h), self._matrix.shape[0], self._matrix.shape[1], _ptr(self._matrix),
                _ptr(self._basis) if self._basis.size else None, self.device), "mi355x_stab_create")
            self._handle = h
        return self._handle

    def _refresh(self):
        if self._stale:
            M = np.empty((self.constraint_count + 1, self.var_count + 1), dtype=np.float32)
            b = np.empty(self.constraint_count, dtype=np.int64)
            capi.check(capi.lib().mi355x_stab_download(self._h, _ptr(M), _ptr(b) if b.size else None, None, None),
                       "mi355x_stab_download")
            self._matrix, self._basis, self._stale = M, b, False

    def info(self):
        """mi355x_stab_info: {"rows", "cols", "ld", "form" (1 pair, 2 LDS), "lds_budget"}."""
        r, c, ld, budget = (ctypes.c_int64() for _ in range(4))
        form = ctypes.c_int()
        capi.check(capi.lib().mi355x_stab_info(self._h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(ld),
                                               ctypes.byref(form), ctypes.byref(budget)), "mi355x_stab_info")
        return {"rows": r.value, "cols": c.value, "ld": ld.value, "form": form.value, "lds_budget": budget.value}

    def pivot_trace(self, cap=1 << 20):
        """(entering column, row) of every pivot made on this tableau since it was uploaded."""
        n = ctypes.c_int64(0)
        capi.check(capi.lib().mi355x_stab_trace(self._h, None, None, 0, ctypes.byref(n)), "mi355x_stab_trace")
        k = min(n.value, cap)
        ec, cr = np.empty(max(k, 1), dtype=np.int64), np.empty(max(k, 1), dtype=np.int64)
        capi.check(capi.lib().mi355x_stab_trace(self._h, _ptr(ec), _ptr(cr), k, ctypes.byref(n)), "mi355x_stab_trace")
        return np.stack([ec[:k], cr[:k]], axis=1)


def set_form(form):
    """mi355x_tune_set_single_form (tests and measurement): the form handles created from now on take."""
    capi.check(capi.lib().mi355x_tune_set_single_form(int(form)), "mi355x_tune_set_single_form")


# ------------------------------------------------------------------ build-tableau (host)
def build_tableau_single(problem, fp_tolerance_factor=1024, device=0):
    """build-tableau (src/simplex.lisp:142-328) on single-float input: a SingleTableau, or [art, main] when
    the trivial basis is infeasible.  The steps are lowering.py's, the ones every precision takes, with the
    numbers combined the way Lisp's contagion does (SINGLE; module docstring); the finished matrices are
    coerced to float32 entry by entry."""
    check_single_problem(problem)

    def make(inst, M, basis, mapping):
        return SingleTableau(problem, inst, M, basis, M.shape[1] - 1, M.shape[0] - 1, mapping, fp_tolerance_factor,
                             device)
    return build(problem, problem, SINGLE, make)


def solve_status(tableau, max_pivots=0, chunk=None):
    """n-solve-tableau (src/simplex.lisp:399-461) in bounded foreign calls, without raising: a SingleTableau or
    [art, main] -> (status, pivots); pivots is a number, or (phase 1 + drive-outs, phase 2) for a pair.
    max_pivots (0: none) caps the pivots, for a pair both phases together; chunk: pivots per foreign call."""
    L = capi.lib()
    if isinstance(tableau, (list, tuple)):
        art, main = tableau
        npv = (ctypes.c_int64 * 2)()
        done = [0, 0]

        def call(cap):
            rc = capi.check(L.mi355x_stab_solve_two_phase(art._h, main._h, int(main.is_max),
                                                          float(main.fp_tolerance_factor), int(cap), npv),
                            "mi355x_stab_solve_two_phase")
            done[0] += int(npv[0])
            done[1] += int(npv[1])
            return rc, int(npv[0]) + int(npv[1])
        try:
            rc, _ = lists.solve_in_chunks(call, art.constraint_count + 1, art.var_count + 1, max_pivots, chunk)
            main.n_pivots = tuple(done)
            return rc, main.n_pivots
        finally:
            art._touch()
            main._touch()
    if not isinstance(tableau, SingleTableau):                # (check-type tableau tableau) :454
        raise TypeError("%r is not a single-float tableau" % (tableau,))
    n = ctypes.c_int64(0)

    def call(cap):
        rc = capi.check(L.mi355x_stab_solve(tableau._h, int(tableau.is_max), float(tableau.fp_tolerance_factor),
                                            int(cap), ctypes.byref(n)), "mi355x_stab_solve")
        return rc, int(n.value)
    try:
        rc, tableau.n_pivots = lists.solve_in_chunks(call, tableau.constraint_count + 1, tableau.var_count + 1,
                                                     max_pivots, chunk)
        return rc, tableau.n_pivots
    finally:
        tableau._touch()


def n_solve_tableau(tableau, max_pivots=0, chunk=None):
    """solve_status with the reference's conditions raised; returns the solved (main) tableau."""
    from .simplex import _raise_for
    rc, _ = solve_status(tableau, max_pivots=max_pivots, chunk=chunk)
    _raise_for(rc)
    return tableau[1] if isinstance(tableau, (list, tuple)) else tableau


def solve_single(problem, fp_tolerance=1024, device=0, max_pivots=0, chunk=None):
    """What mi355x_simplex_solver(problem, precision="single") returns: the solved SingleTableau.  An integer
    problem is declined here; single_bb.py solves it (precision="single", branch_and_bound=True)."""
    if problem.integer_vars:
        raise UnsupportedConstraintError(("integer",) + tuple(problem.integer_vars), "mi355x-simplex")
    tabs = build_tableau_single(problem, fp_tolerance_factor=fp_tolerance, device=device)
    return n_solve_tableau(tabs, max_pivots=max_pivots, chunk=chunk)


# ------------------------------------------------------------------ batches: one workgroup per LP
class SingleBatch:
    """n single-float tableaux of one shape behind a mi355x_sbatch: one workgroup owns one member for its whole
    solve, the member's tableau in LDS (form "lds") or, opt-in and for members beyond the LDS budget, left in device
    memory (form "global").  Member by member the result is what the member's own SingleTableau gives under the same
    sequence of calls."""

    def __init__(self, handle, n_lps, rows, cols, ragged=False):
        self._handle, self.n_lps, self.rows, self.cols = handle, int(n_lps), int(rows), int(cols)
        #: a ragged batch (from_ragged): every member its own shape and sense; rows, cols: the largest member's
        self.ragged = bool(ragged)

    @classmethod
    def from_arrays(cls, matrices, basis, device=0, form="lds"):
        """matrices[n, rows, cols] float32, basis[n, rows - 1].  A shape the batch declines (beyond the LDS
        budget) raises capi.Mi355xError with code MI_UNSUPPORTED.  form="global": mi355x_sbatch_create_global, which
        takes every shape whose pivot row and column snapshot fit the budget."""
        if form not in ("lds", "global"):
            raise ValueError("form=%r: \"lds\" (default) or \"global\"" % (form,))
        M = np.asarray(matrices)
        if M.dtype != np.float32:
            raise TypeError("a SingleBatch takes float32 matrices, not %s" % (M.dtype,))
        if M.ndim != 3:
            raise ValueError("matrices must be [n, rows, cols], not %r" % (M.shape,))
        M = np.ascontiguousarray(M)
        n, rows, cols = M.shape
        b = np.ascontiguousarray(basis, dtype=np.int64)
        if b.shape != (n, rows - 1):
            raise ValueError("basis shape %r does not match [n, rows - 1] = %r" % (b.shape, (n, rows - 1)))
        h = ctypes.c_void_p()
        name = "mi355x_sbatch_create_global" if form == "global" else "mi355x_sbatch_create"
        capi.check(getattr(capi.lib(), name)(ctypes.byref(h), n, rows, cols, _ptr(M), _ptr(b) if b.size else None,
                                             int(device)), name)
        return cls(h, n, rows, cols)

    @classmethod
    def from_lps(cls, lps, sense, col_int_sum=None, device=0, form="lds"):
        """mi355x_sbatch_create_lps: the members' tableaux built on the device from their rows.  lps[n, m + 1,
        ncv + 1] float32 in column space (per member m rows of coefficients and the right-hand side, then the
        objective row), sense[n, m] (0 `<=`, 1 `>=`, 2 `=`), col_int_sum[n, ncv + 1] or None: per member and column
        the sum of the absolute values of the entries Lisp holds as integers (the guard).  Every member has the same
        numbers of `=` and of artificial rows.  -> (main, art or None).  A group the library declines (the guard,
        the LDS budget) raises capi.Mi355xError with code MI_UNSUPPORTED.  form="global":
        mi355x_sbatch_create_lps_global, the same tableaux as members of global-form batches -- every shape whose
        pivot row and column snapshot fit the budget, any number of rows."""
        if form not in ("lds", "global"):
            raise ValueError("form=%r: \"lds\" (default) or \"global\"" % (form,))
        L = np.asarray(lps)
        if L.dtype != np.float32:
            raise TypeError("SingleBatch.from_lps takes float32 rows, not %s" % (L.dtype,))
        if L.ndim != 3:
            raise ValueError("lps must be [n, m + 1, ncv + 1], not %r" % (L.shape,))
        L = np.ascontiguousarray(L)
        n, m, ncv = L.shape[0], L.shape[1] - 1, L.shape[2] - 1
        s = np.ascontiguousarray(sense, dtype=np.int32)
        if s.shape != (n, m):
            raise ValueError("sense shape %r does not match [n, m] = %r" % (s.shape, (n, m)))
        sums = None
        if col_int_sum is not None:
            sums = np.ascontiguousarray(col_int_sum, dtype=np.float64)
            if sums.shape != (n, ncv + 1):
                raise ValueError("col_int_sum shape %r does not match [n, ncv + 1] = %r" % (sums.shape, (n, ncv + 1)))
        hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
        name = "mi355x_sbatch_create_lps_global" if form == "global" else "mi355x_sbatch_create_lps"
        capi.check(getattr(capi.lib(), name)(ctypes.byref(hm), ctypes.byref(ha), n, m, ncv, _ptr(L), _ptr(s),
                                             _ptr(sums) if sums is not None else None, int(device)), name)
        n_eq, n_art = (int(x[0]) for x in lists.row_counts(L[:1, :-1, -1] < 0, s[:1]))
        cols = ncv + (m - n_eq) + 1
        return cls(hm, n, m + 1, cols), (cls(ha, n, m + 1, cols + n_art) if ha else None)

    @classmethod
    def from_ragged(cls, matrices, bases, is_max, device=0):
        """mi355x_sbatch_create_ragged: ONE batch of members of different shapes and senses.  matrices: a list of
        float32 arrays [rows_q, cols_q]; bases: a list of int64 arrays [rows_q - 1]; is_max: a list of truth values,
        or None when every member is a `min` problem (the artificial batch of a pair).  A member beyond the LDS budget
        raises capi.Mi355xError with code MI_UNSUPPORTED; the message names the member."""
        Ms = [np.asarray(M) for M in matrices]
        if not Ms:
            raise ValueError("a ragged batch needs at least one member")
        if len(bases) != len(Ms):
            raise ValueError("%d bases for %d matrices" % (len(bases), len(Ms)))
        if is_max is not None and len(is_max) != len(Ms):
            raise ValueError("%d senses for %d matrices" % (len(is_max), len(Ms)))
        bs = []
        for q, (M, b) in enumerate(zip(Ms, bases)):
            if M.dtype != np.float32:
                raise TypeError("a SingleBatch takes float32 matrices, not %s (member %d)" % (M.dtype, q))
            if M.ndim != 2 or M.shape[0] < 1 or M.shape[1] < 2:
                raise ValueError("member %d must be [rows >= 1, cols >= 2], not %r" % (q, M.shape))
            b = np.ascontiguousarray(b, dtype=np.int64)
            if b.shape != (M.shape[0] - 1,):
                raise ValueError("member %d: basis shape %r does not match [rows - 1] = %r" % (q, b.shape, (M.shape[0] - 1,)))
            bs.append(b)
        rows = np.array([M.shape[0] for M in Ms], dtype=np.int64)
        cols = np.array([M.shape[1] for M in Ms], dtype=np.int64)
        flat = np.concatenate([np.ascontiguousarray(M).ravel() for M in Ms])
        basis = np.concatenate(bs)
        sense = None if is_max is None else np.array([1 if x else 0 for x in is_max], dtype=np.int32)
        h = ctypes.c_void_p()
        capi.check(capi.lib().mi355x_sbatch_create_ragged(
            ctypes.byref(h), len(Ms), _ptr(rows), _ptr(cols), _ptr(sense) if sense is not None else None, _ptr(flat),
            _ptr(basis) if basis.size else None, int(device)), "mi355x_sbatch_create_ragged")
        big = int(np.argmax(rows * cols))
        return cls(h, len(Ms), rows[big], cols[big], ragged=True)

    @classmethod
    def from_lps_ragged(cls, lps_list, sense_list, is_max, col_int_sum_list=None, device=0):
        """mi355x_sbatch_create_lps_ragged: ONE ragged batch (or pair) whose tableaux the device builds from the
        members' rows -- from_lps with a shape and a sense per member.  lps_list: float32 arrays [m_q + 1, ncv_q + 1] in
        column space; sense_list: arrays [m_q] (0 `<=`, 1 `>=`, 2 `=`); is_max: a truth value per member;
        col_int_sum_list: arrays [ncv_q + 1] or None (the guard).  Either no member has artificial rows or every
        member has at least one (the counts may differ): a mixture is declined with MI_BAD_ARG, the caller splits its
        list.  -> (main, art or None), both ragged.  The guard and a member beyond the LDS budget (a two-phase member:
        its artificial shape) raise capi.Mi355xError with code MI_UNSUPPORTED; the message names the member."""
        Ls = [np.asarray(L) for L in lps_list]
        if not Ls:
            raise ValueError("a ragged batch needs at least one member")
        if len(sense_list) != len(Ls):
            raise ValueError("%d sense arrays for %d members" % (len(sense_list), len(Ls)))
        if len(is_max) != len(Ls):
            raise ValueError("%d senses for %d members" % (len(is_max), len(Ls)))
        if col_int_sum_list is not None and len(col_int_sum_list) != len(Ls):
            raise ValueError("%d col_int_sum arrays for %d members" % (len(col_int_sum_list), len(Ls)))
        ss, sums = [], []
        for q, L in enumerate(Ls):
            if L.dtype != np.float32:
                raise TypeError("SingleBatch.from_lps_ragged takes float32 rows, not %s (member %d)" % (L.dtype, q))
            if L.ndim != 2 or L.shape[0] < 2 or L.shape[1] < 2:
                raise ValueError("member %d must be [m + 1 >= 2, ncv + 1 >= 2], not %r" % (q, L.shape))
            s = np.ascontiguousarray(sense_list[q], dtype=np.int32)
            if s.shape != (L.shape[0] - 1,):
                raise ValueError("member %d: sense shape %r does not match [m] = %r" % (q, s.shape, (L.shape[0] - 1,)))
            ss.append(s)
            if col_int_sum_list is not None:
                c = np.ascontiguousarray(col_int_sum_list[q], dtype=np.float64)
                if c.shape != (L.shape[1],):
                    raise ValueError("member %d: col_int_sum shape %r does not match [ncv + 1] = %r"
                                     % (q, c.shape, (L.shape[1],)))
                sums.append(c)
        m = np.array([L.shape[0] - 1 for L in Ls], dtype=np.int64)
        ncv = np.array([L.shape[1] - 1 for L in Ls], dtype=np.int64)
        flat = np.concatenate([np.ascontiguousarray(L).ravel() for L in Ls])
        sense = np.concatenate(ss)
        sums = np.concatenate(sums) if sums else None
        senses = np.array([1 if x else 0 for x in is_max], dtype=np.int32)
        hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
        capi.check(capi.lib().mi355x_sbatch_create_lps_ragged(
            ctypes.byref(hm), ctypes.byref(ha), len(Ls), _ptr(m), _ptr(ncv), _ptr(senses), _ptr(flat), _ptr(sense),
            _ptr(sums) if sums is not None else None, int(device)), "mi355x_sbatch_create_lps_ragged")
        counts = [lists.row_counts(L[:-1, -1] < 0, s) for L, s in zip(Ls, ss)]
        rows = m + 1
        cols = np.array([n + (k - int(e)) + 1 for n, k, (e, _) in zip(ncv, m, counts)], dtype=np.int64)
        acols = cols + np.array([int(a) for _, a in counts], dtype=np.int64)
        big, abig = int(np.argmax(rows * cols)), int(np.argmax(rows * acols))
        return (cls(hm, len(Ls), rows[big], cols[big], ragged=True),
                cls(ha, len(Ls), rows[abig], acols[abig], ragged=True) if ha else None)

    def member_shape(self, q):
        """mi355x_sbatch_member_shape: {"rows", "cols", "ld", "is_max" (1, 0; -1 on a batch of one shape: the sense is
        the call's), "occupancy_class" (workgroups resident per compute unit in the launch the member goes in)}."""
        r, c, ld = (ctypes.c_int64() for _ in range(3))
        sense, cl = ctypes.c_int32(), ctypes.c_int()
        capi.check(capi.lib().mi355x_sbatch_member_shape(self._handle, int(q), ctypes.byref(r), ctypes.byref(c),
                                                         ctypes.byref(ld), ctypes.byref(sense), ctypes.byref(cl)),
                   "mi355x_sbatch_member_shape")
        return {"rows": r.value, "cols": c.value, "ld": ld.value, "is_max": sense.value, "occupancy_class": cl.value}

    def solve(self, is_max, fp_tolerance=1024, max_pivots=0):
        """-> (status[n] int32, n_pivots[n] int64) of this call; self.last_return is what the call itself returned
        (MI_OK, or MI_CANCELLED after cancel(): the unfinished members are MI_RUNNING and the next call carries them on).
        A ragged batch passes -1 for the sense: it is each member's own."""
        st, npv = np.empty(self.n_lps, dtype=np.int32), np.empty(self.n_lps, dtype=np.int64)
        is_max = -1 if self.ragged else is_max
        rc = capi.check(capi.lib().mi355x_sbatch_solve(self._handle, int(is_max), float(fp_tolerance), int(max_pivots),
                                                       _ptr(st), _ptr(npv)), "mi355x_sbatch_solve")
        self.last_return = rc
        return st, npv

    def solve_two_phase(self, main, main_is_max, fp_tolerance=1024, max_pivots=0):
        """self: the batch of artificial tableaux.  -> (status[n], n_pivots[n, 2]: phase 1 + drive-outs, phase 2)."""
        st, npv = np.empty(self.n_lps, dtype=np.int32), np.empty((self.n_lps, 2), dtype=np.int64)
        main_is_max = -1 if main.ragged else main_is_max                    # (a ragged batch: the members' own senses)
        rc = capi.check(capi.lib().mi355x_sbatch_solve_two_phase(self._handle, main._handle, int(main_is_max),
                                                                 float(fp_tolerance), int(max_pivots), _ptr(st), _ptr(npv)),
                        "mi355x_sbatch_solve_two_phase")
        self.last_return = rc
        return st, npv

    def download(self, q):
        """Member q: (matrix float32 [rows, cols], basis int64 [rows - 1]); on a ragged batch the member's own shape."""
        rows, cols = self.rows, self.cols
        if self.ragged:
            shape = self.member_shape(q)
            rows, cols = shape["rows"], shape["cols"]
        M, b = np.empty((rows, cols), dtype=np.float32), np.empty(rows - 1, dtype=np.int64)
        capi.check(capi.lib().mi355x_sbatch_download(self._handle, int(q), _ptr(M), _ptr(b) if b.size else None, None, None),
                   "mi355x_sbatch_download")
        return M, b

    def trace(self, q):
        """(entering column, row) of member q's pivots since the batch was created."""
        n = ctypes.c_int64(0)
        capi.check(capi.lib().mi355x_sbatch_trace(self._handle, int(q), None, None, 0, ctypes.byref(n)), "mi355x_sbatch_trace")
        k = min(n.value, capi.SBATCH_TRACE_CAP)
        ec, cr = np.empty(max(k, 1), dtype=np.int64), np.empty(max(k, 1), dtype=np.int64)
        capi.check(capi.lib().mi355x_sbatch_trace(self._handle, int(q), _ptr(ec), _ptr(cr), k, ctypes.byref(n)),
                   "mi355x_sbatch_trace")
        return np.stack([ec[:k], cr[:k]], axis=1)

    def info(self):
        """mi355x_sbatch_info: {"n_lps", "rows", "cols", "ld", "workgroup_threads", "lds_bytes_per_member",
        "members_per_cu", "form" (mi355x_sbatch_form: 2 LDS, 3 global, 4 ragged: rows = cols = ld = 0, the largest
        member's LDS bytes, the smallest occupancy class)}."""
        n, r, c, ld, lds = (ctypes.c_int64() for _ in range(5))
        thr, per_cu, form = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        capi.check(capi.lib().mi355x_sbatch_info(self._handle, ctypes.byref(n), ctypes.byref(r), ctypes.byref(c),
                                                 ctypes.byref(ld), ctypes.byref(thr), ctypes.byref(lds),
                                                 ctypes.byref(per_cu)), "mi355x_sbatch_info")
        capi.check(capi.lib().mi355x_sbatch_form(self._handle, ctypes.byref(form)), "mi355x_sbatch_form")
        return {"n_lps": n.value, "rows": r.value, "cols": c.value, "ld": ld.value, "workgroup_threads": thr.value,
                "lds_bytes_per_member": lds.value, "members_per_cu": per_cu.value, "form": form.value}

    def cancel(self):
        """mi355x_sbatch_cancel: the running call, or the next one, stops between two rounds with MI_CANCELLED."""
        capi.check(capi.lib().mi355x_sbatch_cancel(self._handle), "mi355x_sbatch_cancel")

    def close(self):
        h, self._handle = self._handle, None
        if h:
            capi.lib().mi355x_sbatch_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_batch_threads(threads):
    """mi355x_tune_set_sbatch_threads (tests and measurement): 0 auto, 256 or 1024 for batches created from now on."""
    capi.check(capi.lib().mi355x_tune_set_sbatch_threads(int(threads)), "mi355x_tune_set_sbatch_threads")


def set_batch_launch_cap(cap):
    """mi355x_tune_set_sbatch_launch_cap (tests): pivots per member and launch, 0 the default."""
    capi.check(capi.lib().mi355x_tune_set_sbatch_launch_cap(int(cap)), "mi355x_tune_set_sbatch_launch_cap")


def set_batch_global_threads(threads):
    """mi355x_tune_set_sbatch_global_threads (tests and measurement): 0 auto, 256 or 1024 for global-form batches
    created from now on."""
    capi.check(capi.lib().mi355x_tune_set_sbatch_global_threads(int(threads)), "mi355x_tune_set_sbatch_global_threads")


def set_batch_ragged_classes(classes):
    """mi355x_tune_set_sbatch_ragged_classes (tests and measurement): 0 the default (one class: the measured choice),
    1 one class for all members, 4 up to four occupancy classes, for ragged batches created from now on."""
    capi.check(capi.lib().mi355x_tune_set_sbatch_ragged_classes(int(classes)), "mi355x_tune_set_sbatch_ragged_classes")


#: the LDS budget of the single-float LDS forms (kSingleLdsBudget) and a member's dynamic LDS (single_lds_bytes):
#: the stored tableau with rows of whole quads, the pivot row, the column snapshot rounded up to a quad
LDS_BUDGET = 156 * 1024


def single_lds_bytes(rows, cols):
    ldl, rp = (int(cols) + 3) // 4 * 4, (int(rows) + 3) // 4 * 4
    return (int(rows) * ldl + ldl + rp) * 4


#: tests: a number here replaces global_batch_min_members' answer for every shape
GLOBAL_BATCH_MIN_MEMBERS = None


def global_batch_min_members(rows, cols):
    """The fewest members of a rows x cols group (beyond the LDS budget) that go as ONE global-form batch under
    beyond_lds=True; a smaller group goes one by one.  One workgroup per member loses to the select / update pair,
    which puts the whole GPU on one tableau, when members are large and few: the crossover grows with the stored
    bytes.  Read off profiles/sbatch_global_rate.txt: the batch is taken only where it was measured
    faster than one by one by more than the one-by-one figure's own spread -- a shape between two measured ones
    takes the larger one's count, a member beyond the largest measured one is never batched."""
    if GLOBAL_BATCH_MIN_MEMBERS is not None:
        return int(GLOBAL_BATCH_MIN_MEMBERS)
    stored = int(rows) * ((int(cols) + 31) // 32 * 32) * 4
    for limit, members in _GLOBAL_MIN_MEMBERS:
        if stored <= limit:
            return members
    return GLOBAL_BATCH_NEVER


#: (stored bytes of a measured member, the fewest members from which the batch was faster at that shape and at every
#: larger count measured), ascending: 256 x 512 (from 2 on), 512 x 1024 (not at 2, from 8 on), 1024 x 2048
_GLOBAL_MIN_MEMBERS = ((257 * 800 * 4, 2), (513 * 1568 * 4, 8), (1025 * 3104 * 4, 64))
#: more members than a batch can have (mi355x_sbatch_create takes up to 2**30)
GLOBAL_BATCH_NEVER = 1 << 31


def group_single_problems(problems, fp_tolerance=1024, device=0):
    """Host only: check_single_problem + build_tableau_single per member.
    -> (slots, groups, groups2): slots[k] is None, "alone" (an integer problem: solve_single declines it in its own
    words) or the condition that building member k raised; groups maps (shape, is_max) to [(k, tableau)] of the
    single-phase members, groups2 maps (art shape, main shape, is_max) to [(k, art, main)] of the two-phase ones.
    There is no unit-basis restriction: the path has no compact form."""
    from .conditions import SolverError
    slots, groups, groups2 = [None] * len(problems), {}, {}
    for k, p in enumerate(problems):
        if p.integer_vars:
            slots[k] = "alone"
            continue
        try:
            check_single_problem(p)
            tabs = build_tableau_single(p, fp_tolerance_factor=fp_tolerance, device=device)
        except SolverError as e:
            slots[k] = e
            continue
        lists.file_by_shape(groups, groups2, k, tabs)
    return slots, groups, groups2


def solve_made_batches(made, is_max, take, fp_tolerance=1024, max_pivots=0, chunk=None):
    """A created group -- [main], or [art, main] for two-phase members -- in bounded chunks (lists.batch_in_chunks):
    per member take(main batch, q, n_pivots) for a solved one, or the exception of its outcome.  Closes the batches."""
    from .simplex import _error_for
    first, sb, two = made[0], made[-1], len(made) == 2
    try:
        st, npv = lists.batch_in_chunks(
            lambda cap: (False,) + (first.solve_two_phase(sb, is_max, fp_tolerance, cap) if two else
                                    sb.solve(is_max, fp_tolerance, cap)), first.rows, first.cols, max_pivots, chunk)
        out = []
        for q in range(sb.n_lps):
            e = _error_for(int(st[q]))
            out.append(take(sb, q, lists.member_pivots(npv, q)) if e is None else e)
        return out
    finally:
        for b in made:
            b.close()


#: mixed_shapes=True: a (shape, sense) group of at least this many members stays a batch of ONE shape instead of
#: joining the ragged batch; None: every member goes ragged.  Read off profiles/sbatch_ragged_rate.txt, part 1 (DESIGN
#: 4.6m): at 256 members the ragged batch is 0.999 / 0.994 / 0.986 of the uniform batch at 24 x 40 / 61 x 97 / 96 x 300,
#: and at 61 x 97 that is 0.2 % below the uniform figure's own smallest run, so groups from some count on stay uniform.
#: The count: rows of 16 to 1024 members are 0.97-1.02 and move by 1-3 % from one run of the tool to the next (61 x 97
#: at 256 was 0.985-0.994 in the last three runs), which is no more than a second batch costs -- part 2 has 16 batches
#: of one shape at 0.62 of the one ragged batch.  The one row beyond that drift, in every run, is 4096 members of
#: 24 x 40 at 0.90: groups of at least 4096 members stay batches of one shape.
RAGGED_UNIFORM_MIN_MEMBERS = 4096


def take_for_ragged(groups, art_shape=False):
    """Takes out of groups (file_by_shape's) the members that go as ONE ragged batch under mixed_shapes=True: those
    inside the LDS budget (for two-phase members: the artificial shape, the larger of the two), except the groups
    RAGGED_UNIFORM_MIN_MEMBERS keeps as batches of one shape.  -> the members in list order; fewer than two are put
    back, as a batch of one member gains nothing."""
    taken = {}
    for key, members in list(groups.items()):
        rows, cols = key[0]                                   # (shape, is_max) or (art shape, main shape, is_max)
        if single_lds_bytes(rows, cols) > LDS_BUDGET:
            continue
        if RAGGED_UNIFORM_MIN_MEMBERS is not None and len(members) >= RAGGED_UNIFORM_MIN_MEMBERS:
            continue
        taken[key] = groups.pop(key)
    if sum(len(v) for v in taken.values()) < 2:
        groups.update(taken)
        return []
    return sorted((m for v in taken.values() for m in v), key=lambda m: m[0])


def solve_problems_single(problems, fp_tolerance=1024, device=0, max_pivots=0, errorp=True, chunk=None,
                          beyond_lds=False, mixed_shapes=False):
    """mi355x_solve_problems(..., precision="single"): what [solve_single(p) for p in problems] returns, the groups
    of two or more as ONE SingleBatch (or a pair of them) in bounded chunks.  Members alone in their group, shapes
    the batch declines and integer problems go through solve_single one by one.
    beyond_lds=True (opt-in): a group the LDS batch declines that has at least global_batch_min_members(rows, cols)
    members (for two-phase members: of the artificial shape) goes as ONE global-form batch (or a pair of them)
    instead of one by one; the results are the same, bit for bit.
    mixed_shapes=True (opt-in): the members inside the LDS budget are not grouped by shape and sense -- all
    single-phase ones go as ONE ragged batch, all two-phase ones as ONE ragged pair (SingleBatch.from_ragged), two
    or more members each, in bounded chunks sized by the largest member; everything else goes as above, and the
    results are the same, bit for bit."""
    results = [None] * len(problems)
    slots, groups, groups2 = group_single_problems(problems, fp_tolerance, device)

    def alone(k):
        return solve_single(problems[k], fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots, chunk=chunk)

    def make(*members, form="lds"):
        """One SingleBatch per list of tableaux, or None when the batch declines a shape (beyond the LDS budget)."""
        made = []
        try:
            for tabs in members:
                made.append(SingleBatch.from_arrays(np.stack([t.matrix for t in tabs]),
                                                    np.stack([t.basis_columns for t in tabs]), device=device,
                                                    **({"form": form} if form != "lds" else {})))
        except capi.Mi355xError as e:
            for b in made:
                b.close()
            if e.code != capi.MI_UNSUPPORTED:
                raise
            return None
        return made

    def adopt(t, sb, q, n_pivots):
        t._matrix, t._basis = sb.download(q)
        t._stale, t._handle = False, None                     # (never uploaded: no handle left behind)
        t.n_pivots = n_pivots
        return t

    for k, s in enumerate(slots):
        if s == "alone":
            lists.one_by_one(results, [k], alone)
        elif s is not None:
            results[k] = s
    if mixed_shapes:
        for members in (take_for_ragged(groups), take_for_ragged(groups2)):
            if not members:
                continue
            ks, firsts, mains = [m[0] for m in members], [m[1] for m in members], [m[-1] for m in members]
            senses = [t.is_max for t in mains]
            made = [SingleBatch.from_ragged([t.matrix for t in mains], [t.basis_columns for t in mains], senses,
                                            device=device)]
            if len(members[0]) == 3:
                try:
                    made.insert(0, SingleBatch.from_ragged([t.matrix for t in firsts], [t.basis_columns for t in firsts],
                                                           None, device=device))
                except BaseException:
                    made[0].close()
                    raise
            lists.place(results, ks, solve_made_batches(made, -1, lambda sb, q, n, mains=mains: adopt(mains[q], sb, q, n),
                                                        fp_tolerance, max_pivots, chunk))
    # a group of two or more is one batch, or for two-phase members a batch of artificial and one of main tableaux
    for members in [*groups.values(), *groups2.values()]:
        ks, firsts, mains = [m[0] for m in members], [m[1] for m in members], [m[-1] for m in members]
        two = len(members[0]) == 3
        lists_of = (firsts, mains) if two else (mains,)
        made = make(*lists_of) if len(members) > 1 else None
        if made is None and beyond_lds and len(members) > 1 and \
                len(members) >= global_batch_min_members(*firsts[0].matrix.shape):
            made = make(*lists_of, form="global")
        if made is None:
            lists.one_by_one(results, ks, alone)
            continue
        lists.place(results, ks, solve_made_batches(made, mains[0].is_max, lambda sb, q, n: adopt(mains[q], sb, q, n),
                                                    fp_tolerance, max_pivots, chunk))
    return lists.finish(results, errorp)
