"""Single-float solves: the reference's single-float path (src/utils.lisp:84-124 with
single-float-epsilon) over the mi355x_stab_* entries of the C ABI.

Common Lisp reads ``0.5`` as a single-float, and the reference then solves in single-float arithmetic
with single-float thresholds.  ``solve_single`` / ``mi355x_simplex_solver(problem, precision="single")``
is that path: build-tableau with Lisp's contagion (integers stay exact Python ints among themselves, an
int becomes float32 when it meets a float, every float operation is an explicit ``np.float32``
operation), the solve in IEEE binary32 on the GPU (kernels_single.inc), the read-back in float32.

Which problems qualify: every number is an integer with |x| <= 2**24 or a float whose value a binary32
holds exactly (``np.float32``, or a Python float with ``float(np.float32(x)) == x``).  Anything else -- a
double that is not a float32 value, a Fraction, a larger integer -- is DECLINED, never rounded silently:
``UnsupportedConstraintError(("single", x), "mi355x-simplex")``.

Known departure (stated the way the double path states its own): integer-only sub-expressions that the
reference would keep as exact ratios through a pivot are floats here from the start -- the tableau that
crosses the boundary is all float32.
"""
import ctypes

import numpy as np

from . import capi
from .conditions import ParsingError, UnboundedProblemError, UnsupportedConstraintError
from .problem import Problem

#: SBCL's single-float-epsilon = 2^-24 (1 + 2^-23)
EPSILON_SINGLE = np.float32(2.0 ** -24 * (1 + 2.0 ** -23))


def thresholds(factor=1024):
    """(pricing, ratio eligibility, phase-1 feasibility) thresholds, computed in float32 from the factor:
    (f/8) eps_s, 0 + (f/2) eps_s, f eps_s."""
    f = np.float32(factor)
    return (np.float32(np.float32(f / np.float32(8)) * EPSILON_SINGLE),
            np.float32(np.float32(0) + np.float32(np.float32(f / np.float32(2)) * EPSILON_SINGLE)),
            np.float32(f * EPSILON_SINGLE))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


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
def _n(x):
    """A qualifying number as Lisp holds it: an exact int, or a single-float."""
    return int(x) if isinstance(x, (int, np.integer)) else np.float32(x)


def _is_int(x):
    return isinstance(x, int)


def _mul(a, b):
    return a * b if _is_int(a) and _is_int(b) else np.float32(np.float32(a) * np.float32(b))


def _add(a, b):
    return a + b if _is_int(a) and _is_int(b) else np.float32(np.float32(a) + np.float32(b))


def _sub(a, b):
    return a - b if _is_int(a) and _is_int(b) else np.float32(np.float32(a) - np.float32(b))


def _neg(a):
    return -a if _is_int(a) else np.float32(-np.float32(a))


def _to_f32(M):
    out = np.empty(M.shape, dtype=np.float32)
    for idx, x in np.ndenumerate(M):
        out[idx] = np.float32(x)
    return out


# ------------------------------------------------------------------ the tableau
class SingleTableau:
    """The `tableau` struct (src/simplex.lisp:48-58) with a single-float matrix, behind a mi355x_stab."""
    exact = False
    single = True

    def __init__(self, problem, instance_problem, matrix, basis_columns, var_count, constraint_count,
                 var_mapping, fp_tolerance_factor=1024, device=0):
        self.problem = problem
        self.instance_problem = instance_problem
        self.var_count = int(var_count)
        self.constraint_count = int(constraint_count)
        self.var_mapping = var_mapping
        self.fp_tolerance_factor = fp_tolerance_factor
        self.device = device
        matrix = np.asarray(matrix)
        if matrix.dtype != np.float32:
            raise TypeError("a SingleTableau takes a float32 matrix, not %s" % (matrix.dtype,))
        matrix = np.ascontiguousarray(matrix)
        basis = np.ascontiguousarray(basis_columns, dtype=np.int64)
        if matrix.shape != (self.constraint_count + 1, self.var_count + 1):
            raise ValueError("matrix shape %r does not match counts" % (matrix.shape,))
        if basis.shape != (self.constraint_count,):
            raise ValueError("basis length %r does not match constraint count" % (basis.shape,))
        self._matrix, self._basis, self._stale = matrix.copy(), basis.copy(), False
        self._handle = None
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

    def _touch(self):
        self._stale = True

    @property
    def matrix(self):
        """tableau-matrix (host copy, float32)."""
        self._refresh()
        return self._matrix

    @property
    def basis_columns(self):
        self._refresh()
        return self._basis

    @property
    def is_max(self):
        return self.instance_problem.type == "max"

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

    def __del__(self):
        h = getattr(self, "_handle", None)
        self._handle = None
        if h:
            try:
                capi.lib().mi355x_stab_destroy(h)
            except Exception:
                pass


def set_form(form):
    """mi355x_tune_set_single_form (tests and measurement): the form handles created from now on take."""
    capi.check(capi.lib().mi355x_tune_set_single_form(int(form)), "mi355x_tune_set_single_form")


# ------------------------------------------------------------------ read-back (host, O(n), float32)
def tableau_objective_value(tableau):
    """tableau-objective-value (src/simplex.lisp:74-78)."""
    return np.float32(tableau.matrix[tableau.constraint_count, tableau.var_count])


def _basic_value(tableau, col):
    pos = np.nonzero(tableau.basis_columns == col)[0]        # `position`: first match
    return np.float32(tableau.matrix[pos[0], tableau.var_count]) if pos.size else np.float32(0)


def tableau_variable(tableau, var):
    """tableau-variable (src/simplex.lisp:81-107) in float32, the lower-bound offset included."""
    if var == tableau.instance_problem.objective_var:
        return tableau_objective_value(tableau)
    mapping = tableau.var_mapping.get(var)
    if mapping is None:
        raise KeyError("%s is not a variable in the tableau" % (var,))
    if mapping[0] == "positive":
        return np.float32(np.float32(mapping[2]) + _basic_value(tableau, mapping[1]))
    if mapping[0] == "negative":
        return np.float32(np.float32(mapping[2]) + np.float32(-_basic_value(tableau, mapping[1])))
    return np.float32(_basic_value(tableau, mapping[1]) - _basic_value(tableau, mapping[1] + 1))


def tableau_reduced_cost(tableau, var):
    """tableau-reduced-cost (src/simplex.lisp:111-120)."""
    mapping = tableau.var_mapping.get(var)
    if mapping is None:
        raise KeyError("%s is not a variable in the tableau" % (var,))
    if mapping[0] != "positive":
        raise ValueError("%s has no lower bound" % (var,))
    return np.float32(tableau.matrix[tableau.constraint_count, mapping[1]])


# ------------------------------------------------------------------ build-tableau (host)
def build_tableau_single(problem, fp_tolerance_factor=1024, device=0):
    """build-tableau (src/simplex.lisp:142-328) on single-float input: a SingleTableau, or [art, main] when
    the trivial basis is infeasible.  Numbers are combined the way Lisp's contagion does (module docstring);
    the finished matrices are coerced to float32 entry by entry."""
    check_single_problem(problem)
    constraints = [(op, list(expr), rhs) for op, expr, rhs in problem.constraints]
    pvars = list(problem.vars)
    n = len(pvars)
    bounds = dict(problem.var_bounds)
    mappings = {}

    def zeros(shape):
        M = np.empty(shape, dtype=object)
        M.fill(0)
        return M

    def mk(M, basis, var_count, ccount, inst):
        return SingleTableau(problem, inst, _to_f32(M), basis, var_count, ccount, mappings, fp_tolerance_factor, device)

    if not constraints:                                                  # :153-186
        M = zeros((n + 1, n + 1))
        basis = np.arange(n, dtype=np.int64)
        objd = dict(problem.objective_func)
        is_max = problem.type == "max"
        objective_value = 0
        for i, var in enumerate(pvars):
            coef = _n(objd[var])
            lb, ub = bounds.get(var, (None, None))
            M[i, i] = 1
            bound = ub if (0 <= coef) == is_max else lb
            if bound is None:
                raise UnboundedProblemError()
            mappings[var] = ("positive", i, _n(bound))
            objective_value = _add(objective_value, _mul(coef, _n(bound)))
        M[n, n] = objective_value
        return mk(M, basis, n, n, problem)

    ncv = n                                                              # :189-212
    column = 0
    for var in pvars:
        if var not in bounds:
            mappings[var] = ("positive", column, 0)
        else:
            lb, ub = bounds[var]
            if lb is not None and ub is not None:
                if 0 <= ub:
                    constraints.insert(0, ("<=", [(var, 1)], ub))
                else:
                    constraints.insert(0, (">=", [(var, 1)], _neg(_n(ub))))
                mappings[var] = ("positive", column, _n(lb))
            elif lb is not None:
                mappings[var] = ("positive", column, _n(lb))
            elif ub is not None:
                mappings[var] = ("negative", column, _n(ub))
            else:
                mappings[var] = ("signed", column)
                column += 1
                ncv += 1
        column += 1

    m = len(constraints)                                                 # :214-221
    num_slack = sum(1 for c in constraints if c[0] != "=")
    num_cols = ncv + num_slack + 1
    M = zeros((m + 1, num_cols))
    basis = np.zeros(m, dtype=np.int64)
    art_rows = []
    col_offset = 0
    last = num_cols - 1
    for row, (op, expr, rhs) in enumerate(constraints):                  # :223-268
        M[row, last] = _n(rhs)
        for var, coef in expr:
            mp, coef = mappings[var], _n(coef)
            if mp[0] == "positive":
                M[row, mp[1]] = coef
                M[row, last] = _sub(M[row, last], _mul(coef, mp[2]))     # :235
            elif mp[0] == "negative":
                M[row, mp[1]] = _neg(coef)
                M[row, last] = _sub(M[row, last], _mul(coef, mp[2]))     # :238
            else:
                M[row, mp[1]] = coef
                M[row, mp[1] + 1] = _neg(coef)
        if M[row, last] < 0:                                             # :243-252
            for c in range(num_cols):
                M[row, c] = _neg(M[row, c])
            op = {"<=": ">=", ">=": "<=", "=": "="}.get(op, op)
        if op == "<=":                                                   # :254-265
            M[row, ncv + col_offset] = 1
            basis[row] = ncv + col_offset
            col_offset += 1
        elif op == ">=":
            art_rows.insert(0, row)
            M[row, ncv + col_offset] = -1
            basis[row] = num_cols
            col_offset += 1
        elif op == "=":
            art_rows.insert(0, row)
            basis[row] = num_cols
        else:
            raise ParsingError("%r is not a valid constraint equation" % ((op, expr, rhs),))
    for var, coef in problem.objective_func:                             # :270-283
        mp, coef = mappings[var], _n(coef)
        if mp[0] == "positive":
            M[m, mp[1]] = _neg(coef)
            M[m, last] = _add(M[m, last], _mul(coef, mp[2]))
        elif mp[0] == "negative":
            M[m, mp[1]] = coef
            M[m, last] = _add(M[m, last], _mul(coef, mp[2]))
        else:
            M[m, mp[1]] = _neg(coef)
            M[m, mp[1] + 1] = coef
    main = mk(M, basis, num_cols - 1, m, problem)
    if not art_rows:
        return main
    num_art = len(art_rows)                                              # :292-325
    nac = num_cols + num_art
    A = zeros((m + 1, nac))
    abasis = basis.copy()
    for i, row in enumerate(art_rows):
        abasis[row] = num_cols - 1 + i
        A[row, num_cols - 1 + i] = 1
    for c in range(num_cols - 1):
        for r in range(m):
            A[r, c] = M[r, c]
    for r in range(m):
        A[r, nac - 1] = M[r, last]
    for c in list(range(num_cols - 1)) + [nac - 1]:
        s = 0
        for r in range(m):                                               # same summation order
            if r in art_rows:
                s = _add(s, A[r, c])
        A[m, c] = s
    art_problem = Problem(type="min", vars=list(problem.vars))           # artificial problem
    art = mk(A, abasis, num_cols - 1 + num_art, m, art_problem)
    return [art, main]


# ------------------------------------------------------------------ the hot path (device)
def find_entering_column(tableau):
    """find-entering-column (src/simplex.lisp:362-379): column index or None."""
    col = ctypes.c_int64(-1)
    capi.check(capi.lib().mi355x_stab_price(tableau._h, int(tableau.is_max), float(tableau.fp_tolerance_factor),
                                            ctypes.byref(col)), "mi355x_stab_price")
    return None if col.value < 0 else int(col.value)


def find_pivoting_row(tableau, entering_col):
    """find-pivoting-row (src/simplex.lisp:382-389): row index or None."""
    row = ctypes.c_int64(-1)
    capi.check(capi.lib().mi355x_stab_ratio(tableau._h, int(entering_col), float(tableau.fp_tolerance_factor),
                                            ctypes.byref(row)), "mi355x_stab_ratio")
    return None if row.value < 0 else int(row.value)


def n_pivot_row(tableau, entering_col, changing_row):
    """n-pivot-row (src/simplex.lisp:337-359): destructively applies a single pivot."""
    capi.check(capi.lib().mi355x_stab_pivot(tableau._h, int(entering_col), int(changing_row)), "mi355x_stab_pivot")
    tableau._touch()
    return tableau


def solve_status(tableau, max_pivots=0, chunk=None):
    """n-solve-tableau (src/simplex.lisp:399-461) in bounded foreign calls, without raising: a SingleTableau or
    [art, main] -> (status, pivots); pivots is a number, or (phase 1 + drive-outs, phase 2) for a pair.
    max_pivots (0: none) caps the pivots, for a pair both phases together; chunk: pivots per foreign call."""
    from .simplex import chunk_pivots
    L = capi.lib()
    if isinstance(tableau, (list, tuple)):
        art, main = tableau
        chunk = chunk or chunk_pivots(art.constraint_count + 1, art.var_count + 1)
        npv = (ctypes.c_int64 * 2)()
        n1 = n2 = 0
        try:
            while True:
                done = n1 + n2
                cap = min(chunk, max_pivots - done) if max_pivots > 0 else chunk
                rc = capi.check(L.mi355x_stab_solve_two_phase(art._h, main._h, int(main.is_max),
                                                              float(main.fp_tolerance_factor), int(cap), npv),
                                "mi355x_stab_solve_two_phase")
                n1, n2 = n1 + int(npv[0]), n2 + int(npv[1])
                if rc != capi.MI_MAX_PIVOTS or (max_pivots > 0 and n1 + n2 >= max_pivots):
                    main.n_pivots = (n1, n2)
                    return rc, (n1, n2)
        finally:
            art._touch()
            main._touch()
    if not isinstance(tableau, SingleTableau):                # (check-type tableau tableau) :454
        raise TypeError("%r is not a single-float tableau" % (tableau,))
    chunk = chunk or chunk_pivots(tableau.constraint_count + 1, tableau.var_count + 1)
    n, total = ctypes.c_int64(0), 0
    try:
        while True:
            cap = min(chunk, max_pivots - total) if max_pivots > 0 else chunk
            rc = capi.check(L.mi355x_stab_solve(tableau._h, int(tableau.is_max), float(tableau.fp_tolerance_factor),
                                                int(cap), ctypes.byref(n)), "mi355x_stab_solve")
            total += int(n.value)
            if rc != capi.MI_MAX_PIVOTS or (max_pivots > 0 and total >= max_pivots):
                tableau.n_pivots = total
                return rc, total
    finally:
        tableau._touch()


def n_solve_tableau(tableau, max_pivots=0, chunk=None):
    """solve_status with the reference's conditions raised; returns the solved (main) tableau."""
    from .simplex import _raise_for
    rc, _ = solve_status(tableau, max_pivots=max_pivots, chunk=chunk)
    _raise_for(rc)
    return tableau[1] if isinstance(tableau, (list, tuple)) else tableau


def solve_single(problem, fp_tolerance=1024, device=0, max_pivots=0, chunk=None):
    """What mi355x_simplex_solver(problem, precision="single") returns: the solved SingleTableau."""
    if problem.integer_vars:
        raise UnsupportedConstraintError(("integer",) + tuple(problem.integer_vars), "mi355x-simplex")
    tabs = build_tableau_single(problem, fp_tolerance_factor=fp_tolerance, device=device)
    return n_solve_tableau(tabs, max_pivots=max_pivots, chunk=chunk)
