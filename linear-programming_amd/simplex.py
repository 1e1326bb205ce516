"""Host-side mirror of the reference's `linear-programming/simplex` package
(src/simplex.lisp) over the MI355X C ABI.

Same names (Lisp `n-pivot-row` -> `n_pivot_row`), same argument meaning, same error
behaviour, so the parity tests read like t/simplex.lisp.  Every numeric step of the hot path
-- pricing, ratio test, rank-1 update, the solve loops, the two-phase hand-over -- runs in
``libmi355x_simplex.so`` on the GPU; this module only moves arrays across the boundary and
does the O(n) bookkeeping that stays on the host in the Lisp glue as well
(`build-tableau` before the boundary, `tableau-variable` read-back after it).

The tableau lives in HBM behind ``Tableau._h``; ``Tableau.matrix`` / ``basis_columns`` are
host copies refreshed lazily after every device-side mutation.
"""
import ctypes

import numpy as np

from . import capi
from .capi import _ptr
from .conditions import InfeasibleProblemError, SolverError, UnboundedProblemError, UnsupportedConstraintError
from .lists import chunk_pivots                              # noqa: F401  (simplex.chunk_pivots: its name for tools)
from .lists import file_by_shape, finish, member_pivots, one_by_one, place, solve_in_chunks
from .lowering import DOUBLE, EXACT, build
from .problem import Problem


class TableauStruct:
    """What Tableau, SingleTableau and ExactTableau share: the fields of the `tableau` struct
    (src/simplex.lisp:48-58: problem, instance-problem, matrix, basis-columns, var-count,
    constraint-count, var-mapping), host copies of matrix and basis that the class's _refresh brings
    up to date after a device-side mutation (_touch), and the release of the handle.  A class names
    its number system (lowering.py) and the prefix of its C entries: mi355x_<_entry>_*."""
    exact = False
    ns = _entry = None
    _handle = _light = None

    def _struct(self, problem, instance_problem, var_count, constraint_count, var_mapping, device,
                matrix=None, basis_columns=None):
        """The fields; matrix (contiguous, of the class's type) and basis_columns: the host copies a tableau
        starts from (the upload happens at the first device operation)."""
        self.problem = problem
        self.instance_problem = instance_problem
        self.var_count = int(var_count)
        self.constraint_count = int(constraint_count)
        self.var_mapping = var_mapping
        self.device = device
        if matrix is None:
            return
        basis = np.ascontiguousarray(basis_columns, dtype=np.int64)
        if matrix.shape != (self.constraint_count + 1, self.var_count + 1):
            raise ValueError("matrix shape %r does not match counts" % (matrix.shape,))
        if basis.shape != (self.constraint_count,):
            raise ValueError("basis length %r does not match constraint count" % (basis.shape,))
        self._matrix, self._basis, self._stale = matrix.copy(), basis.copy(), False

    def _entry_point(self, name):
        return getattr(capi.lib(), "mi355x_%s_%s" % (self._entry, name))

    def _touch(self):
        self._stale = True
        self._light = None

    def _readback(self):
        """(objective row, RHS column, basis) -- all the read-back functions need (src/simplex.lisp:74-120)."""
        M = self.matrix
        return M[-1], M[:, -1], self.basis_columns

    @property
    def matrix(self):
        """tableau-matrix (host copy of the device-resident matrix)."""
        self._refresh()
        return self._matrix

    @property
    def basis_columns(self):
        """tableau-basis-columns."""
        self._refresh()
        return self._basis

    @property
    def is_max(self):
        return self.instance_problem.type == "max"

    def __del__(self):
        h = getattr(self, "_handle", None)
        self._handle = None
        if h:
            try:
                self._entry_point("destroy")(h)
            except Exception:
                pass


class Tableau(TableauStruct):
    """The `tableau` struct in double-float, with fp-tolerance-factor, behind a mi355x_tab."""
    ns, _entry = DOUBLE, "tab"

    def __init__(self, problem, instance_problem, matrix, basis_columns, var_count,
                 constraint_count, var_mapping, fp_tolerance_factor=1024, device=0, _handle=None):
        self.fp_tolerance_factor = fp_tolerance_factor
        if _handle is not None:
            self._struct(problem, instance_problem, var_count, constraint_count, var_mapping, device)
            self._handle, self._matrix, self._basis, self._stale = _handle, None, None, True
        else:
            self._struct(problem, instance_problem, var_count, constraint_count, var_mapping, device,
                         np.ascontiguousarray(matrix, dtype=np.float64), basis_columns)

    # -- device <-> host
    @property
    def _h(self):
        """The device handle (uploads the host arrays on first use; no CPU fallback)."""
        if self._handle is None:
            h = ctypes.c_void_p()
            capi.check(capi.lib().mi355x_tab_create(
                ctypes.byref(h), self._matrix.shape[0], self._matrix.shape[1], _ptr(self._matrix),
                _ptr(self._basis) if self._basis.size else None, self.device), "mi355x_tab_create")
            self._handle = h
        return self._handle

    def _refresh(self):
        if self._stale:
            R, C = self.constraint_count + 1, self.var_count + 1
            M = np.empty((R, C), dtype=np.float64)
            b = np.empty(max(R - 1, 0), dtype=np.int64)
            capi.check(capi.lib().mi355x_tab_download(self._h, _ptr(M), _ptr(b) if b.size else None,
                                                      None, None), "mi355x_tab_download")
            self._matrix, self._basis, self._stale = M, b, False

    def _readback(self):
        """Served from the host copy when it is current, otherwise fetched alone
        (mi355x_tab_download without the matrix), never the whole tableau."""
        if not self._stale:
            return self._matrix[-1], self._matrix[:, -1], self._basis
        if self._light is None:
            R, C = self.constraint_count + 1, self.var_count + 1
            row, col = np.empty(C), np.empty(R)
            b = np.empty(max(R - 1, 0), dtype=np.int64)
            capi.check(capi.lib().mi355x_tab_download(self._h, None, _ptr(b) if b.size else None,
                                                      _ptr(row), _ptr(col)), "mi355x_tab_download")
            self._light = (row, col, b)
        return self._light

    def pivot_trace(self, cap=1 << 20):
        """(entering column, row) of every pivot made on this tableau since it was uploaded."""
        n = ctypes.c_int64(0)
        ec = np.empty(cap, dtype=np.int64)
        cr = np.empty(cap, dtype=np.int64)
        capi.check(capi.lib().mi355x_tab_trace(self._h, _ptr(ec), _ptr(cr), cap, ctypes.byref(n)),
                   "mi355x_tab_trace")
        k = min(n.value, cap)
        return np.stack([ec[:k], cr[:k]], axis=1)


def copy_tableau(tableau):
    """copy-tableau (src/simplex.lisp:61-71): deep-copies matrix and basis (device to device),
    shares everything else."""
    h = ctypes.c_void_p()
    capi.check(capi.lib().mi355x_tab_copy(ctypes.byref(h), tableau._h), "mi355x_tab_copy")
    return Tableau(tableau.problem, tableau.instance_problem, None, None, tableau.var_count,
                   tableau.constraint_count, tableau.var_mapping, tableau.fp_tolerance_factor,
                   tableau.device, _handle=h)


# ------------------------------------------------------------------ read-back (host, O(n))
# One copy for the three tableau classes: entries come back as the tableau's number system returns them
# (ns.value: float, Fraction, np.float32) and a mapping's offset is added as ns.offset of it (single-float: in
# float32).
def tableau_objective_value(tableau):
    """tableau-objective-value (src/simplex.lisp:74-78)."""
    return tableau.ns.value(tableau._readback()[0][tableau.var_count])


def _basic_value(tableau, col):
    _, rhs, basis = tableau._readback()
    pos = np.nonzero(basis == col)[0]                       # `position`: first match
    return tableau.ns.value(rhs[pos[0]] if pos.size else 0)


def tableau_variable(tableau, var):
    """tableau-variable (src/simplex.lisp:81-107), the bound's offset included."""
    if var == tableau.instance_problem.objective_var:
        return tableau_objective_value(tableau)
    mapping = tableau.var_mapping.get(var)
    if mapping is None:
        raise KeyError("%s is not a variable in the tableau" % (var,))
    kind = mapping[0]
    if kind == "positive":
        return tableau.ns.offset(mapping[2]) + _basic_value(tableau, mapping[1])
    if kind == "negative":
        return tableau.ns.offset(mapping[2]) + (-_basic_value(tableau, mapping[1]))
    return _basic_value(tableau, mapping[1]) - _basic_value(tableau, mapping[1] + 1)


def tableau_reduced_cost(tableau, var):
    """tableau-reduced-cost (src/simplex.lisp:111-120)."""
    mapping = tableau.var_mapping.get(var)
    if mapping is None:
        raise KeyError("%s is not a variable in the tableau" % (var,))
    if mapping[0] != "positive":
        raise ValueError("%s has no lower bound" % (var,))
    return tableau.ns.value(tableau._readback()[0][mapping[1]])


def with_tableau_variables(var_list, tableau):
    """with-tableau-variables (src/simplex.lisp:125-139) as a function: the values of the given
    variables (a sequence of names, or a Problem: its objective variable and all its variables)
    read from the tableau, as a dict."""
    if isinstance(var_list, Problem):
        names = [var_list.objective_var] + list(var_list.vars)
    else:
        names = list(var_list)
    return {v: tableau_variable(tableau, v) for v in names}


# ------------------------------------------------------------------ build-tableau (host)
def build_tableau(problem, instance_problem=None, fp_tolerance_factor=1024, device=0, exact=False, min_bits=0,
                  general=False, max_bits=128):
    """build-tableau (src/simplex.lisp:142-328) in double-float: returns a Tableau, or
    [art_tableau, main_tableau] when the trivial basis is infeasible.  The steps are lowering.py's.

    This is the producer of what crosses the boundary; in the Lisp deployment the reference's
    own build-tableau does this job and the glue converts the result to double-float.
    exact=True: the same steps in exact rationals (Fraction object matrices, Fraction mapping
    offsets), the reference's own build-tableau on rational input; the result is an ExactTableau
    (exact.py, min_bits: its starting width, max_bits: the widest it may escalate to, 128 or 256) or a
    list of two.
    general=True: the general form only -- the main tableau of :189-283 (basis entry = the number of
    columns on a row that needs an artificial variable), also for a problem without constraints: what
    branch-and-bound nodes are assembled from (exact_bb.py; host_problem.cpp's build(general=true))."""
    if instance_problem is None:
        instance_problem = problem
    if exact:
        from .exact import ExactTableau

        def make(inst, M, basis, mapping):
            return ExactTableau(problem, inst, M, basis, M.shape[1] - 1, M.shape[0] - 1, mapping, device, min_bits,
                                max_bits)
    else:
        def make(inst, M, basis, mapping):
            return Tableau(problem, inst, M, basis, M.shape[1] - 1, M.shape[0] - 1, mapping,
                           fp_tolerance_factor, device)
    return build(problem, instance_problem, EXACT if exact else DOUBLE, make, general)


# ------------------------------------------------------------------ the hot path (device)
# (a Tableau or a SingleTableau: the same three entries behind the class's prefix)
def find_entering_column(tableau):
    """find-entering-column (src/simplex.lisp:362-379): column index or None."""
    col = ctypes.c_int64(-1)
    capi.check(tableau._entry_point("price")(tableau._h, int(tableau.is_max), float(tableau.fp_tolerance_factor),
                                             ctypes.byref(col)), "mi355x_%s_price" % tableau._entry)
    return None if col.value < 0 else int(col.value)


def find_pivoting_row(tableau, entering_col):
    """find-pivoting-row (src/simplex.lisp:382-389): row index or None."""
    row = ctypes.c_int64(-1)
    capi.check(tableau._entry_point("ratio")(tableau._h, int(entering_col), float(tableau.fp_tolerance_factor),
                                             ctypes.byref(row)), "mi355x_%s_ratio" % tableau._entry)
    return None if row.value < 0 else int(row.value)


def n_pivot_row(tableau, entering_col, changing_row):
    """n-pivot-row (src/simplex.lisp:337-359): destructively applies a single pivot."""
    capi.check(tableau._entry_point("pivot")(tableau._h, int(entering_col), int(changing_row)),
               "mi355x_%s_pivot" % tableau._entry)
    tableau._touch()
    return tableau


def pivot_row(tableau, entering_col, changing_row):
    """pivot-row (src/simplex.lisp:333-335): non-destructive."""
    return n_pivot_row(copy_tableau(tableau), entering_col, changing_row)


def _raise_for(rc):
    if rc == capi.MI_UNBOUNDED:
        raise UnboundedProblemError()
    if rc == capi.MI_INFEASIBLE:
        raise InfeasibleProblemError()
    if rc == capi.MI_ART_NONZERO:
        raise SolverError("Artificial variable still non-zero")
    if rc == capi.MI_ART_STUCK:
        raise SolverError("Artificial variable still in basis and cannot be replaced")
    if rc == capi.MI_MAX_PIVOTS:
        raise SolverError("pivot cap reached")
    if rc == capi.MI_CANCELLED:
        raise SolveCancelled("solve cancelled (mi355x_tab_cancel)")


def _error_for(rc):
    """The exception of a member's final status (None: it has a solution)."""
    try:
        _raise_for(rc)
    except SolverError as e:
        return e


class SolveCancelled(SolverError):
    """cancel_solve() was called from another thread: the solve stopped between two chunks of
    launches.  The tableau holds whole pivots only and can be solved further.  (In Lisp the same
    situation is an interrupt honoured between two bounded foreign calls.)"""


def cancel_solve(tableau):
    """Ask the solve running on `tableau` (in another thread) -- or the next one -- to stop:
    mi355x_tab_cancel.  The reference's loop has no cap and no anti-cycling rule
    (src/simplex.lisp:453-461); in Lisp a cycling LP is interruptible, a foreign call is not."""
    for t in (tableau if isinstance(tableau, (list, tuple)) else [tableau]):
        capi.check(capi.lib().mi355x_tab_cancel(t._h), "mi355x_tab_cancel")


def _solve_two_phase_in_chunks(art, main, max_pivots=0, chunk=None):
    """The glue's `solve-two-phase-in-chunks`: phase 1 in chunks on the artificial tableau,
    mi355x_two_phase_handover, phase 2 in chunks on the main tableau -- the pivots and bits of
    mi355x_solve_two_phase without an unbounded foreign call; max_pivots caps the phases together."""
    L = capi.lib()
    n = ctypes.c_int64(0)
    f = float(main.fp_tolerance_factor)
    rows, cols = art.constraint_count + 1, art.var_count + 1

    def phase(t, is_max):
        def call(cap):
            rc = capi.check(L.mi355x_tab_solve(t._h, int(is_max), f, int(cap), ctypes.byref(n)), "mi355x_tab_solve")
            return rc, int(n.value)
        return call
    try:
        rc, n1 = solve_in_chunks(phase(art, 0), rows, cols, int(max_pivots), chunk=chunk)
        main.n_pivots = (n1, 0)
        if rc != capi.MI_OPTIMAL:
            return rc
        rc = capi.check(L.mi355x_two_phase_handover(art._h, main._h, f, ctypes.byref(n)), "mi355x_two_phase_handover")
        n1 += int(n.value)
        main.n_pivots = (n1, 0)
        if rc != capi.MI_OK:
            return rc
        if max_pivots > 0 and n1 >= max_pivots:
            return capi.MI_MAX_PIVOTS
        rc, n2 = solve_in_chunks(phase(main, main.is_max), rows, cols, max_pivots - n1 if max_pivots > 0 else 0, chunk=chunk)
        main.n_pivots = (n1, n2)
        return rc
    finally:
        art._touch()
        main._touch()


def n_solve_tableau(tableau, max_pivots=0, chunked=False, chunk=None):
    """n-solve-tableau (src/simplex.lisp:399-461): a Tableau (single phase) or a list
    [art, main] (two-phase).  Returns the solved (main) tableau.  chunked: bounded foreign calls
    (what the Lisp glue does, see chunk_pivots)."""
    if isinstance(tableau, (list, tuple)):
        art, main = tableau
        if not isinstance(art, Tableau) or not isinstance(main, Tableau):
            raise TypeError("expected tableaus")
        if chunked:
            rc = _solve_two_phase_in_chunks(art, main, int(max_pivots), chunk=chunk)
            _raise_for(rc)
            return main
        npv = (ctypes.c_int64 * 2)()
        rc = capi.check(capi.lib().mi355x_solve_two_phase(
            art._h, main._h, int(main.is_max), float(main.fp_tolerance_factor), npv),
            "mi355x_solve_two_phase")
        art._touch()
        main._touch()
        main.n_pivots = (int(npv[0]), int(npv[1]))
        _raise_for(rc)
        return main
    if not isinstance(tableau, Tableau):                    # (check-type tableau tableau) :454
        raise TypeError("%r is not a tableau" % (tableau,))
    n = ctypes.c_int64(0)

    def call(cap):
        rc = capi.check(capi.lib().mi355x_tab_solve(tableau._h, int(tableau.is_max),
                                                    float(tableau.fp_tolerance_factor),
                                                    int(cap), ctypes.byref(n)),
                        "mi355x_tab_solve")
        return rc, int(n.value)
    if chunked:
        rc, total = solve_in_chunks(call, tableau.constraint_count + 1, tableau.var_count + 1, int(max_pivots), chunk=chunk)
    else:
        rc, total = call(max_pivots)
    tableau._touch()
    tableau.n_pivots = total
    _raise_for(rc)
    return tableau


def solve_tableau(tableau):
    """solve-tableau (src/simplex.lisp:391-397): leaves the argument(s) untouched."""
    if isinstance(tableau, (list, tuple)):
        return n_solve_tableau([copy_tableau(t) for t in tableau])
    return n_solve_tableau(copy_tableau(tableau))


# ------------------------------------------------------------------ the *solver* hook value
def _solve_column_partitioned(tableau, devices, max_pivots=0):
    """The glue's `solve-column-partitioned` (lisp/mi355x-simplex.lisp): the tableau of a
    single-phase problem split over `devices` GPUs behind mi355x_colpart_create / _solve /
    _download / _destroy.  Returns False when the library stopped with MI_NONFINITE (the tableau
    overflowed; compact shards cannot reproduce that case): the caller's tableau is untouched."""
    L = capi.lib()
    M, b = tableau.matrix, tableau.basis_columns
    h = ctypes.c_void_p()
    capi.check(L.mi355x_colpart_create(ctypes.byref(h), M.shape[0], M.shape[1], _ptr(M), _ptr(b),
                                       int(devices)), "mi355x_colpart_create")
    try:
        n = ctypes.c_int64(0)

        def call(cap):
            rc = capi.check(L.mi355x_colpart_solve(h, int(tableau.is_max), float(tableau.fp_tolerance_factor),
                                                   int(cap), ctypes.byref(n)), "mi355x_colpart_solve")
            return rc, int(n.value)
        rc, total = solve_in_chunks(call, M.shape[0], M.shape[1], int(max_pivots))
        if rc == capi.MI_NONFINITE:
            return False
        tableau.n_pivots = total
        _raise_for(rc)
        G, bg = np.empty_like(M), np.empty_like(b)
        capi.check(L.mi355x_colpart_download(h, _ptr(G), _ptr(bg), None, None), "mi355x_colpart_download")
    finally:
        L.mi355x_colpart_destroy(h)
    # the solved arrays become the tableau's host copy; its device handle (if any) is stale
    old, tableau._handle = tableau._handle, None
    if old:
        L.mi355x_tab_destroy(old)
    tableau._matrix, tableau._basis, tableau._stale, tableau._light = G, bg, False, None
    return True


def _solve_two_phase_column_partitioned(art, main, devices):
    """The two-phase branch with the artificial tableau column-partitioned over `devices` GPUs
    (mi355x_colpart_create -> mi355x_colpart_solve_two_phase -> download of both tableaux).  The
    main tableau is never uploaded: the library takes its objective row only.  Returns False when
    the partitioned path does not apply (MI_UNSUPPORTED: the artificial basis is not a set of unit
    columns; MI_NONFINITE: the tableau overflowed) -- the caller's tableaux are untouched."""
    L = capi.lib()
    A, ab = art.matrix, art.basis_columns
    Mm = main.matrix
    h = ctypes.c_void_p()
    capi.check(L.mi355x_colpart_create(ctypes.byref(h), A.shape[0], A.shape[1], _ptr(A), _ptr(ab),
                                       int(devices)), "mi355x_colpart_create")
    hm = ctypes.c_void_p()
    try:
        obj = np.ascontiguousarray(Mm[-1])
        npv = (ctypes.c_int64 * 2)()
        rc = L.mi355x_colpart_solve_two_phase(h, int(Mm.shape[1]), _ptr(obj), int(main.is_max),
                                              float(main.fp_tolerance_factor), npv, ctypes.byref(hm))
        if rc in (capi.MI_UNSUPPORTED, capi.MI_NONFINITE):
            return False
        capi.check(rc, "mi355x_colpart_solve_two_phase")
        GA, ga = np.empty_like(A), np.empty_like(ab)
        capi.check(L.mi355x_colpart_download(h, _ptr(GA), _ptr(ga), None, None), "mi355x_colpart_download")
        GM, gm = None, None
        if hm:
            GM, gm = np.empty_like(Mm), np.empty_like(main.basis_columns)
            capi.check(L.mi355x_colpart_download(hm, _ptr(GM), _ptr(gm), None, None), "mi355x_colpart_download")
    finally:
        if hm:
            L.mi355x_colpart_destroy(hm)
        L.mi355x_colpart_destroy(h)
    for tab, G, g in ((art, GA, ga), (main, GM, gm)):
        if G is None:
            continue
        old, tab._handle = tab._handle, None
        if old:
            L.mi355x_tab_destroy(old)
        tab._matrix, tab._basis, tab._stale, tab._light = G, g, False, None
    main.n_pivots = (int(npv[0]), int(npv[1]))
    _raise_for(rc)
    return True


def _native_number(x):
    """The glue's `native-number-p`: numbers the library's double-float build-tableau treats exactly
    as generic arithmetic followed by a coerce would -- doubles and integers a double holds exactly
    (a Fraction, like a Lisp ratio, is combined exactly first and rounded afterwards)."""
    if isinstance(x, bool):
        return False
    if isinstance(x, int):
        return abs(x) <= 2 ** 53
    return isinstance(x, float)


def _native_numbers(problem):
    ok = all(_native_number(c) for _, c in problem.objective_func)
    ok = ok and all((lb is None or _native_number(lb)) and (ub is None or _native_number(ub))
                    for _, (lb, ub) in problem.var_bounds)
    return ok and all(all(_native_number(c) for _, c in e) and _native_number(rhs)
                      for _, e, rhs in problem.constraints)


def mi355x_simplex_solver(problem, fp_tolerance=1024, device=0, devices=1, max_pivots=0,
                          full_tableau=False, native="auto", chunk=None, branch_and_bound=False,
                          bb_width=1, int_tolerance=0, max_nodes=0, exact=False, exact_bits=0, exact_max_bits=128,
                          pivot_rule="dantzig", precision="double", beyond_lds=False, mixed_shapes=False, **_ignored):
    """What the Lisp glue installs as `*solver*` (src/solver.lisp:39-56): takes a problem and
    backend keyword arguments, returns a solution object answering the four solution-*
    generics -- on the NATIVE route (default whenever the problem's numbers are floats / integers
    and neither full_tableau nor devices > 1 asks for the tableau itself; native=True forces it,
    native=False never takes it) a NativeSolution (the glue's MI355X-SOLUTION: problem marshalled
    through mi355x_problem_*, mi355x_simplex_solver_begin / _step in bounded chunks / _finish), on
    the build-tableau route a solved Tableau.  By default integer/binary variables are declined the way a backend must
    (unsupported-constraint-error, src/conditions.lisp:69-77); branch_and_bound=True opts in (below).  devices > 1: the tableau
    (single-phase problems) or the artificial tableau (two-phase problems: phase 1, the hand-over
    and phase 2 all stay partitioned) is column-partitioned over that many GPUs (logical shards of
    one GPU when fewer are visible); tableaux that overflow run on `device`.
    branch_and_bound=True (opt-in) solves integer problems instead: the reference's branch-and-bound
    (src/simplex.lisp:462-542) node for node through the library's job (mi355x_simplex_solver_bb_*,
    stepped in bounded chunks of nodes), up to bb_width node LPs side by side on `devices` GPUs
    (logical devices of one GPU when fewer are visible); int_tolerance > 0 counts values within
    int_tolerance * epsilon of an integer as integral (0: exact); max_nodes caps the nodes
    processed (0: no cap).  Returns the incumbent's NativeSolution.
    exact=True (opt-in): a problem whose numbers are all rational (int or Fraction) is solved with the
    reference's rational semantics (src/utils.lisp:84-124) on exact integer tableaux (exact.py) and the
    solved ExactTableau is returned, its read-back in Fractions; exact_bits 128 starts at 128 bits
    instead of 64.  Any float in the problem means the double path, unchanged.  exact_max_bits=256
    (opt-in; default 128) lets a solve whose entries outgrow 128 bits start again at 256 bits instead of
    being declined (exact_bits=256 then starts there); the condition past 256 bits names that limit.
    exact=True together with branch_and_bound=True, on a problem with integer variables whose numbers are
    all rational: the reference's branch-and-bound in rational arithmetic, where its integrality test is
    `integerp` of a ratio (src/simplex.lisp:475-480) -- exact_bb.py: up to bb_width node LPs side by side
    as batches of exact tableaux assembled on the device; returns the incumbent's solved ExactTableau.
    (With a float anywhere: the f64 branch-and-bound above, unchanged.  Without integer variables the
    combination is declined.)  Exact branch-and-bound rides on batches, which stop at 128 bits: together
    with exact_max_bits=256 it is an argument error.
    pivot_rule (opt-in, exact solves only): "dantzig" (default) is the reference's choice of entering column
    and pivot row (find-entering-column / find-pivoting-row), which has no anti-cycling rule, so that on
    rationals a cycle never ends; "bland" takes the lowest eligible column and breaks ratio ties by the lowest
    basis column, "dantzig-bland" does so only after a degenerate pivot and until the next one that is not.
    Both end on every input.  It reaches the exact branch-and-bound's root and node batches as well.  An
    unknown name and a rule other than "dantzig" without exact=True are argument errors (in floating point
    neither rule is a theorem); with exact=True on a problem that holds a float -- which would take the double
    path -- such a rule is declined: unsupported-constraint-error ("exact", "pivot-rule", name).
    precision="single" (opt-in; default "double": everything above, unchanged): the reference's single-float path
    (single.py) -- build-tableau with Lisp's contagion, IEEE binary32 arithmetic and single-float-epsilon thresholds
    on the GPU, the solved SingleTableau returned, its read-back in np.float32.  Every number of the problem must
    be an integer with |x| <= 2**24 or a float whose value a binary32 holds exactly; anything else is declined:
    unsupported-constraint-error ("single", number).  Together with exact, devices > 1, native=True, full_tableau
    or a pivot_rule other than "dantzig" it is an argument error that names the pair; so is an unknown precision.
    precision="single" together with branch_and_bound=True, on a problem WITH integer variables (opt-in): the
    reference's branch-and-bound in single-float arithmetic (single_bb.py) -- the search of the exact route with
    the float32 reading of `integerp` (v == floor(v); int_tolerance > 0: within int_tolerance *
    single-float-epsilon of an integer), floor / ceiling bounds as exact integers, up to bb_width node LPs side by
    side as batches of single-float tableaux assembled on the device; max_nodes, max_pivots (per node LP, both
    phases together) and chunk as on the exact search.  Returns the incumbent's solved SingleTableau.  On a problem
    without integer variables the pair stays an argument error that names "single" and "branch_and_bound"; without
    branch_and_bound an integer problem is declined: unsupported-constraint-error ("integer" ...).
    beyond_lds=True (opt-in, with that pair only -- an argument error anywhere else on this function): a node group
    beyond the batches' LDS budget that has at least single.global_batch_min_members nodes goes as ONE global-form
    batch (or pair) instead of node by node; the search and its result are the same, bit for bit.
    mixed_shapes=True (opt-in, with that pair only -- an argument error anywhere else on this function): the node LPs
    of a round that fit the LDS budget go as ONE ragged batch and ONE ragged pair built on the device, whatever their
    depths, instead of one batch per (depth, artificial rows) group; the search and its result are the same, bit for
    bit."""
    if precision not in ("double", "single"):
        raise ValueError("precision=%r: \"double\" (default) or \"single\"" % (precision,))
    single_bb_route = precision == "single" and branch_and_bound and problem.integer_vars and not exact and \
        devices <= 1 and native is not True and not full_tableau and pivot_rule == "dantzig"
    if beyond_lds and not single_bb_route:
        raise ValueError("beyond_lds=True needs precision=\"single\", branch_and_bound=True and a problem with integer "
                         "variables: it batches the single-float node LPs beyond the LDS budget")
    if mixed_shapes and not single_bb_route:
        raise ValueError("mixed_shapes=True needs precision=\"single\", branch_and_bound=True and a problem with integer "
                         "variables: it batches the single-float node LPs of a round whatever their depths")
    if precision == "single" and branch_and_bound and problem.integer_vars and not exact and devices <= 1 and \
            native is not True and not full_tableau and pivot_rule == "dantzig":
        from .single_bb import solve_branch_and_bound_single
        return solve_branch_and_bound_single(problem, width=bb_width, fp_tolerance=fp_tolerance,
                                             int_tolerance=int_tolerance, device=device, max_pivots=max_pivots,
                                             max_nodes=max_nodes, chunk=chunk,
                                             **({"beyond_lds": True} if beyond_lds else {}),
                                             **({"mixed_shapes": True} if mixed_shapes else {}))
    if precision == "single":
        for name, clash in (("exact", bool(exact)), ("branch_and_bound", bool(branch_and_bound)),
                            ("devices", devices > 1), ("native", native is True), ("full_tableau", bool(full_tableau)),
                            ("pivot_rule", pivot_rule != "dantzig")):
            if clash:
                raise ValueError("precision=\"single\" does not go with %s=%r: the single-float path is one tableau "
                                 "on one device under the reference's rule"
                                 % (name, {"exact": exact, "branch_and_bound": branch_and_bound, "devices": devices,
                                           "native": native, "full_tableau": full_tableau, "pivot_rule": pivot_rule}[name]))
        from .single import solve_single
        return solve_single(problem, fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots, chunk=chunk)
    from .exact import pivot_rule_code
    if pivot_rule_code(pivot_rule) != 0 and not exact:
        raise ValueError("pivot_rule=%r needs exact=True: the double-precision paths keep the reference's rule"
                         % (pivot_rule,))
    if pivot_rule != "dantzig":
        from .exact import rational_problem
        if not rational_problem(problem):
            raise UnsupportedConstraintError(("exact", "pivot-rule", pivot_rule), "mi355x-simplex")
    if exact and exact_max_bits != 128:
        from .exact import _check_widths
        _check_widths(exact_bits, exact_max_bits)
        if branch_and_bound:
            raise ValueError("exact=True, branch_and_bound=True does not take exact_max_bits=%r: exact "
                             "branch-and-bound runs on batches of at most 128 bits" % (exact_max_bits,))
    if exact and branch_and_bound:
        from .exact import rational_problem
        if not problem.integer_vars:
            raise UnsupportedConstraintError(("exact", "branch-and-bound"), "mi355x-simplex")
        if rational_problem(problem):
            from .exact_bb import solve_branch_and_bound_exact
            return solve_branch_and_bound_exact(problem, width=bb_width, device=device, max_pivots=max_pivots,
                                                max_nodes=max_nodes, min_bits=exact_bits, chunk=chunk,
                                                pivot_rule=pivot_rule)
    if problem.integer_vars and branch_and_bound:
        from .native import solve_branch_and_bound
        return solve_branch_and_bound(problem, fp_tolerance=fp_tolerance, int_tolerance=int_tolerance,
                                      width=bb_width, devices=devices, max_nodes=max_nodes)
    if problem.integer_vars:
        raise UnsupportedConstraintError(("integer",) + tuple(problem.integer_vars),
                                         "mi355x-simplex")
    if exact:
        from .exact import rational_problem, solve_exact
        if rational_problem(problem):
            return solve_exact(problem, device=device, max_pivots=max_pivots, min_bits=exact_bits, chunk=chunk,
                               exact_max_bits=exact_max_bits, pivot_rule=pivot_rule)
    if native and not full_tableau and devices <= 1 and len(problem.vars) > 0 and \
            (native is True or _native_numbers(problem)):
        from .native import NativeProblem
        return NativeProblem(problem).solve_in_chunks(fp_tolerance=fp_tolerance, device=device,
                                                      max_pivots=max_pivots, chunk=chunk)
    tabs = build_tableau(problem, problem, fp_tolerance_factor=fp_tolerance, device=device)
    if devices > 1 and isinstance(tabs, Tableau) and _solve_column_partitioned(tabs, devices, max_pivots):
        return tabs
    if devices > 1 and isinstance(tabs, list) and _solve_two_phase_column_partitioned(tabs[0], tabs[1], devices):
        return tabs[1]
    return n_solve_tableau(tabs, max_pivots=max_pivots, chunked=True, chunk=chunk)


simplex_solver = mi355x_simplex_solver


def mi355x_solve_problems(problems, fp_tolerance=1024, device=0, devices=1, max_pivots=0, errorp=True, native=False,
                          exact=False, exact_bits=0, exact_max_bits=128, pivot_rule="dantzig", device_build=False,
                          from_rows=False, precision="double", beyond_lds=False, mixed_shapes=False):
    """The glue's `mi355x-solve-problems`: a LIST of problems -> the list of their solved tableaus,
    what [solve_problem(p) for p in problems] returns, with the independent LPs side by side on the
    GPU(s).  Single-phase problems are grouped by tableau shape and sense; a group of two or more
    is ONE multi-device batch (mi355x_multibatch_create / _solve in bounded chunks / _download per
    member / _destroy: `devices` sub-batches, no communication).  Two-phase problems
    (src/simplex.lisp:402-452) are grouped by the shapes of their two tableaux; a group of two or more
    is a pair of batches: phase 1 and phase 2 through mi355x_multibatch_solve in bounded chunks, the
    per-member feasibility test, drive-out pivots and hand-over through
    mi355x_multibatch_two_phase_handover.  Integer problems (declined) and problems alone in their
    group go through mi355x_simplex_solver one by one; max_pivots caps every phase.  A member without a solution does not abort the
    others: errorp False leaves the exception object in its place, errorp True raises the first
    one after every member has been attempted.
    exact=True (opt-in): the members whose numbers are all rational (and that have no integer variables)
    are built with build_tableau(exact=True) and grouped in the same way; a group of two or more is ONE
    batch of exact tableaux (mi355x_xbatch_create / _solve or _solve_two_phase in bounded chunks, one
    workgroup per member, exact.py), and every member comes back as the solved ExactTableau that
    mi355x_simplex_solver(p, exact=True) returns (exact_bits as there).  Members alone in their group,
    shapes the batch declines and members with a float anywhere go through
    mi355x_simplex_solver(..., exact=True) one by one; max_pivots caps each member (both phases
    together, as there).  exact_max_bits=256: batches stay at 64 / 128 bits; a member a batch declines for
    overflowing 128 bits is solved again alone with 256 bits allowed and its result takes its slot.
    exact=False: nothing changes.
    device_build=True (opt-in, with exact=True only -- an argument error otherwise): the exact members' tableaux are
    built on the device from their rows (exact_lps.py: mi355x_xbatch_create_lps) instead of on the host; the
    results are the same, member for member.
    from_rows=True (opt-in, double precision only -- with exact=True an argument error that points to device_build,
    as is native="many", which builds its members in the library): the members are only lowered to their rows
    (batch_lps.py: lower_problem_rows) and the groups' tableaux are built on the device
    (mi355x_multibatch_create_lps) instead of on the host and uploaded; groups are formed by (constraints,
    structural columns, `=` rows, artificial rows, sense) and solved in the same bounded chunks, and every member
    comes back as the Tableau the default route returns.  Integer problems, problems without constraints, members
    alone in their group and single-phase members the default route solves alone go through the default route
    one by one.
    pivot_rule: as for mi355x_simplex_solver, for every batch and every member solved alone; an unknown name
    and a rule other than "dantzig" with exact=False are argument errors, and a member with a float declines
    such a rule (its condition takes its slot when errorp is False).
    precision="single" (opt-in; default "double": everything above, unchanged): every member takes the reference's
    single-float path (single.py), what [mi355x_simplex_solver(p, precision="single") for p in problems] returns,
    the solved SingleTableaus with their read-back in np.float32.  Single-phase members are grouped by (shape,
    sense), two-phase members by (artificial shape, main shape, sense) -- no unit-basis restriction -- and a group
    of two or more is ONE batch of single-float tableaux (mi355x_sbatch_create / _solve or _solve_two_phase in
    bounded chunks, one workgroup per member with the member's tableau in LDS).  Members alone in their group,
    shapes beyond the batch's LDS budget and integer problems go one by one; a member with a number no binary32
    holds is declined: unsupported-constraint-error ("single", number) in its slot.  Together with exact,
    native="many", from_rows, device_build, devices > 1 or a pivot_rule other than "dantzig" it is an argument
    error that names the pair; so is an unknown precision.
    beyond_lds=True (opt-in, with precision="single" only -- an argument error otherwise): a group beyond the batch's
    LDS budget with at least single.global_batch_min_members(rows, cols) members is ONE global-form batch (one
    workgroup per member, the member's tableau left in device memory: mi355x_sbatch_create_global) instead of going
    one by one; every member comes back as the same SingleTableau, bit for bit.
    mixed_shapes=True (opt-in, with precision="single" only -- an argument error otherwise): the members are NOT
    grouped by shape and sense; all single-phase members inside the LDS budget are ONE ragged batch
    (mi355x_sbatch_create_ragged: every member its own shape and sense) and all two-phase members ONE ragged pair,
    two or more members each.  Members beyond the budget and integer problems go as without the keyword; every
    member comes back as the same SingleTableau, bit for bit."""
    if precision not in ("double", "single"):
        raise ValueError("precision=%r: \"double\" (default) or \"single\"" % (precision,))
    if beyond_lds and precision != "single":
        raise ValueError("beyond_lds=True needs precision=\"single\": it batches the single-float members beyond the "
                         "LDS budget")
    if mixed_shapes and precision != "single":
        raise ValueError("mixed_shapes=True needs precision=\"single\": it batches the single-float members of "
                         "different shapes and senses")
    if precision == "single":
        given = {"exact": exact, "native": native, "from_rows": from_rows, "device_build": device_build,
                 "devices": devices, "pivot_rule": pivot_rule}
        for name, clash in (("exact", bool(exact)), ("native", native == "many"), ("from_rows", bool(from_rows)),
                            ("device_build", bool(device_build)), ("devices", devices > 1),
                            ("pivot_rule", pivot_rule != "dantzig")):
            if clash:
                raise ValueError("precision=\"single\" does not go with %s=%r: the single-float batch is one device "
                                 "under the reference's rule" % (name, given[name]))
        from .single import solve_problems_single
        kw = {"beyond_lds": True} if beyond_lds else {}                    # (the default: the call as it was)
        if mixed_shapes:
            kw["mixed_shapes"] = True
        return solve_problems_single(problems, fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots,
                                     errorp=errorp, **kw)
    from .exact import pivot_rule_code
    if pivot_rule_code(pivot_rule) != 0 and not exact:
        raise ValueError("pivot_rule=%r needs exact=True: the double-precision paths keep the reference's rule"
                         % (pivot_rule,))
    if device_build and not exact:
        raise ValueError("device_build=True needs exact=True: it builds the tableaux of the exact batches")
    if from_rows and exact:
        raise ValueError("from_rows=True builds the double-precision batches; with exact=True it is device_build=True "
                         "that builds the tableaux on the device")
    if from_rows and native == "many":
        raise ValueError("from_rows=True does not go with native=\"many\": that route builds its members in the library")
    if exact:
        from .exact import solve_problems_exact
        kw = {"device_build": True} if device_build else {}               # (the default: the call as it was)
        return solve_problems_exact(problems, fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots,
                                    errorp=errorp, native=native, min_bits=exact_bits, exact_max_bits=exact_max_bits,
                                    pivot_rule=pivot_rule, **kw)
    from .batch import MultiDeviceBatch
    if native == "many":
        # the whole list behind ONE job of the library (mi355x_simplex_solver_many_*): members come
        # back as NativeSolution objects (the glue's :native :many)
        from .native import solve_many
        return finish(solve_many(problems, fp_tolerance=fp_tolerance, devices=devices, max_pivots=max_pivots), errorp)
    if from_rows:
        from .batch_lps import solve_problems_from_rows

        def host_route(p):
            return mi355x_solve_problems([p], fp_tolerance=fp_tolerance, device=device, devices=devices,
                                         max_pivots=max_pivots, errorp=False, native=native)[0]
        return finish(solve_problems_from_rows(problems, host_route, fp_tolerance=fp_tolerance, device=device,
                                               devices=devices, max_pivots=max_pivots), errorp)
    from .batch_lps import solve_batches
    results = [None] * len(problems)
    groups, groups2 = {}, {}

    def alone(k):
        # (native: what the one-problem hook may return for a member solved alone -- False keeps the
        # list homogeneous, every member a Tableau; "auto" lets lone members take the native route)
        return mi355x_simplex_solver(problems[k], fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots,
                                     native=native)

    for k, p in enumerate(problems):
        if p.integer_vars:
            one_by_one(results, [k], alone)
            continue
        try:
            tabs = build_tableau(p, p, fp_tolerance_factor=fp_tolerance, device=device)
        except SolverError as e:                       # e.g. the unbounded no-constraint special case
            results[k] = e
            continue
        if isinstance(tabs, Tableau) and not _unit_basis(tabs):
            one_by_one(results, [k], alone)
        else:
            file_by_shape(groups, groups2, k, tabs)

    def batch(tabs):
        return MultiDeviceBatch.from_arrays(np.stack([t.matrix for t in tabs]),
                                            np.stack([t.basis_columns for t in tabs]), n_devices=devices)

    def adopt(t, mb, q, st, npv):
        e = _error_for(int(st[q]))
        if e is not None:
            return e
        G, gb = mb.download(q)
        old, t._handle = t._handle, None
        if old:
            capi.lib().mi355x_tab_destroy(old)
        t._matrix, t._basis, t._stale, t._light = G, gb, False, None
        t.n_pivots = member_pivots(npv, q)
        return t

    # a group of two or more is one batch, or for two-phase members a batch of artificial and a batch of main
    # tableaux: phase 1, the per-member step between the phases and phase 2 in bounded calls (solve_batches)
    for members in [*groups.values(), *groups2.values()]:
        ks, mains = [m[0] for m in members], [m[-1] for m in members]
        if len(members) == 1:
            one_by_one(results, ks, alone)
            continue
        amb = batch([m[1] for m in members]) if len(members[0]) == 3 else None
        mmb = batch(mains)
        st, npv = solve_batches(mmb, amb, mains[0].is_max, fp_tolerance, max_pivots)
        place(results, ks, [adopt(t, mmb, q, st, npv) for q, t in enumerate(mains)])
    return finish(results, errorp)


def _unit_basis(tableau):
    """The glue's `unit-basis-p`: every basis column is exactly the unit vector of its row."""
    M, b = tableau.matrix, tableau.basis_columns
    if len(set(b.tolist())) != len(b) or (len(b) and (b.min() < 0 or b.max() >= M.shape[1] - 1)):
        return False
    cols = M[:, b]
    unit = np.zeros_like(cols)
    unit[np.arange(len(b)), np.arange(len(b))] = 1.0
    return bool(np.array_equal(cols, unit) and not np.signbit(cols).any())
