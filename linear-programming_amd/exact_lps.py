"""Exact batches built on the device (opt-in: ``mi355x_solve_problems(ps, exact=True, device_build=True)``,
and the array front end ``solve_lps_exact``).

The default exact route builds every member's tableau on the host -- build_tableau(exact=True), one Fraction
per entry -- and uploads it, with its artificial twin for a two-phase member.  Here a problem is only
*lowered*: the first stage of build-tableau, the one that needs the problem's names (lowering.lower, the very
function build_tableau(exact=True) starts with: src/simplex.lisp:189-241, :270-283), leaves one row of
numerators and denominators per constraint, in column space, and everything after that -- the flip of a negative right-hand side, slack and
artificial columns, the artificial objective row, the integer scale (:243-328 and x_start_state) -- is
k_xb_assemble_lps on the device (mi355x_xbatch_create_lps, csrc/kernels_exact_lps.inc).  The members a batch
solves are the ones the default route solves, entry for entry, so are the pivot sequences and every result.
(One limit of the default route does not exist here: it declines a member whose artificial objective row, a
sum of coefficients, holds a numerator or denominator beyond 64 bits, because that row crosses the boundary;
here only the problem's own coefficients do.)
"""
import ctypes
from collections import namedtuple
from fractions import Fraction

import numpy as np

from . import capi, lists
from .conditions import UnsupportedConstraintError
from .exact import (ExactTableau, XBatch, _I64_MAX, _check_widths, _declined, _member_error, _ptr, batch_in_chunks,
                    pivot_rule_code, rational_problem)
from .lists import SENSES                                     # noqa: F401
from .lowering import EXACT, lower
from .problem import Problem

Lowered = namedtuple("Lowered", "num den sense mapping is_max")


def host_reason(problem):
    """Why a problem stays on the host-built route (None: lower_problem takes it)."""
    if problem.integer_vars:
        return "integer variables"
    if not rational_problem(problem):
        return "float"
    return lists.rows_reason(problem)


def _check64(x):
    if abs(x.numerator) > _I64_MAX or x.denominator > _I64_MAX:
        raise _declined(("coefficient", str(x)))


def lower_problem(problem):
    """lowering.lower in Fractions as what crosses the boundary: (num, den, sense, mapping, is_max) with num /
    den int64 arrays (m + 1) x (ncv + 1) -- per constraint the structural coefficients and the right-hand side
    less the offsets, then the objective row with its signs applied and its constant -- sense an int32 array
    (0 `<=`, 1 `>=`, 2 `=`), mapping build_tableau's var_mapping.  Raises the ("exact", "coefficient", ...)
    decline for a value beyond 64 bits as it is stored (also one that a later term of the same variable
    replaces); None for what stays on the host route (host_reason)."""
    if host_reason(problem) is not None:
        return None
    L, _, constraints, mapping = lower(problem, EXACT, stored=_check64)
    flat = L.ravel().tolist()                                             # (every stored value has been checked)
    num = np.array([x.numerator for x in flat], dtype=np.int64).reshape(L.shape)
    den = np.array([x.denominator for x in flat], dtype=np.int64).reshape(L.shape)
    sense = np.array([SENSES[op] for op, _, _ in constraints], dtype=np.int32)
    return Lowered(num, den, sense, EXACT.mapping(mapping), problem.type == "max")


def row_counts(num, sense):
    """(`=` rows, artificial rows) per member of num (... x (m + 1) x (ncv + 1)) and sense (... x m): a row is
    artificial when it is `=` or, after the flip of a negative right-hand side (:243-252), `>=`."""
    return lists.row_counts(num[..., :-1, -1] < 0, sense)


def group_lowered(problems):
    """The grouping of mi355x_solve_problems(exact=True, device_build=True), host only: (host, groups).
    host {k: why the member goes through the host-built route} -- host_reason's words, "coefficient" for a value
    beyond 64 bits, "alone" for a member alone in its group; groups {(m, ncv, `=` rows, artificial rows, is_max):
    [(k, Lowered)]}, each of two or more members."""
    host, lowered = {}, []
    for k, p in enumerate(problems):
        why = host_reason(p)
        if why is None:
            try:
                low = lower_problem(p)
            except UnsupportedConstraintError:
                why = "coefficient"
        if why is not None:
            host[k] = why
            continue
        lowered.append((k, low.num, *row_counts(low.num, low.sense), low))
    return host, lists.group_by_rows(lowered, host)


def create_lps(num, den, sense, device=0, min_bits=0, pivot_rule="dantzig"):
    """mi355x_xbatch_create_lps for members of one group (num, den: n x (m + 1) x (ncv + 1) int64, sense: n x m):
    (main XBatch, artificial XBatch or None), both with pivot_rule set.  Raises the ("exact", "batch", "shape",
    ...) decline for a shape the batch does not take."""
    pivot_rule_code(pivot_rule)
    num = np.ascontiguousarray(num, dtype=np.int64)
    den = np.ascontiguousarray(den, dtype=np.int64)
    sense = np.ascontiguousarray(sense, dtype=np.int32)
    n, rows, w = num.shape
    m, ncv = rows - 1, w - 1
    n_eq, n_art = (int(x) for x in row_counts(num[0], sense[0])) if m > 0 else (0, 0)
    cols = ncv + (m - n_eq) + 1
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    rc = capi.lib().mi355x_xbatch_create_lps(ctypes.byref(hm), ctypes.byref(ha), n, m, ncv, _ptr(num), _ptr(den),
                                             _ptr(sense), device, int(min_bits))
    if rc == capi.MI_UNSUPPORTED:
        raise _declined(("batch", "shape", rows, cols + n_art))
    capi.check(rc, "mi355x_xbatch_create_lps")
    main = XBatch.from_handle(hm, n, rows, cols)
    art = XBatch.from_handle(ha, n, rows, cols + n_art) if ha else None      # (owned from here on)
    main.set_pivot_rule(pivot_rule)
    if art:
        art.set_pivot_rule(pivot_rule)
    return main, art


def _member_tableau(problem, inst, mapping, batch, q, device, min_bits):
    """Member q of a batch as an ExactTableau whose matrix comes with the first read."""
    R, C = batch.rows, batch.cols
    t = ExactTableau.__new__(ExactTableau)
    t.problem, t.instance_problem = problem, inst
    t.var_count, t.constraint_count, t.var_mapping = C - 1, R - 1, mapping
    t.device, t.min_bits, t.max_bits = device, int(min_bits), 128
    t.n_pivots, t.phase1, t._handle = 0, None, None
    t._matrix, t._basis = np.empty((R, C), dtype=object), np.empty(R - 1, dtype=np.int64)
    t._batch, t._stale = (batch, q), True
    return t


def solve_group(problems, lowered, device=0, max_pivots=0, min_bits=0, chunk=None, pivot_rule="dantzig"):
    """One group of group_lowered in bounded calls: per member the solved (main) ExactTableau, backed by its
    batch slot, the exception of its outcome, or None for a member that ended MI_EXACT_OVERFLOW (the caller
    sends it through the host-built route).  Raises the decline of create_lps."""
    num = np.stack([l.num for l in lowered])
    den = np.stack([l.den for l in lowered])
    sense = np.stack([l.sense for l in lowered])
    main, art = create_lps(num, den, sense, device=device, min_bits=min_bits, pivot_rule=pivot_rule)
    st, total = batch_in_chunks(art or main, main if art else None, lowered[0].is_max, max_pivots, chunk)
    out = []
    for q, (p, low) in enumerate(zip(problems, lowered)):
        if st[q] == capi.MI_EXACT_OVERFLOW:
            out.append(None)
            continue
        e = _member_error(capi.MI_CANCELLED if st[q] == capi.MI_RUNNING else st[q])
        if e is not None:
            out.append(e)
            continue
        t = _member_tableau(p, p, low.mapping, main, q, device, min_bits)
        if art:
            t.phase1 = _member_tableau(p, Problem(type="min", vars=list(p.vars)), low.mapping, art, q, device, min_bits)
        t.n_pivots = lists.member_pivots(total, q)
        out.append(t)
    return out


def solve_problems_device_built(problems, host_route, device=0, max_pivots=0, min_bits=0, chunk=None,
                                pivot_rule="dantzig"):
    """mi355x_solve_problems(exact=True, device_build=True) less its last step: the list of results (a solved
    ExactTableau or the member's exception).  host_route(list of problems) -> their results by the default
    route; it gets the members group_lowered names, the groups the batch declines, and the members that
    ended MI_EXACT_OVERFLOW."""
    results = [None] * len(problems)
    host, groups = group_lowered(problems)
    back = sorted(host)
    for members in groups.values():
        ks = [k for k, _ in members]
        try:
            rs = solve_group([problems[k] for k in ks], [l for _, l in members], device, max_pivots, min_bits, chunk,
                             pivot_rule)
        except UnsupportedConstraintError:              # a shape the batch declines
            back += ks
            continue
        lists.place(results, ks, rs)
        back += [k for k, r in zip(ks, rs) if r is None]
    back.sort()
    if back:
        lists.place(results, back, host_route([problems[k] for k in back]))
    return results


# ------------------------------------------------------------------ the array front end
LpResult = namedtuple("LpResult", "status objective x reduced_costs pivots")


def _fractions(a, what):
    """An operand -- an integer array or a (num, den) pair -- as reduced int64 numerators and denominators."""
    if isinstance(a, tuple):
        n, d = (np.asarray(x) for x in a)
    else:
        n = np.asarray(a)
        d = np.ones_like(n)
    for x in (n, d):
        ok = x.dtype.kind in "iu"
        if ok and x.size and x.dtype.itemsize == 8:                         # (|x| <= 2^63 - 1)
            ok = int(x.max()) <= _I64_MAX and (x.dtype.kind == "u" or int(x.min()) >= -_I64_MAX)
        if not ok:
            raise ValueError("%s: integers of at most 64 bits are needed" % what)
    n, d = np.broadcast_arrays(n.astype(np.int64), d.astype(np.int64))
    if (d == 0).any():
        raise ValueError("%s: a denominator is zero" % what)
    g = np.gcd(n, d)
    g = np.where(d < 0, -g, g)
    return n // g, d // g


def solve_lps_exact(a, b, c, sense, c0=None, is_max=True, device=0, max_pivots=0, min_bits=0, chunk=None,
                    pivot_rule="dantzig"):
    """Batches of  max / min c . x + c0  subject to  A x (<=, >=, =) b,  x >= 0,  given as arrays: a (n x m x k), b
    (n x m), c (n x k), c0 (n, optional), each an integer array or a (num, den) pair of them; sense (n x m): 0
    `<=`, 1 `>=`, 2 `=`.  The fractions are reduced with numpy, the members grouped by their numbers of `=` and
    of artificial rows, and each group is one mi355x_xbatch_create_lps + bounded solve calls + one light
    read-back: no Python runs per entry.  Returns per member an LpResult: the MI_* status, and for MI_OPTIMAL
    the objective value, x and the reduced costs as Fractions (None otherwise), and the pivots (two-phase
    groups: (phase 1, phase 2))."""
    from .exact_bb import readback
    _check_widths(min_bits, 128)
    pivot_rule_code(pivot_rule)
    an, ad = _fractions(a, "a")
    if an.ndim != 3 or an.shape[1] < 1 or an.shape[2] < 1:
        raise ValueError("a: an n x m x k array with m >= 1 and k >= 1 is needed")
    n, m, k = an.shape
    bn, bd = _fractions(b, "b")
    cn, cd = _fractions(c, "c")
    zn, zd = _fractions(np.zeros(n, dtype=np.int64) if c0 is None else c0, "c0")
    sense = np.ascontiguousarray(sense, dtype=np.int32)
    if bn.shape != (n, m) or cn.shape != (n, k) or zn.shape != (n,) or sense.shape != (n, m):
        raise ValueError("b, c, c0 and sense must be n x m, n x k, n and n x m")
    if ((sense < 0) | (sense > 2)).any():
        raise ValueError("sense: 0 `<=`, 1 `>=` or 2 `=`")
    num = np.empty((n, m + 1, k + 1), dtype=np.int64)
    den = np.empty((n, m + 1, k + 1), dtype=np.int64)
    num[:, :m, :k], den[:, :m, :k] = an, ad
    num[:, :m, k], den[:, :m, k] = bn, bd
    num[:, m, :k], den[:, m, :k] = -cn, cd                                 # (:270-283: -c for a positive variable)
    num[:, m, k], den[:, m, k] = zn, zd
    n_eq, n_art = row_counts(num, sense)
    results = [None] * n
    for key in sorted(set(zip(n_eq.tolist(), n_art.tolist()))):
        ks = np.nonzero((n_eq == key[0]) & (n_art == key[1]))[0]
        main, art = create_lps(num[ks], den[ks], sense[ks], device=device, min_bits=min_bits, pivot_rule=pivot_rule)
        try:
            st, total = batch_in_chunks(art or main, main if art else None, is_max, max_pivots, chunk)
            light = readback(main)
        finally:
            main.close()
            if art:
                art.close()
        for q, i in enumerate(ks.tolist()):
            status = int(capi.MI_CANCELLED if st[q] == capi.MI_RUNNING else st[q])
            pivots = tuple(int(x) for x in total[q]) if art else int(total[q])
            if status == capi.MI_OPTIMAL and light[q] is None:
                status = capi.MI_EXACT_OVERFLOW
            if status != capi.MI_OPTIMAL:
                results[i] = LpResult(status, None, None, None, pivots)
                continue
            D, rhs, obj, basis = light[q]
            where = {}
            for pos, col in enumerate(basis.tolist()):
                where.setdefault(col, pos)                                  # `position`: the first match
            x = [Fraction(rhs[where[j]], D) if j in where else Fraction(0) for j in range(k)]
            results[i] = LpResult(status, Fraction(obj[-1], D), x, [Fraction(obj[j], D) for j in range(k)], pivots)
    return results
