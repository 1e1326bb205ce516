"""Double-precision batches built on the device (opt-in: ``mi355x_solve_problems(ps, from_rows=True)``, and the
array front end ``solve_lps``).

The default list route builds every member's tableau on the host -- build_tableau, a dense [A | I | b] matrix
per member and its artificial twin for a two-phase member -- stacks them and uploads them all.  Here a problem
is only *lowered*: the first stage of build-tableau, the one that needs the problem's names (lowering.lower,
the very function build_tableau starts with: src/simplex.lisp:189-241, :270-283), leaves one row of doubles per
constraint, in column space, and everything after that -- the flip of a negative right-hand side, slack and artificial columns, both
bases, the artificial objective row (:243-328) -- is k_blp_rows / k_assemble / k_art_objective on the
device (mi355x_multibatch_create_lps, csrc/kernels_batch_lps.inc).  What a batch starts from is what
build_tableau produces, bit for bit, so are the pivot sequences and every result.  The exact batches have the
same entry in exact_lps.py.
"""
from collections import namedtuple

import numpy as np

from . import capi, lists
from .batch import MultiDeviceBatch
from .lists import SENSES                                     # noqa: F401
from .lowering import DOUBLE, lower

LoweredRows = namedtuple("LoweredRows", "L sense mapping is_max")


def host_reason(problem):
    """Why a problem stays on the default route (None: lower_problem_rows takes it)."""
    return "integer variables" if problem.integer_vars else lists.rows_reason(problem)


def lower_problem_rows(problem):
    """lowering.lower in doubles, the first stage of build_tableau: (L, sense, mapping, is_max) with L a float64
    array (m + 1) x (ncv + 1) -- per constraint the structural coefficients and the right-hand side less the
    offsets, then the objective row with its signs applied and its constant -- sense an int32 array (0 `<=`,
    1 `>=`, 2 `=`), mapping build_tableau's var_mapping.  None for what stays on the default route
    (host_reason)."""
    if host_reason(problem) is not None:
        return None
    L, _, constraints, mapping = lower(problem, DOUBLE)
    sense = np.array([SENSES[op] for op, _, _ in constraints], dtype=np.int32)
    return LoweredRows(L, sense, mapping, problem.type == "max")


def row_counts(L, sense):
    """(`=` rows, artificial rows, negated rows) per member of L (... x (m + 1) x (ncv + 1)) and sense (... x m): a
    row is negated when its right-hand side is < 0.0 (:243-252; not -0.0, not NaN), and artificial when it is
    `=` or, after the flip, `>=`."""
    flip = L[..., :-1, -1] < 0.0
    return (*lists.row_counts(flip, sense), flip.sum(axis=-1))


def group_lowered_rows(problems):
    """The grouping of mi355x_solve_problems(from_rows=True), host only: (host, groups).  host {k: why the member
    goes through the default route} -- host_reason's words, "basis" for a single-phase member the default
    route solves alone as well (a negated row leaves -0.0 in the other rows' slack columns: not the unit basis
    its batches start from, simplex._unit_basis), "alone" for a member alone in its group; groups {(m, ncv, `=`
    rows, artificial rows, is_max): [(k, LoweredRows)]}, each of two or more members."""
    host, lowered = {}, []
    for k, p in enumerate(problems):
        low = lower_problem_rows(p)
        if low is None:
            host[k] = host_reason(p)
            continue
        n_eq, n_art, n_flip = (int(x) for x in row_counts(low.L, low.sense))
        if n_art == 0 and n_flip > 0 and len(low.sense) > 1:
            host[k] = "basis"
            continue
        lowered.append((k, low.L, n_eq, n_art, low))
    return host, lists.group_by_rows(lowered, host)


def solve_batches(main, art, is_max, fp_tolerance=1024, max_pivots=0):
    """A created group in bounded calls (the glue's `multibatch-solve-in-chunks`: lists.batch_in_chunks), what
    mi355x_solve_problems does with its host-built groups as well: single phase (art None), or phase 1 on the
    artificial batch, the per-member step between the phases (mi355x_multibatch_two_phase_handover) and phase 2 on
    the main batch; max_pivots caps every phase.
    -> (status per member, pivots per member: n, or n x 2 for a two-phase group)."""
    first = main if art is None else art

    def phase(mb, is_max):
        return lists.batch_in_chunks(
            lambda cap: (False,) + mb.solve(is_max=is_max, fp_tolerance=fp_tolerance, max_pivots=cap),
            first.rows, first.cols, max_pivots)
    if art is None:
        return phase(main, is_max)
    st1, np1 = phase(art, False)
    between, nd = art.two_phase_handover(main, fp_tolerance=fp_tolerance, phase1_status=st1)
    st2, np2 = phase(main, is_max)
    return np.where(between == capi.MI_OK, st2, between).astype(np.int32), np.stack([np1 + nd, np2], axis=1)


def solve_group(problems, lowered, fp_tolerance=1024, device=0, devices=1, max_pivots=0):
    """One group of group_lowered_rows: per member the solved (main) Tableau the default route returns -- matrix,
    basis, n_pivots, var_mapping -- or the exception of its outcome."""
    from .simplex import Tableau, _error_for
    main, art = MultiDeviceBatch.from_lps(np.stack([l.L for l in lowered]), np.stack([l.sense for l in lowered]),
                                          n_devices=devices)
    st, npv = solve_batches(main, art, lowered[0].is_max, fp_tolerance, max_pivots)
    out = []
    for q, (p, low) in enumerate(zip(problems, lowered)):
        r = _error_for(int(st[q]))
        if r is None:
            G, gb = main.download(q)
            r = Tableau(p, p, G, gb, main.cols - 1, main.rows - 1, low.mapping, fp_tolerance, device)
            r.n_pivots = lists.member_pivots(npv, q)
        out.append(r)
    return out


def solve_problems_from_rows(problems, host_route, fp_tolerance=1024, device=0, devices=1, max_pivots=0):
    """mi355x_solve_problems(from_rows=True) less its last step: the list of results (a solved Tableau or the
    member's exception).  host_route(problem) -> that member's result by the default route; it gets the members
    group_lowered_rows names, one by one."""
    results = [None] * len(problems)
    host, groups = group_lowered_rows(problems)
    for members in groups.values():
        ks = [k for k, _ in members]
        lists.place(results, ks, solve_group([problems[k] for k in ks], [l for _, l in members], fp_tolerance, device,
                                             devices, max_pivots))
    for k in sorted(host):
        results[k] = host_route(problems[k])
    return results


# ------------------------------------------------------------------ the array front end
def solve_lps(lps, sense, is_max=True, fp_tolerance=1024, devices=1, max_pivots=0):
    """One group given as arrays -- lps n x (m + 1) x (ncv + 1) float64 in column space (per member m rows of ncv
    coefficients and the right-hand side, then the objective row as build-tableau stores it: -c for max / min
    c . x over x >= 0, the constant last), sense n x m (0 `<=`, 1 `>=`, 2 `=`), every member with the same numbers
    of `=` and of artificial rows: mi355x_multibatch_create_lps, the bounded solve calls of solve_batches and ONE
    read-back.  No Python runs per entry and no matrix comes back.  -> (statuses n, pivots n or n x 2 for a
    two-phase group, last rows n x cols, last columns n x rows, bases n x m): the objective value of member q is
    last_rows[q, -1], the value of column j last_cols[q, i] where bases[q, i] == j (0 otherwise), its reduced
    cost last_rows[q, j].  A member that did not end MI_OPTIMAL has no meaningful values."""
    main, art = MultiDeviceBatch.from_lps(lps, sense, n_devices=devices)
    st, npv = solve_batches(main, art, is_max, fp_tolerance, max_pivots)
    last_rows, last_cols, bases = main.readback()
    return st, npv, last_rows, last_cols, bases
