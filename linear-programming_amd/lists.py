"""What the routes behind ``mi355x_solve_problems(list)`` share -- the default route (simplex.py), from_rows
(batch_lps.py), exact (exact.py), exact with device_build (exact_lps.py) and precision="single" (single.py):
the two bounded-call loops, the two groupings, and the placement of results.  Host only; every route keeps its
own plumbing (how a batch is made, what a call passes, how a member's tableau takes its result, who owns the
handles).
"""
import numpy as np

from . import capi
from .conditions import SolverError


# ------------------------------------------------------------------ bounded foreign calls
def chunk_pivots(rows, cols):
    """The glue's `chunk-pivots`: pivots per foreign call, about a tenth to half a second of GPU
    time at every size, so that a single-threaded host is back in its own code (where interrupts
    are served) a few times per second."""
    return max(1024, min(65536, (1 << 36) // max(1, rows * cols)))


def solve_in_chunks(call, rows, cols, max_pivots, chunk=None):
    """The glue's `solve-in-chunks`: call(cap) -> (status, pivots of that call) until the status is
    something else than MI_MAX_PIVOTS or max_pivots (0 = no cap) are used up.  A solve continued
    call by call takes exactly the pivots of one long call.  (chunk: tests force a small one.)"""
    chunk, total = chunk or chunk_pivots(rows, cols), 0
    while True:
        cap = min(chunk, max_pivots - total) if max_pivots > 0 else chunk
        rc, k = call(cap)
        total += k
        if rc != capi.MI_MAX_PIVOTS or (max_pivots > 0 and total >= max_pivots):
            return rc, total


def batch_in_chunks(call, rows, cols, max_pivots, chunk=None):
    """The glue's `multibatch-solve-in-chunks`: call(cap) -> (stop, status[n], pivots[n] or [n, 2] of that call)
    until no member is left at MI_MAX_PIVOTS, max_pivots (0 = no cap) are used up -- counted in the caps granted,
    whatever the members report -- or the call says stop (a route that honours a cancelled call; the others pass
    False).  -> (last statuses, pivots summed per member); the arrays a call returns are left as they are."""
    chunk, done, total = chunk or chunk_pivots(rows, cols), 0, 0
    while True:
        cap = min(chunk, max_pivots - done) if max_pivots > 0 else chunk
        stop, st, npv = call(cap)
        total = total + npv
        done += cap
        if stop or (max_pivots > 0 and done >= max_pivots) or not (st == capi.MI_MAX_PIVOTS).any():
            return st, total


def member_pivots(total, q):
    """Member q's n_pivots of batch_in_chunks' sums: a number, or (phase 1 + drive-outs, phase 2) for a pair."""
    return int(total[q]) if total.ndim == 1 else (int(total[q, 0]), int(total[q, 1]))


# ------------------------------------------------------------------ grouping host-built tableaux
def file_by_shape(groups, groups2, k, tabs):
    """Member k's build-tableau result under its key: a tableau in groups {(shape, is_max): [(k, tableau)]}, a
    two-phase pair (src/simplex.lisp:326-328) in groups2 {(art shape, main shape, is_max): [(k, art, main)]}."""
    if isinstance(tabs, list):
        art, main = tabs
        groups2.setdefault((art.matrix.shape, main.matrix.shape, main.is_max), []).append((k, art, main))
    else:
        groups.setdefault((tabs.matrix.shape, tabs.is_max), []).append((k, tabs))


def pop_singletons(groups):
    """Takes the groups of one member out; -> those members' indices."""
    return [groups.pop(key)[0][0] for key in [key for key, members in groups.items() if len(members) == 1]]


# ------------------------------------------------------------------ grouping lowered rows
SENSES = {"<=": 0, ">=": 1, "=": 2}


def rows_reason(problem):
    """Why a problem without integer variables cannot be lowered to rows (None: it can)."""
    if not problem.constraints:
        return "no constraints"
    if any(op not in SENSES for op, _, _ in problem.constraints):
        return "constraint"
    return None


def row_counts(flip, sense):
    """(`=` rows, artificial rows) per member: flip (... x m) marks the rows with a negative right-hand side, which
    are negated (:243-252), sense (... x m) is SENSES'; a row is artificial when it is `=` or, after the flip, `>=`."""
    op = np.where(sense == 2, 2, np.where(flip, 1 - sense, sense))
    return (sense == 2).sum(axis=-1), (op != 0).sum(axis=-1)


def group_by_rows(lowered, host):
    """lowered: [(k, rows array (m + 1) x (ncv + 1), `=` rows, artificial rows, the member's lowered form with its
    is_max)] in list order -> {(m, ncv, `=` rows, artificial rows, is_max): [(k, lowered form)]}, each of two or
    more members; a member alone in its group goes to host[k] = "alone"."""
    groups = {}
    for k, rows, n_eq, n_art, low in lowered:
        groups.setdefault((rows.shape[0] - 1, rows.shape[1] - 1, int(n_eq), int(n_art), low.is_max), []).append((k, low))
    for k in pop_singletons(groups):
        host[k] = "alone"
    return groups


# ------------------------------------------------------------------ results
def place(results, ks, rs):
    """A group's results into their members' slots."""
    for k, r in zip(ks, rs):
        results[k] = r


def one_by_one(results, ks, solve):
    """Members ks through the route's one-problem solver, solve(k); a member without a solution leaves its
    condition in its slot."""
    for k in ks:
        try:
            results[k] = solve(k)
        except SolverError as e:
            results[k] = e


def finish(results, errorp):
    """The end of every route, after every member has been attempted: errorp raises the first member's
    exception, otherwise the exceptions stay in their slots."""
    if errorp:
        for r in results:
            if isinstance(r, Exception):
                raise r
    return results
