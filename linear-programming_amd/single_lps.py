"""Single-float batches built on the device from problem rows (opt-in: ``solve_problems_single_from_rows`` and the
array front end ``solve_lps_single``) -- the single-float twin of batch_lps.py.

``solve_problems_single`` builds every member's tableau on the host: build_tableau_single, a dense [A | I | b]
matrix of Lisp numbers per member and its artificial twin for a two-phase member, coerced entry by entry, stacked
and uploaded.  Here a problem is only *lowered* (lowering.lower with SINGLE: src/simplex.lisp:189-241, :270-283),
which leaves one row per constraint in column space, and everything after that -- the flip of a negative right-hand
side, slack and artificial columns, both bases, the artificial objective row (:243-328) -- is k_slp_assemble on the
device (mi355x_sbatch_create_lps, csrc/kernels_single_lps.inc).  What a batch starts from is what
build_tableau_single produces, bit for bit, sign of zero included; so are the pivot sequences and every result.

Two things the float rows cannot say keep a member on the host route:
  "float zero"    Lisp negates a row with a negative right-hand side entry by entry: an INTEGER zero stays 0 (+0.0
                  once coerced), a single-float zero the user wrote (``0.0``) becomes -0.0.  The device reads every
                  zero of a negated row as an integer zero.
  "integer sum"   Lisp keeps integers exact among themselves in the sum of the artificial objective row; the device
                  sums floats.  The two agree while, per column, the absolute values of the integer entries sum to
                  at most 2**24 (the guard of mi355x_sbatch_create_lps).
"""
from collections import namedtuple

import numpy as np

from . import capi, lists, single
from .batch_lps import host_reason
from .conditions import SolverError
from .lists import SENSES
from .lowering import lower
from .single import SINGLE, SingleBatch, SingleTableau, check_single_problem, solve_made_batches, solve_single

LoweredRowsSingle = namedtuple("LoweredRowsSingle", "L sense mapping is_max col_int_sum float_zero")

#: the integers a float holds exactly: |x| <= 2**24
EXACT_INTS = 2.0 ** 24


def lower_problem_rows_single(problem):
    """check_single_problem, then lowering.lower under Lisp's contagion, the first stage of build_tableau_single:
    (L, sense, mapping, is_max, col_int_sum, float_zero) with L a float32 array (m + 1) x (ncv + 1) -- per
    constraint the structural coefficients and the right-hand side less the offsets, then the objective row with
    its signs applied and its constant -- sense an int32 array (0 `<=`, 1 `>=`, 2 `=`), mapping
    build_tableau_single's var_mapping, col_int_sum per column the sum of the absolute values of the entries Lisp
    holds as integers, over the constraint rows (float64, capped at 2**63), float_zero whether a row with a negative
    right-hand side holds a single-float zero.  None for what stays on the host route (batch_lps.host_reason); a
    number that does not qualify raises check_single_problem's condition."""
    if host_reason(problem) is not None:
        return None
    check_single_problem(problem)
    Lo, _, constraints, mapping = lower(problem, SINGLE)
    m = len(constraints)
    values = [x.v for x in Lo.flat]
    L = np.array(values, dtype=np.float32).reshape(Lo.shape)
    is_int = np.array([type(v) is int for v in values], dtype=bool).reshape(Lo.shape)
    W = Lo.shape[1]
    sums = [sum(abs(v) for v in values[c:m * W:W] if type(v) is int) for c in range(W)]
    col_int_sum = np.array([min(float(s), 2.0 ** 63) for s in sums], dtype=np.float64)
    negated = L[:m, -1] < 0
    float_zero = bool(((L[:m] == 0) & ~is_int[:m])[negated].any())
    sense = np.array([SENSES[op] for op, _, _ in constraints], dtype=np.int32)
    return LoweredRowsSingle(L, sense, SINGLE.mapping(mapping), problem.type == "max", col_int_sum, float_zero)


def lower_list_single(problems):
    """The first half of group_lowered_rows_single, host only: (host, lowered).  host {k: why the member goes one by
    one} as there, without "alone"; lowered [(k, rows, `=` rows, artificial rows, LoweredRowsSingle)] in list order,
    what lists.group_by_rows takes."""
    host, lowered = {}, []
    for k, p in enumerate(problems):
        try:
            low = lower_problem_rows_single(p)
        except SolverError as e:
            host[k] = e
            continue
        if low is None:
            host[k] = host_reason(p)
        elif low.float_zero:
            host[k] = "float zero"
        elif (low.col_int_sum > EXACT_INTS).any():
            host[k] = "integer sum"
        else:
            n_eq, n_art = lists.row_counts(low.L[:-1, -1] < 0, low.sense)
            lowered.append((k, low.L, n_eq, n_art, low))
    return host, lowered


def group_lowered_rows_single(problems):
    """The grouping of solve_problems_single_from_rows, host only: (host, groups).  host {k: why the member goes one
    by one} -- batch_lps.host_reason's words, "float zero" and "integer sum" (the module docstring), "alone" for a
    member alone in its group, or the condition check_single_problem raised (it stays in the member's slot);
    groups {(m, ncv, `=` rows, artificial rows, is_max): [(k, LoweredRowsSingle)]}, each of two or more members.
    There is no "basis" reason: the single-float path has no compact form."""
    host, lowered = lower_list_single(problems)
    return host, lists.group_by_rows(lowered, host)


#: mixed_shapes=True: the fewest members that make a device-built ragged batch (or pair): a batch of one member gains
#: nothing, so two.  What was measured by member count is in DESIGN 4.6n.
RAGGED_ROWS_MIN_MEMBERS = 2


def take_rows_for_ragged(lowered):
    """Takes out of lowered (lower_list_single's) the members that go as device-built ragged batches under
    mixed_shapes=True: those whose tableau -- for a member with artificial rows the artificial one -- is inside the
    LDS budget, except the (m, ncv, `=` rows, artificial rows, sense) groups that single.RAGGED_UNIFORM_MIN_MEMBERS
    keeps as batches of one shape.  -> (what is left, the single-phase set, the two-phase set), each set in list order
    and of RAGGED_ROWS_MIN_MEMBERS or more members, else empty and its members left."""
    sizes = {}
    for k, rows, n_eq, n_art, low in lowered:
        key = (rows.shape, int(n_eq), int(n_art), low.is_max)
        sizes[key] = sizes.get(key, 0) + 1
    sets, rest = ([], []), []
    for item in lowered:
        k, rows, n_eq, n_art, low = item
        m, ncv = rows.shape[0] - 1, rows.shape[1] - 1
        uniform = single.RAGGED_UNIFORM_MIN_MEMBERS is not None and \
            sizes[(rows.shape, int(n_eq), int(n_art), low.is_max)] >= single.RAGGED_UNIFORM_MIN_MEMBERS
        if uniform or single.single_lds_bytes(m + 1, ncv + (m - int(n_eq)) + 1 + int(n_art)) > single.LDS_BUDGET:
            rest.append(item)
        else:
            sets[1 if n_art else 0].append(item)
    out = []
    for members in sets:
        if len(members) < RAGGED_ROWS_MIN_MEMBERS:
            rest.extend(members)
            members = []
        out.append(members)
    return sorted(rest, key=lambda item: item[0]), out[0], out[1]


def solve_problems_single_from_rows(problems, fp_tolerance=1024, device=0, max_pivots=0, errorp=True, chunk=None,
                                    beyond_lds=False, mixed_shapes=False):
    """What solve_problems_single(problems, ...) returns, member for member -- the solved SingleTableau (matrix,
    basis, n_pivots, var_mapping, read-back in np.float32) or the member's condition -- with the tableaux of every
    group of group_lowered_rows_single built on the device (SingleBatch.from_lps) and solved in bounded chunks.
    The members that function names, and the groups the batch declines (MI_UNSUPPORTED: the LDS budget), go
    through solve_single one by one.
    beyond_lds=True (opt-in): a group the LDS batch declines that has at least single.global_batch_min_members(rows,
    cols) members (for a two-phase group: of the artificial shape) is built on the device all the same, as ONE
    global-form batch or pair (SingleBatch.from_lps(form="global")); the results are the same, bit for bit.
    mixed_shapes=True (opt-in): the members inside the LDS budget are not grouped by shape and sense -- all
    single-phase ones go as ONE device-built ragged batch, all two-phase ones as ONE device-built ragged pair
    (SingleBatch.from_lps_ragged; take_rows_for_ragged), in bounded chunks sized by the largest member; everything
    else goes as above, and the results are the same, bit for bit."""
    results = [None] * len(problems)
    if mixed_shapes:
        host, lowered = lower_list_single(problems)
        lowered, *ragged_sets = take_rows_for_ragged(lowered)
        groups = lists.group_by_rows(lowered, host)
    else:
        (host, groups), ragged_sets = group_lowered_rows_single(problems), ()

    def alone(k):
        return solve_single(problems[k], fp_tolerance=fp_tolerance, device=device, max_pivots=max_pivots, chunk=chunk)

    def taker(ks, lows):
        def take(sb, q, n_pivots):
            p = problems[ks[q]]
            M, b = sb.download(q)
            t = SingleTableau(p, p, M, b, M.shape[1] - 1, M.shape[0] - 1, lows[q].mapping, fp_tolerance, device)
            t.n_pivots = n_pivots
            return t
        return take

    for k in sorted(host):
        if isinstance(host[k], Exception):
            results[k] = host[k]
        else:
            lists.one_by_one(results, [k], alone)
    for members in ragged_sets:
        if not members:
            continue
        ks, lows = [item[0] for item in members], [item[-1] for item in members]
        try:
            main, art = SingleBatch.from_lps_ragged([low.L for low in lows], [low.sense for low in lows],
                                                    [low.is_max for low in lows], [low.col_int_sum for low in lows],
                                                    device=device)
        except capi.Mi355xError as e:                                     # declined all the same: one by one
            if e.code != capi.MI_UNSUPPORTED:
                raise
            lists.one_by_one(results, ks, alone)
            continue
        lists.place(results, ks, solve_made_batches([main] if art is None else [art, main], -1, taker(ks, lows),
                                                    fp_tolerance, max_pivots, chunk))
    for members in groups.values():
        ks, lows = [k for k, _ in members], [low for _, low in members]
        arrays = (np.stack([low.L for low in lows]), np.stack([low.sense for low in lows]),
                  np.stack([low.col_int_sum for low in lows]))

        def make(form="lds"):
            """(main, art or None), or None when the form declines the shape."""
            try:
                return SingleBatch.from_lps(*arrays, device=device, **({"form": form} if form != "lds" else {}))
            except capi.Mi355xError as e:
                if e.code != capi.MI_UNSUPPORTED:
                    raise
                return None
        made = make()
        if made is None and beyond_lds:
            m, ncv = arrays[0].shape[1] - 1, arrays[0].shape[2] - 1
            n_eq, n_art = (int(x[0]) for x in lists.row_counts(arrays[0][:1, :-1, -1] < 0, arrays[1][:1]))
            if len(ks) >= single.global_batch_min_members(m + 1, ncv + (m - n_eq) + 1 + n_art):
                made = make("global")
        if made is None:
            lists.one_by_one(results, ks, alone)
            continue
        main, art = made
        lists.place(results, ks, solve_made_batches([main] if art is None else [art, main], lows[0].is_max,
                                                    taker(ks, lows), fp_tolerance, max_pivots, chunk))
    return lists.finish(results, errorp)


# ------------------------------------------------------------------ the array front end
def solve_lps_single(lps, sense, is_max=True, int_mask=None, fp_tolerance=1024, device=0, max_pivots=0, form="lds"):
    """One group given as arrays, the float twin of batch_lps.solve_lps -- lps n x (m + 1) x (ncv + 1) float32 in
    column space (per member m rows of ncv coefficients and the right-hand side, then the objective row as
    build-tableau stores it: -c for max / min c . x over x >= 0, the constant last), sense n x m (0 `<=`, 1 `>=`,
    2 `=`), every member with the same numbers of `=` and of artificial rows: mi355x_sbatch_create_lps, the bounded
    solve calls and ONE mi355x_sbatch_readback.  No Python runs per entry and no matrix comes back.
    int_mask (the shape of lps, or None: no entry is an integer) marks the entries Lisp holds as INTEGERS; the
    guard's col_int_sum is computed from it, and a group with an integer column sum beyond 2**24 is declined
    (capi.Mi355xError, MI_UNSUPPORTED).  ZEROS ARE READ AS INTEGER ZEROS whatever int_mask says: a zero in a row
    with a negative right-hand side comes out +0.0, where Lisp makes -0.0 of a single-float zero.
    -> (statuses n, pivots n or n x 2 for a two-phase group, rhs n x (m + 1), obj_rows n x cols, bases n x m): the
    objective value of member q is obj_rows[q, -1], the value of column j rhs[q, i] where bases[q, i] == j (0
    otherwise), its reduced cost obj_rows[q, j].  A member that did not end MI_OPTIMAL has no meaningful values.
    form="global" (opt-in): the group as global-form batches (mi355x_sbatch_create_lps_global), for members beyond the
    LDS budget; the caller chooses, no member-count rule applies here."""
    from .single_bb import readback
    if form not in ("lds", "global"):
        raise ValueError("form=%r: \"lds\" (default) or \"global\"" % (form,))
    L = np.asarray(lps)
    sums = None
    if int_mask is not None:
        mask = np.asarray(int_mask, dtype=bool)
        if mask.shape != L.shape:
            raise ValueError("int_mask shape %r does not match lps %r" % (mask.shape, L.shape))
        sums = np.where(mask[:, :-1, :], np.abs(L[:, :-1, :].astype(np.float64)), 0.0).sum(axis=1)
    main, art = SingleBatch.from_lps(L, sense, sums, device=device, **({"form": form} if form != "lds" else {}))
    made = [main] if art is None else [art, main]
    try:
        first = made[0]
        st, npv = lists.batch_in_chunks(
            lambda cap: (False,) + (art.solve_two_phase(main, is_max, fp_tolerance, cap) if art is not None else
                                    main.solve(is_max, fp_tolerance, cap)), first.rows, first.cols, max_pivots)
        rhs, obj_rows, bases = readback(main)
        return st, npv, rhs, obj_rows, bases
    finally:
        for b in made:
            b.close()
