"""Cases of the single-float batches built from problem rows (tests/test_single_lps_host.py and
tests/test_gpu_single_lps.py), and a plain-NumPy restatement of what the device makes of a member's rows.

The yardstick is the float32 model of tests/single_cases.py (`build`, `solve`, `two_phase`): every case is a problem
dict of that module, so the model builds and solves it by itself, with Lisp's contagion on exact ints and
single-floats.  Nothing here touches the library.

    assemble_rows        rules (a)-(c) of mi355x_sbatch_create_lps on a member's float32 rows, in NumPy
    lds_bytes / fits     the LDS footprint of a member in the batch's solve (single_lds_bytes) and the budget
    *_group(s)           lists of problem dicts that form ONE group each (same m, ncv, `=` rows, artificial rows, sense)
"""
import functools

import numpy as np

from tests import single_cases as sc

F32 = np.float32
EXACT_INTS = 2 ** 24
LDS_BUDGET = 156 * 1024


def to_problem(lp, d, integer_vars=()):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[(b[0], (b[1], b[2])) for b in d.get("bounds", [])],
                      constraints=list(d["constraints"]), integer_vars=list(integer_vars))


# ------------------------------------------------------------------ the rules, restated
def assemble_rows(L, sense, col_int_sum=None, guard=True):
    """A member's rows (m + 1) x (ncv + 1) float32 and senses -> (main, main basis, art or None, art basis or None),
    or None when the guard declines the member.
    (a) a row with right-hand side < 0 is negated and its sense flipped; a zero of it stays +0.0, and so do its slack
        columns (Lisp negates integer zeros there);
    (b) artificial columns in decreasing row order; the artificial objective row per column the float32 sum of the
        artificial rows in increasing row order from +0.0, one rounded addition per row;
    (c) col_int_sum (per column the sum of |integer entries|) beyond 2**24 in any column: declined."""
    L, sense = np.asarray(L), np.asarray(sense)
    assert L.dtype == np.float32
    if guard and col_int_sum is not None and (np.asarray(col_int_sum, dtype=np.float64) > EXACT_INTS).any():
        return None
    m, ncv = L.shape[0] - 1, L.shape[1] - 1
    flip = L[:m, -1] < F32(0)
    op = np.where(sense == 2, 2, np.where(flip, 1 - sense, sense))
    has_slack = sense != 2
    cols = ncv + int(has_slack.sum()) + 1
    M = np.zeros((m + 1, cols), dtype=F32)
    M[:, :ncv], M[:, -1] = L[:, :ncv], L[:, -1]
    basis = np.zeros(m, dtype=np.int64)
    scol = ncv + np.cumsum(has_slack) - has_slack
    for r in range(m):
        if flip[r]:
            M[r] = np.where(M[r] == 0, F32(0), -M[r])
        if op[r] != 2:
            M[r, scol[r]] = F32(1) if op[r] == 0 else F32(-1)
        basis[r] = scol[r] if op[r] == 0 else cols
    art_rows = [r for r in range(m) if op[r] != 0]
    if not art_rows:
        return M, basis, None, None
    A = np.zeros((m + 1, cols + len(art_rows)), dtype=F32)
    A[:m, :cols - 1], A[:m, -1] = M[:m, :cols - 1], M[:m, -1]
    acc = np.zeros(A.shape[1], dtype=F32)
    with np.errstate(all="ignore"):
        for r in art_rows:
            acc = (acc + A[r]).astype(F32)
    A[m] = acc
    abasis = basis.copy()
    for i, r in enumerate(reversed(art_rows)):
        A[r, cols - 1 + i] = F32(1)
        abasis[r] = cols - 1 + i
    return M, basis, A, abasis


def lds_bytes(rows, cols):
    """single_lds_bytes (csrc/kernels_single.inc): the stored tableau, the pivot row and the column snapshot."""
    ldl, rp = (cols + 3) // 4 * 4, (rows + 3) // 4 * 4
    return (rows * ldl + ldl + rp) * 4


def fits(rows, cols):
    return lds_bytes(rows, cols) <= LDS_BUDGET


# ------------------------------------------------------------------ generated members
_FLOATS = [F32(k) / F32(8) for k in (-20, -9, -4, -3, 3, 5, 12, 17, 33)]      # never zero: no "float zero" by accident
_INTS = [-3, -2, -1, 1, 2, 3, 5]


def member(seed, ncv, rows, kind="max", zeros=True):
    """rows: [(op, negative right-hand side?)].  Coefficients are exact ints, float32 eighths, integer zeros or not
    mentioned at all (zeros=True); the right-hand side of a negative row is < 0, the others >= 0 (some exactly 0)."""
    rng = np.random.default_rng(seed)
    names = ["x%d" % j for j in range(ncv)]

    def number():
        return _INTS[rng.integers(len(_INTS))] if rng.integers(2) else _FLOATS[rng.integers(len(_FLOATS))]
    cons = []
    for op, negative in rows:
        expr = []
        for v in names:
            k = rng.integers(6) if zeros else 2
            if k == 0:
                continue                                     # not mentioned
            expr.append((v, 0 if k == 1 else number()))      # (an INTEGER zero)
        mag = abs(number()) if rng.integers(4) or negative else 0
        cons.append((op, expr, -mag if negative else mag))
    return dict(type=kind, vars=names, objective_var="w", objective=[(v, number()) for v in names], bounds=[],
                constraints=cons)


def feasible_member(seed, ncv, rows, kind="max"):
    """A member with the point x0 (small integers) feasible, so that phase 1 ends feasible and both phases pivot:
    every product and sum of the right-hand side is exact in float32 (eighths of small integers)."""
    rng = np.random.default_rng(seed)
    names = ["x%d" % j for j in range(ncv)]
    x0 = rng.integers(1, 4, size=ncv)
    cons = []
    for op, negative in rows:
        a = rng.integers(1, 24, size=ncv) * (-1 if negative else 1)          # (eighths; |a . x0| >= 9 > the slack below)
        rhs8 = int(a @ x0) + {"<=": 1, ">=": -1, "=": 0}[op] * int(rng.integers(1, 8))
        assert (rhs8 < 0) == negative
        coef = [int(k) // 8 if k % 8 == 0 else F32(int(k)) / F32(8) for k in a]
        cons.append((op, list(zip(names, coef)), rhs8 // 8 if rhs8 % 8 == 0 else F32(rhs8) / F32(8)))
    # a bounded objective for max: every variable also sits under a `<=` row in the callers' row lists
    return dict(type=kind, vars=names, objective_var="w",
                objective=[(v, int(c) if c % 2 else F32(int(c)) / F32(4)) for v, c in zip(names, rng.integers(1, 9, size=ncv))],
                bounds=[], constraints=cons)


def counts(rows):
    """(`=` rows, artificial rows) of a row list of `member`."""
    flipped = {"<=": ">=", ">=": "<=", "=": "="}
    ops = [flipped[op] if neg else op for op, neg in rows]
    return sum(op == "=" for op in ops), sum(op != "<=" for op in ops)


def sweep_rows(m, ncv):
    """All three senses and both signs over the sweep m 1..7 x ncv 1..5."""
    return [(("<=", ">=", "=")[(i + ncv) % 3], (3 * i + m + ncv) % 4 == 0) for i in range(m)]


@functools.lru_cache(maxsize=None)
def sweep_groups():
    """{(m, ncv): [3 members]} for m 1..7, ncv 1..5."""
    return {(m, ncv): [member(1000 * m + 10 * ncv + k, ncv, sweep_rows(m, ncv)) for k in range(3)]
            for m in range(1, 8) for ncv in range(1, 6)}


#: members of one group whose flips and `=` rows fall on different rows: slack columns and artificial ranks differ per
#: member.  Every list has one `=` row and three artificial rows.  In members 0 and 1 a `<=` row is flipped into an
#: artificial one, in members 1 and 2 a `>=` row is flipped out of one.
MOVING_ROWS = [[("=", False), ("<=", True), (">=", False), ("<=", False)],
               [("<=", True), ("=", True), (">=", True), (">=", False)],
               [(">=", False), (">=", True), (">=", False), ("=", False)],
               [("<=", False), (">=", False), ("=", True), ("<=", True)]]


@functools.lru_cache(maxsize=None)
def moving_group():
    assert len({counts(r) for r in MOVING_ROWS}) == 1 and counts(MOVING_ROWS[0]) == (1, 3)
    return [member(50 + k, 3, rows) for k, rows in enumerate(MOVING_ROWS)]


@functools.lru_cache(maxsize=None)
def zero_rhs_group():
    """Right-hand sides -0.0 and 0: no flip (`<` is false for both); and a negated row of integer zeros and
    coefficients the problem never mentions."""
    def one(a, b):
        return dict(type="min", vars=["x", "y", "z"], objective_var="w", objective=[("x", a), ("y", 1), ("z", F32(0.5))],
                    bounds=[], constraints=[("<=", [("x", 1), ("y", b)], F32(-0.0)),
                                            (">=", [("x", a), ("z", 2)], 0),
                                            ("<=", [("x", 1), ("y", 0)], -3),            # negated: 0 and no z
                                            (">=", [("y", b), ("z", 0)], F32(-1.5)),     # negated out of `>=`
                                            ("=", [("x", 0), ("y", 1), ("z", 1)], -2)])
    return [one(2, F32(1.5)), one(F32(0.25), 3)]


BIG, ULP_HALF, SUB = F32(3e38), F32(2.0 ** -24), F32(1e-40)     # near FLT_MAX, half an ulp of 1, a subnormal


@functools.lru_cache(maxsize=None)
def extreme_rows_group():
    """m = 5, ncv = 4, float32 coefficients; rows 0 .. 2 are the artificial ones.  Per member the three artificial
    rows hold 3e38, 3e38, -3e38 in column x and 1, 2**-24, 2**-24 in column y, each member in another order: the
    artificial objective row is the float sum in increasing row order from +0.0 --
        x   (3e38, 3e38, -3e38) -> inf     (3e38, -3e38, 3e38) -> 3e38      (-3e38, 3e38, 3e38) -> 3e38
        y   (1, h, h) -> 1                 (h, 1, h) -> 1                   (h, h, 1) -> 1 + 2**-23
    and any other order of the same rows gives another value.  Row 3 is a `>=` row with a subnormal negative
    right-hand side and subnormal coefficients: negated exactly, its sense flipped into `<=`.  Row 4 has the
    right-hand side -0.0: not flipped."""
    def one(xs, ys, k):
        return dict(type="max", vars=["x", "y", "z", "u"], objective_var="w",
                    objective=[("x", 1), ("y", F32(0.5)), ("z", 2), ("u", 1)], bounds=[],
                    constraints=[(">=", [("x", xs[0]), ("y", ys[0]), ("z", 1)], 1 + k),
                                 ("=", [("x", xs[1]), ("y", ys[1]), ("u", F32(0.5))], F32(2.5)),
                                 (">=", [("x", xs[2]), ("y", ys[2]), ("z", 2), ("u", 1)], 2),
                                 (">=", [("z", -SUB), ("u", F32(-3e-39)), ("x", -1)], -SUB),
                                 ("<=", [("x", 1), ("y", -1), ("z", F32(1.5))], F32(-0.0))])
    return [one((BIG, BIG, -BIG), (F32(1), ULP_HALF, ULP_HALF), 0),
            one((BIG, -BIG, BIG), (ULP_HALF, F32(1), ULP_HALF), 1),
            one((-BIG, BIG, BIG), (ULP_HALF, ULP_HALF, F32(1)), 2)]


@functools.lru_cache(maxsize=None)
def bounds_group():
    """Offsets (a lower bound, an upper bound alone), a free variable (two columns) and a doubly bounded one (a row
    in front): the lowering's part, the same statements as build_tableau_single's."""
    def one(k):
        return dict(type="max", vars=["x", "y", "z", "u"], objective_var="w",
                    objective=[("x", 1), ("y", F32(0.5)), ("z", -1), ("u", 2)],
                    bounds=[("x", 1, None), ("y", None, 5), ("z", None, None), ("u", F32(0.5), 4)],
                    constraints=[("<=", [("x", 1), ("y", 2), ("z", 1), ("u", 1)], 9 + k),
                                 (">=", [("x", 1), ("z", F32(-0.5))], F32(1.5) + F32(k)),
                                 ("<=", [("y", -1), ("u", 1)], -7),
                                 ("=", [("x", 1), ("y", 1), ("u", F32(1.5))], 6 + k)])
    return [one(0), one(1)]


def ld_step_group(main_cols=None, art_cols=None):
    """Two members whose main (all `<=`, 5 rows) or artificial (all `>=`, 10 rows) tableau has that many columns:
    32 | 33 and 64 | 65 are where the leading dimension steps."""
    if main_cols is not None:
        return [member(main_cols + k, main_cols - 6, [("<=", False)] * 5) for k in range(2)]
    return [member(art_cols + k, art_cols - 21, [(">=", False), ("<=", True)] * 5) for k in range(2)]


def _synthetic_problem(n, m, seed, two_phase):
    """sc.synthetic's numbers (all float32) as a problem; two_phase: every row ends `>=` -- written as such, or as a
    `<=` row with both sides negated (every third row), which the flip turns into one."""
    M0, _ = sc.synthetic(n, m, seed=seed)
    names = ["x%d" % j for j in range(n)]
    cons = []
    for i in range(m):
        if two_phase and i % 3 == 1:
            cons.append(("<=", [(v, F32(-a)) for v, a in zip(names, M0[i, :n])], F32(-M0[i, -1])))
        else:
            cons.append((">=" if two_phase else "<=", [(v, F32(a)) for v, a in zip(names, M0[i, :n])], F32(M0[i, -1])))
    return dict(type="max", vars=names, objective_var="w", objective=[(v, F32(-c)) for v, c in zip(names, M0[m, :n])],
                bounds=[], constraints=cons)


#: the largest m x 300 whose artificial tableau fits the LDS budget when every row is artificial and has a slack
#: column: (m + 1) x (300 + 2 m + 1).  83: 84 x 467, stored 84 x 468 floats + 468 + 84 -> 159 456 bytes <= 159 744;
#: 84: 85 x 469, stored 85 x 472 + 472 + 88 -> 162 720 bytes
BIG_TWO_PHASE_M = 83


@functools.lru_cache(maxsize=None)
def big_group(two_phase):
    m = BIG_TWO_PHASE_M if two_phase else 96
    return [_synthetic_problem(300, m, seed, two_phase) for seed in (3, 4)]


# ------------------------------------------------------------------ groups that are solved
@functools.lru_cache(maxsize=None)
def outcome_group():
    """m = 2, ncv = 2, one artificial row: INFEASIBLE, OPTIMAL, UNBOUNDED, ART_NONZERO (sc.small_pairs' members 1-4)."""
    h = sc.hand_problem
    return [sc.INFEASIBLE_LP,
            h([("<=", [("x", 1), ("y", 1)], F32(3.5)), (">=", [("x", 1)], F32(0.5))], [("x", 1), ("y", F32(0.5))]),
            h([("<=", [("x", 1), ("y", -1)], F32(1.5)), (">=", [("x", 1)], F32(0.5))], [("x", 1), ("y", 1)]),
            h([("<=", [("x", 1), ("y", 1)], F32(1.5)), (">=", [("x", F32(1e-6))], F32(1e-5))], [("x", 1), ("y", 1)])]


OUTCOMES = [sc.INFEASIBLE, sc.OPTIMAL, sc.UNBOUNDED, sc.ART_NONZERO]


@functools.lru_cache(maxsize=None)
def driveout_group():
    """sc.DRIVEOUT_LP and two relatives: phase 1 leaves the artificial of the `=` row basic at zero."""
    def variant(c, rhs):
        return dict(sc.DRIVEOUT_LP, constraints=[("=", [("x", -1), ("y", -1)], 0),
                                                 ("<=", [("x", 1), ("y", 2), ("z", c)], rhs)])
    return [sc.DRIVEOUT_LP, variant(F32(1.25), 5), variant(2, F32(4.5))]


@functools.lru_cache(maxsize=None)
def single_phase_group():
    """m = 3, ncv = 3, no artificial row (one `>=` row flipped out of it): optimal members and an unbounded one."""
    def one(c, unbounded):
        return dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", c), ("y", 2), ("z", 1)],
                    bounds=[], constraints=[("<=", [("x", 1), ("y", 1)] + ([] if unbounded else [("z", 1)]), 10),
                                            (">=", [("x", -1), ("y", F32(0.5))], F32(-6.5)),
                                            ("<=", [("y", 3), ("x", 0)], 12)])
    return [one(3, False), one(F32(0.5), False), one(1, True)]


MEDIUM_ROWS = [("<=", False)] * 6 + [(">=", False), ("<=", True), ("=", False), (">=", False), (">=", True), ("=", True)]


@functools.lru_cache(maxsize=None)
def medium_group(kind="max"):
    """m = 12, ncv = 9, two `=` rows, five artificial rows, flips both ways: members that pivot in both phases."""
    return [feasible_member(700 + k, 9, MEDIUM_ROWS, kind) for k in range(4)]


@functools.lru_cache(maxsize=None)
def model_solution(group_fn, *args):
    """The model's build and solve of every member of a group (computed once, shared)."""
    out = []
    for d in group_fn(*args):
        b = sc.build(d)
        is_max = d["type"] == "max"
        if b["art"] is None:
            st, tr, M, basis = sc.solve(b["main"][0], b["main"][1], is_max)
            out.append(dict(build=b, status=st, n=(len(tr),), main_trace=tr, M=M, mbasis=basis))
        else:
            r = sc.two_phase(b["art"][0], b["art"][1], b["main"][0], b["main"][1], is_max)
            out.append(dict(build=b, status=r["status"], n=(len(r["art_trace"]), r["n2"]), art_trace=r["art_trace"],
                            main_trace=r["main_trace"], M=r["M"], mbasis=r["mbasis"], A=r["A"], abasis=r["abasis"]))
    return out


# ------------------------------------------------------------------ members for the host route
def float_zero_member():
    """x + 0.0 y + 0 z <= -3: Lisp negates the single-float zero into -0.0, the integer one stays 0."""
    return dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", -1), ("y", -1), ("z", -1)], bounds=[],
                constraints=[("<=", [("x", 1), ("y", F32(0.0)), ("z", 0)], -3), ("<=", [("x", 1), ("y", 1), ("z", 1)], 10)])


def integer_sum_member():
    """`=` rows with 2**24, 1, 1 in x's column: Lisp's artificial objective row holds 16777218 there, a float32
    running sum 16777216.  (Three equations in two unknowns, satisfied by x = 1, y = 0: the reference ends with an
    artificial variable stuck in the basis, on every route.)"""
    return dict(type="max", vars=["x", "y"], objective_var="w", objective=[("x", 1), ("y", 1)], bounds=[],
                constraints=[("=", [("x", 2 ** 24), ("y", 1)], 2 ** 24), ("=", [("x", 1), ("y", 1)], 1),
                             ("=", [("x", 1), ("y", 2)], 1)])


def declined_member():
    return sc.hand_problem([("<=", [("x", 1), ("y", 0.1)], 4)], [("x", 1), ("y", 1)])      # 0.1: no binary32 holds it


def lone_member():
    return member(9, 4, [("<=", False), ("<=", False)], zeros=False)


def no_constraints_member():
    return dict(type="max", vars=["x"], objective_var="w", objective=[("x", 1)], bounds=[("x", 0, 4)], constraints=[])
