"""The MODEL of the single-float path: SURVEY section 8 a3-a9 and Appendix A restated in NumPy float32, with
`float` in place of `double` -- the yardstick of tests/test_single_host.py and tests/test_gpu_single.py.

Every number is an np.float32 and every operation an np.float32 operation: a product is rounded, then the
difference is rounded (NumPy's multiply and subtract are separate ufuncs: no FMA), division is true division.
The scans are written in the reference's order (`finding i minimizing`: start at the first candidate, replace
only by a strictly smaller one), so the NaN rules fall out by themselves: a NaN never replaces anything and
is never replaced where it is the first candidate.

    thresholds           (f/8) eps_s, 0 + (f/2) eps_s, f eps_s in float32 (src/utils.lisp:84-124)
    price / ratio / pivot   find-entering-column, find-pivoting-row, n-pivot-row (src/simplex.lisp:337-389)
    solve                n-solve-tableau, single tableau (:453-461), with the backend's pivot cap
    two_phase            n-solve-tableau, two-phase branch (:402-452)
    build                build-tableau (:142-328) with Lisp's contagion on exact ints and single-floats
    variable / objective / reduced_cost    the read-back (:74-120) in float32
and the shapes and special tableaux the tests share.  Nothing here touches the library.
"""
import functools

import numpy as np

F32 = np.float32
EPS_S = F32(2.0 ** -24 * (1 + 2.0 ** -23))                 # SBCL's single-float-epsilon
OPTIMAL, UNBOUNDED, INFEASIBLE, MAX_PIVOTS, ART_NONZERO, ART_STUCK = 0, 1, 2, 3, 4, 5


def thresholds(factor=1024):
    f = F32(factor)
    return (F32(F32(f / F32(8)) * EPS_S), F32(F32(0) + F32(F32(f / F32(2)) * EPS_S)), F32(f * EPS_S))


# ------------------------------------------------------------------ the step-wise pieces
def price(M, is_max, factor=1024):
    """find-entering-column: column or None."""
    ptol = thresholds(factor)[0]
    obj = M[-1]
    vc = M.shape[1] - 1
    if vc < 1:
        return None
    col = 0
    for i in range(1, vc):
        if (obj[i] < obj[col]) if is_max else (obj[i] > obj[col]):
            col = i
    if is_max:
        return col if obj[col] < F32(F32(0) - ptol) else None
    return col if obj[col] > F32(F32(0) + ptol) else None


def ratio(M, ec, factor=1024):
    """find-pivoting-row: row or None."""
    thr = thresholds(factor)[1]
    vc = M.shape[1] - 1
    best, bq = None, None
    with np.errstate(all="ignore"):
        for i in range(M.shape[0] - 1):
            a = M[i, ec]
            if thr < a:
                q = F32(M[i, vc] / a)
                if best is None or q < bq:
                    best, bq = i, q
    return best


def pivot(M, basis, ec, cr):
    """n-pivot-row, in place."""
    with np.errstate(all="ignore"):
        col = M[:, ec].copy()
        prow = (M[cr] / M[cr, ec]).astype(F32)
        prod = np.multiply.outer(col, prow).astype(F32)     # rounded products ...
        new = (M - prod).astype(F32)                        # ... then rounded differences
        new[cr] = prow
    M[...] = new
    if len(basis):
        basis[cr] = ec


def solve(M0, basis0, is_max, factor=1024, cap=0):
    """-> (status, trace [(ec, cr) ...], M, basis); cap > 0: MAX_PIVOTS once `cap` pivots are made and the
    tableau is not optimal (the backend's order of tests: optimal, cap, unbounded)."""
    M, basis = np.array(M0, dtype=F32, copy=True), np.array(basis0, dtype=np.int64, copy=True)
    trace = []
    while True:
        ec = price(M, is_max, factor)
        if ec is None:
            return OPTIMAL, trace, M, basis
        if cap > 0 and len(trace) >= cap:
            return MAX_PIVOTS, trace, M, basis
        cr = ratio(M, ec, factor)
        if cr is None:
            return UNBOUNDED, trace, M, basis
        pivot(M, basis, ec, cr)
        trace.append((ec, cr))


def two_phase(A0, abasis0, M0, mbasis0, main_is_max, factor=1024):
    """n-solve-tableau on (art main) -> dict(status, n1 (phase 1 + drive-outs), n2, art_trace, main_trace, A, abasis,
    M, mbasis); M / mbasis are the main tableau as the call leaves it (untouched unless the hand-over was made)."""
    st, t1, A, ab = solve(A0, abasis0, False, factor)
    M, mb = np.array(M0, dtype=F32, copy=True), np.array(mbasis0, dtype=np.int64, copy=True)
    out = dict(status=st, n1=len(t1), n2=0, art_trace=t1, main_trace=[], A=A, abasis=ab, M=M, mbasis=mb)
    if st != OPTIMAL:
        return out
    m, nv, nav = M.shape[0] - 1, M.shape[1] - 1, A.shape[1] - 1
    if not (abs(F32(F32(0) - A[m, nav])) <= thresholds(factor)[2]):         # (fp= 0 objective factor)
        out["status"] = INFEASIBLE
        return out
    for i in range(m):                                                      # :419-434
        if ab[i] >= nv:
            if A[i, nav] != 0:
                out["status"] = ART_NONZERO
                return out
            new_col = -1
            for j in range(nv):
                if A[i, j] != 0 and all(int(b) != j for b in ab):
                    new_col = j
                    break
            if new_col == -1:
                out["status"] = ART_STUCK
                return out
            pivot(A, ab, new_col, i)
            t1.append((new_col, i))
    out["n1"] = len(t1)
    M[:m, :nv] = A[:m, :nv]                                                 # :437-441
    M[:m, nv] = A[:m, nav]
    with np.errstate(all="ignore"):
        for i in range(m):                                                  # :444-451, sequential in i
            mb[i] = ab[i]
            scale = M[m, ab[i]]
            if scale != 0:
                M[m] = (M[m] - (scale * M[i]).astype(F32)).astype(F32)
    st2, t2, M2, mb2 = solve(M, mb, main_is_max, factor)
    out.update(status=st2, n2=len(t2), main_trace=t2, M=M2, mbasis=mb2)
    return out


# ------------------------------------------------------------------ build-tableau and read-back
def _n(x):
    return int(x) if isinstance(x, (int, np.integer)) and not isinstance(x, bool) else F32(x)


def _op(fn, *xs):
    """One Lisp arithmetic operation: exact on ints, a single-float operation once a float takes part."""
    if all(isinstance(x, int) for x in xs):
        return fn(*xs)
    with np.errstate(all="ignore"):                          # (an overflow is an infinity, as on the device)
        return F32(fn(*[F32(x) for x in xs]))


def build(problem):
    """problem: dict(type, vars, objective [(var, c)], bounds [(var, lb, ub)], constraints [(op, [(var, c)], rhs)]).
    -> dict(main=(M, basis), art=(A, abasis) or None, mapping, type)."""
    add, sub, mul, neg = (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda a: -a)
    cons = [(op, [(v, _n(c)) for v, c in e], _n(r)) for op, e, r in problem["constraints"]]
    bounds = {b[0]: (b[1], b[2]) for b in problem.get("bounds", [])}
    mapping, column = {}, 0
    assert cons, "the model covers problems with constraints"
    for var in problem["vars"]:
        lb, ub = bounds.get(var, (None, None))
        if var not in bounds:
            mapping[var] = ("positive", column, 0)
        elif lb is not None and ub is not None:
            cons.insert(0, ("<=", [(var, 1)], _n(ub)) if 0 <= ub else (">=", [(var, 1)], _op(neg, _n(ub))))
            mapping[var] = ("positive", column, _n(lb))
        elif lb is not None:
            mapping[var] = ("positive", column, _n(lb))
        elif ub is not None:
            mapping[var] = ("negative", column, _n(ub))
        else:
            mapping[var] = ("signed", column)
            column += 1
        column += 1
    ncv, m = column, len(cons)
    ncols = ncv + sum(1 for c in cons if c[0] != "=") + 1
    M = [[0] * ncols for _ in range(m + 1)]
    basis, art_rows, off = [0] * m, [], 0
    for r, (op, expr, rhs) in enumerate(cons):
        M[r][-1] = rhs
        for var, coef in expr:
            mp = mapping[var]
            if mp[0] == "signed":
                M[r][mp[1]], M[r][mp[1] + 1] = coef, _op(neg, coef)
            else:
                M[r][mp[1]] = coef if mp[0] == "positive" else _op(neg, coef)
                M[r][-1] = _op(sub, M[r][-1], _op(mul, coef, mp[2]))
        if M[r][-1] < 0:
            M[r] = [_op(neg, x) for x in M[r]]
            op = {"<=": ">=", ">=": "<=", "=": "="}[op]
        if op == "<=":
            M[r][ncv + off], basis[r] = 1, ncv + off
            off += 1
        elif op == ">=":
            art_rows.insert(0, r)
            M[r][ncv + off], basis[r] = -1, ncols
            off += 1
        else:
            art_rows.insert(0, r)
            basis[r] = ncols
    for var, coef in problem["objective"]:
        mp, coef = mapping[var], _n(coef)
        if mp[0] == "signed":
            M[m][mp[1]], M[m][mp[1] + 1] = _op(neg, coef), coef
        else:
            M[m][mp[1]] = _op(neg, coef) if mp[0] == "positive" else coef
            M[m][-1] = _op(add, M[m][-1], _op(mul, coef, mp[2]))

    def f32(rows):
        return np.array([[F32(x) for x in row] for row in rows], dtype=F32)
    out = dict(main=(f32(M), np.array(basis, dtype=np.int64)), art=None, mapping=mapping, type=problem["type"])
    if art_rows:
        na = len(art_rows)
        A = [[0] * (ncols + na) for _ in range(m + 1)]
        ab = list(basis)
        for i, r in enumerate(art_rows):
            ab[r] = ncols - 1 + i
            A[r][ncols - 1 + i] = 1
        for src, dst in [(c, c) for c in range(ncols - 1)] + [(ncols - 1, ncols + na - 1)]:
            s = 0
            for r in range(m):
                A[r][dst] = M[r][src]
                if r in art_rows:
                    s = _op(add, s, A[r][dst])
            A[m][dst] = s
        out["art"] = (f32(A), np.array(ab, dtype=np.int64))
    return out


def objective(M):
    return F32(M[-1, -1])


def variable(M, basis, mapping, var):
    def basic(col):
        pos = [i for i, b in enumerate(basis) if int(b) == col]
        return F32(M[pos[0], -1]) if pos else F32(0)
    mp = mapping[var]
    if mp[0] == "positive":
        return F32(F32(mp[2]) + basic(mp[1]))
    if mp[0] == "negative":
        return F32(F32(mp[2]) + F32(-basic(mp[1])))
    return F32(basic(mp[1]) - basic(mp[1] + 1))


def reduced_cost(M, mapping, var):
    assert mapping[var][0] == "positive"
    return F32(M[-1, mapping[var][1]])


def solve_problem(problem, factor=1024):
    """-> dict(status, pivots, M, basis, mapping): the model's answer to the public function."""
    b = build(problem)
    if b["art"] is None:
        st, tr, M, basis = solve(b["main"][0], b["main"][1], b["type"] == "max", factor)
        return dict(status=st, pivots=len(tr), trace=tr, M=M, basis=basis, mapping=b["mapping"])
    r = two_phase(b["art"][0], b["art"][1], b["main"][0], b["main"][1], b["type"] == "max", factor)
    return dict(status=r["status"], pivots=(r["n1"], r["n2"]), trace=(r["art_trace"], r["main_trace"]), M=r["M"],
                basis=r["mbasis"], mapping=b["mapping"], two_phase=r)


# ------------------------------------------------------------------ shared tableaux
def synthetic(n, m, seed=None):
    """SURVEY 8(d)'s generator (splitmix64 stream: A = 0.05 + u, b = n (0.25 + 0.5 u), c = 0.5 + u) with the inputs
    rounded to float32: [A | I | b ; -c | 0 | 0], basis n .. n+m-1, a max problem."""
    gamma = np.uint64(0x9E3779B97F4A7C15)
    seed = np.uint64((0x9E3779B97F4A7C15 ^ (20260928 + 1000 * n + m)) if seed is None else seed)

    def u01(start, count):
        with np.errstate(over="ignore"):
            k = np.arange(start + 1, start + count + 1, dtype=np.uint64)
            z = seed + k * gamma
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    M = np.zeros((m + 1, n + m + 1), dtype=F32)
    M[:m, :n] = (0.05 + u01(0, n * m).reshape(m, n)).astype(F32)
    M[np.arange(m), n + np.arange(m)] = 1
    M[:m, n + m] = (float(n) * (0.25 + 0.5 * u01(n * m, m))).astype(F32)
    M[m, :n] = -(0.5 + u01(n * m + m, n)).astype(F32)
    return M, np.arange(n, n + m, dtype=np.int64)


_CACHE = {}


def solved_synthetic(n, m, is_max=True, cap=0):
    """The model's solve of synthetic(n, m) (computed once per process, read-only)."""
    key = (n, m, is_max, cap)
    if key not in _CACHE:
        M0, b0 = synthetic(n, m)
        if not is_max:
            M0 = M0.copy()
            M0[-1] = -M0[-1]                                # min -c'x: the mirrored problem, same pivots
        st, tr, M, b = solve(M0, b0, is_max, 1024, cap)
        for a in (M0, b0, M, b):
            a.setflags(write=False)
        _CACHE[key] = (M0, b0, st, tr, M, b)
    return _CACHE[key]


def overflow_tableau():
    """4 x 7, a max problem [A | I | b ; -c | 0 | 0]: the first pivot (0, 0) divides 3e38 by 0.5 -- inf in the pivot
    row, -inf in row 1, NaN (0 * inf) in row 2, +inf in the objective row; the second pivot (2, 1) then leaves
    inf - inf = NaN in the objective row's column 1, which never enters (a NaN is no candidate outside column 0)."""
    M = np.zeros((4, 7), dtype=F32)
    M[:3, :3] = [[0.5, 3e38, 0.1], [1, 1, 2], [0, 1, 1]]
    M[np.arange(3), 3 + np.arange(3)] = 1
    M[:3, 6] = [1, 4, 3]
    M[3, :3] = [-4, -1, -2]
    return M, np.array([3, 4, 5], dtype=np.int64)


def same_bits(G, M):
    """Bit for bit, except that any NaN equals any NaN (its payload and sign are the hardware's choice)."""
    G, M = np.asarray(G), np.asarray(M)
    if G.shape != M.shape or G.dtype != np.float32 or M.dtype != np.float32:
        return False
    nan = np.isnan(M)
    return bool(np.array_equal(np.isnan(G), nan) and np.array_equal(G.view(np.uint32)[~nan], M.view(np.uint32)[~nan]))


#: phase 1 has nothing to do (the artificial objective row is <= 0 from the start) and leaves the artificial of the
#: `=` row basic at zero: the hand-over drives it out with a forced pivot on -1
DRIVEOUT_LP = dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", 1), ("y", F32(0.5)), ("z", 1)],
                bounds=[], constraints=[("=", [("x", -1), ("y", -1)], 0),
                                        ("<=", [("x", 1), ("y", 2), ("z", F32(0.7))], F32(3.5))])
INFEASIBLE_LP = dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", 1)], bounds=[],
                  constraints=[("<=", [("x", 1), ("y", 1)], F32(1.5)), (">=", [("x", 1)], F32(2.5))])


def hand_problem(constraints, objective):
    return dict(type="max", vars=["x", "y"], objective_var="z", objective=objective, bounds=[], constraints=constraints)


@functools.lru_cache(maxsize=None)
def small_pairs():
    """Five 2 x 2 two-phase pairs (art, art basis, main, main basis), one of every outcome: OPTIMAL after one drive-out,
    INFEASIBLE, OPTIMAL, UNBOUNDED, and ART_NONZERO (1e-6 x >= 1e-5: phase 1 ends inside f eps with the artificial
    still basic at a level that is no exact zero)."""
    ds = [DRIVEOUT_LP, INFEASIBLE_LP,
          hand_problem([("<=", [("x", 1), ("y", 1)], F32(3.5)), (">=", [("x", 1)], F32(0.5))], [("x", 1), ("y", F32(0.5))]),
          hand_problem([("<=", [("x", 1), ("y", -1)], F32(1.5)), (">=", [("x", 1)], F32(0.5))], [("x", 1), ("y", 1)]),
          hand_problem([("<=", [("x", 1), ("y", 1)], F32(1.5)), (">=", [("x", F32(1e-6))], F32(1e-5))], [("x", 1), ("y", 1)])]
    built = [build(d) for d in ds]
    return tuple((b["art"][0], b["art"][1], b["main"][0], b["main"][1]) for b in built)


def tiny_coefficient_problem():
    """max 1e-6 x  s.t. x <= 1, the coefficient a float32: below the single-float pricing threshold (7.6e-6), far
    above the double one (1.4e-14) -- the input that tells the two precisions apart."""
    return dict(type="max", vars=["x"], objective_var="z", objective=[("x", F32(1e-6))], bounds=[],
                constraints=[("<=", [("x", 1)], 1)])


def tie_tableau(n, m, tied_cols, tied_rows, is_max=True, slack=True):
    """Integer-valued float32 LP with exact ties: the objective entries of `tied_cols` are equal and the most
    negative (max) / positive (min); in the first of them the rows `tied_rows` have equal ratios, the smallest.
    slack=False leaves the slack columns out ([A | b ; -c | 0], basis entries all 0): not a basis a solver would
    start from, but the same arithmetic and the same scans, and the only way to more than 1024 rows inside the LDS
    budget."""
    ns = m if slack else 0
    M = np.zeros((m + 1, n + ns + 1), dtype=F32)
    rng = np.random.default_rng(n * 1000 + m)
    M[:m, :n] = rng.integers(1, 5, size=(m, n)).astype(F32)
    if slack:
        M[np.arange(m), n + np.arange(m)] = 1
    M[:m, n + ns] = 64
    M[m, :n] = -rng.integers(1, 8, size=n).astype(F32)
    for c in tied_cols:
        M[m, c] = -16
        M[:m, c] = 1
        for r in tied_rows:
            M[r, c] = 8                                      # ratio 64 / 8 = 8 against 64 / 1 elsewhere
    if not is_max:
        M[m] = -M[m]
    return M, (np.arange(n, n + m, dtype=np.int64) if slack else np.zeros(m, dtype=np.int64))
