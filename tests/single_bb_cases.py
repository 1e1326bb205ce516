"""The MODEL of the single-float branch-and-bound: the reference's loop (simplex-solver, src/simplex.lisp:462-542)
written directly over tests/single_cases.py -- the yardstick of tests/test_single_bb_host.py and
tests/test_gpu_single_bb.py.  Nothing here touches the library.

    integral      v == floor(v) on the np.float32 that `variable` returns; int_tolerance > 0: |v - round(v)| <=
                  int_tolerance * eps_s, computed in float32
    bounds        floor(v) / ceil(v) as exact Python integers; a node's constraints are entry ++ problem constraints,
                  the entry's rows `var <= / >= bound` with integer coefficient 1, newest first
    node LP       single_cases.build of the node problem, then single_cases.solve / the two-phase branch, with a
                  pivot cap (both phases together): the reference has no anti-cycling rule
    comparator    `<` (max) / `>` (min) on np.float32 objective values

Problems are single_cases' dicts with an "integer_vars" list.  A trace row is exact_bb.search's: (parent trace
index, var or None, sense, float(bound), outcome, float(objective) or NaN).
"""
import functools
import math

import numpy as np

from tests import single_cases as sc

F32 = np.float32
PIVOT_CAP = 200                                     # per node LP, both phases together; the library gets the same
INFEASIBLE, PRUNED, BRANCHED, INCUMBENT, NOT_BETTER, FAILED = range(6)      # MI_BB_*
NODE_CAP = "node-cap"


# ------------------------------------------------------------------ one node LP
def two_phase(A0, abasis0, M0, mbasis0, main_is_max, cap):
    """single_cases.two_phase with the backend's cap: `cap` pivots for phase 1, the drive-outs and phase 2 together."""
    st, t1, A, ab = sc.solve(A0, abasis0, False, 1024, cap)
    if st != sc.OPTIMAL:
        return st, None, None
    M, mb = np.array(M0, dtype=F32, copy=True), np.array(mbasis0, dtype=np.int64, copy=True)
    m, nv, nav = M.shape[0] - 1, M.shape[1] - 1, A.shape[1] - 1
    if not (abs(F32(F32(0) - A[m, nav])) <= sc.thresholds()[2]):
        return sc.INFEASIBLE, None, None
    n1 = len(t1)
    for i in range(m):
        if ab[i] >= nv:
            if A[i, nav] != 0:
                return sc.ART_NONZERO, None, None
            new_col = next((j for j in range(nv) if A[i, j] != 0 and all(int(b) != j for b in ab)), -1)
            if new_col == -1:
                return sc.ART_STUCK, None, None
            sc.pivot(A, ab, new_col, i)
            n1 += 1
    M[:m, :nv] = A[:m, :nv]
    M[:m, nv] = A[:m, nav]
    with np.errstate(all="ignore"):
        for i in range(m):
            mb[i] = ab[i]
            scale = M[m, ab[i]]
            if scale != 0:
                M[m] = (M[m] - (scale * M[i]).astype(F32)).astype(F32)
    if cap > 0 and n1 >= cap:
        return sc.MAX_PIVOTS, None, None
    st2, _, M2, mb2 = sc.solve(M, mb, main_is_max, 1024, cap - n1 if cap > 0 else 0)
    return st2, M2, mb2


def node_problem(problem, entry):
    rows = [("<=" if sense == 0 else ">=", [(var, 1)], int(bound)) for var, sense, bound in entry]
    return dict(problem, constraints=rows + list(problem["constraints"]))


def build_node(problem, entry):
    """single_cases.build of the node problem: (main, main basis, art or None, art basis or None)."""
    b = sc.build(node_problem(problem, entry))
    return b["main"][0], b["main"][1], (b["art"][0] if b["art"] else None), (b["art"][1] if b["art"] else None)


def solve_node(problem, entry, cap=PIVOT_CAP):
    """-> (status, M, basis, mapping)."""
    b = sc.build(node_problem(problem, entry))
    is_max = problem["type"] == "max"
    if b["art"] is None:
        st, _, M, basis = sc.solve(b["main"][0], b["main"][1], is_max, 1024, cap)
    else:
        st, M, basis = two_phase(b["art"][0], b["art"][1], b["main"][0], b["main"][1], is_max, cap)
    return st, M, basis, b["mapping"]


# ------------------------------------------------------------------ the search
def fractional(v, int_tolerance=0):
    v = F32(v)
    if int_tolerance > 0:
        return not (abs(F32(v - np.round(v))) <= F32(F32(int_tolerance) * sc.EPS_S))
    return not (v == np.floor(v))


class Result:
    """status: sc.OPTIMAL (an incumbent), sc.INFEASIBLE (none), NODE_CAP, or the status of the node LP that ended
    the search; trace; depth: the deepest node processed; M / basis / mapping / values / objective: the incumbent's."""

    def __init__(self):
        self.status, self.trace, self.depth = None, [], 0
        self.M = self.basis = self.mapping = self.values = self.objective = None


def search(problem, max_nodes=0, cap=PIVOT_CAP, int_tolerance=0):
    is_max = problem["type"] == "max"

    def better(inc, v):
        return inc < v if is_max else inc > v
    res = Result()
    stack = [((), -1)]                                                    # (entry, parent trace index)
    while stack:
        if max_nodes and len(res.trace) >= max_nodes:
            res.status = NODE_CAP
            return res
        entry, parent = stack.pop()
        res.depth = max(res.depth, len(entry))
        var, sense, bound = entry[0] if entry else (None, 0, 0)
        st, M, basis, mapping = solve_node(problem, entry, cap)

        def row(outcome, obj=float("nan")):
            res.trace.append((parent, var, sense, float(bound), outcome, float(obj)))
        if st == sc.INFEASIBLE:
            row(INFEASIBLE)
            continue
        if st != sc.OPTIMAL:
            row(FAILED)
            res.status = st
            return res
        obj = sc.objective(M)
        values = {v: sc.variable(M, basis, mapping, v) for v in problem["vars"]}
        viol = next((v for v in problem["integer_vars"] if fractional(values[v], int_tolerance)), None)
        if viol is not None and res.objective is not None and not better(res.objective, obj):
            row(PRUNED, obj)
        elif viol is not None:
            me = len(res.trace)
            v = float(values[viol])
            stack.append((((viol, 1, math.ceil(v)),) + entry, me))
            stack.append((((viol, 0, math.floor(v)),) + entry, me))       # the `<=` child on top
            row(BRANCHED, obj)
        elif res.objective is None or better(res.objective, obj):
            res.M, res.basis, res.mapping, res.values, res.objective = M, basis, mapping, values, obj
            row(INCUMBENT, obj)
        else:
            row(NOT_BETTER, obj)
    res.status = sc.OPTIMAL if res.objective is not None else sc.INFEASIBLE
    return res


def same_trace(got, want):
    """Outcomes, variables, senses, bounds, parents, and objectives as float32 bits (any NaN equal to any NaN)."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if tuple(g[:5]) != tuple(w[:5]):
            return False
        if not sc.same_bits(np.array([g[5]], dtype=F32), np.array([w[5]], dtype=F32)):
            return False
    return True


# ------------------------------------------------------------------ cases
def quarters(rng, lo, hi):
    """k / 4 as float32, k in [4 lo, 4 hi); an integer value stays a Python int (Lisp reads `2`, not `2.0`)."""
    k = int(rng.integers(4 * lo, 4 * hi))
    return k // 4 if k % 4 == 0 else F32(k / 4)


def halves(rng, lo, hi):
    k = int(rng.integers(2 * lo, 2 * hi))
    return k // 2 if k % 2 == 0 else F32(k / 2)


def random_ilp(seed, shape):
    """shape 0: `<=` rows only; 1: one `>=` row as well; 2: a `>=` and an `=` row (two-phase nodes with 1-3
    artificial rows).  3-5 variables, 2-4 `<=` rows, max and min."""
    rng = np.random.default_rng(1000 * shape + seed)
    n, m = int(rng.integers(3, 6)), int(rng.integers(2, 5))
    names = ["x%d" % i for i in range(n)]
    is_max = bool(rng.integers(0, 2))
    cons = [("<=", [(v, quarters(rng, 1, 5)) for v in names], halves(rng, 8, 20)) for _ in range(m)]
    if shape >= 1:
        cons.append((">=", [(v, quarters(rng, 1, 3)) for v in names[:2]], halves(rng, 1, 4)))
    if shape >= 2:
        cons.append(("=", [(names[0], 1), (names[-1], F32(0.5))], halves(rng, 2, 5)))
    if is_max:
        objective = [(v, quarters(rng, 1, 6)) for v in names]
    else:                                           # min: costs below zero pull against the `<=` rows
        objective = [(v, quarters(rng, -5, 0)) for v in names]
    return dict(type="max" if is_max else "min", vars=names, objective_var="z", objective=objective, bounds=[],
                constraints=cons, integer_vars=names[: int(rng.integers(1, n + 1))])


def kind_case(kind):
    """One problem per mapping kind of the integer variable x: "lower" (lb 0.5: a float32 offset), "upper" (upper
    bound only: `negative`, its node rows flip), "free" (`signed`: a negative branching bound, its node row flips),
    "both" (doubly bounded: a bound row in front)."""
    bounds = {"lower": [("x", F32(0.5), None)], "upper": [("x", None, F32(4.5))], "free": [("x", None, None)],
              "both": [("x", F32(-1.5), F32(3.5))]}[kind]
    cons = [("<=", [("x", 2), ("y", F32(1.5))], F32(7.5)), ("<=", [("x", F32(0.75)), ("y", 2)], F32(8.5))]
    objective = [("x", 3), ("y", F32(2.5))]
    kind_type = "max"
    if kind == "free":                              # x is pushed below zero: min x + y with x >= -2.5 - y / 2
        cons = [(">=", [("x", 2), ("y", 1)], F32(-5.5)), ("<=", [("y", 1)], F32(2.5)), ("<=", [("x", 1)], 4)]
        objective, kind_type = [("x", 1), ("y", F32(0.25))], "min"
    return dict(type=kind_type, vars=["x", "y"], objective_var="z", objective=objective, bounds=bounds, constraints=cons,
                integer_vars=["x", "y"])


#: (name, seed, shape) of the random cases: chosen so that the model alone ends within 64 nodes at depth 8 or less
RANDOM_CASES = (("le_1", 1, 0), ("le_2_min", 2, 0), ("le_6", 6, 0), ("le_7", 7, 0),
                ("ge_0", 0, 1), ("ge_1", 1, 1), ("ge_2", 2, 1), ("ge_4_min", 4, 1),
                ("eq_22", 22, 2), ("eq_54_min", 54, 2), ("eq_62", 62, 2), ("eq_69", 69, 2))
#: the one that does not settle (depth 139 at a cap of 300 nodes): float `integerp` never holds along its spine --
#: the max_nodes case, nothing else
DEEP_CASE = (4, 0)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (problem dict, the model's Result), computed once per process."""
    if name.startswith("kind_"):
        p = kind_case(name[5:])
    else:
        _, seed, shape = next(c for c in RANDOM_CASES if c[0] == name)
        p = random_ilp(seed, shape)
    r = search(p)
    assert r.status in (sc.OPTIMAL, sc.INFEASIBLE) and len(r.trace) <= 64 and r.depth <= 8, (name, r.status, len(r.trace), r.depth)
    return p, r


def search_cases():
    return ["kind_lower", "kind_upper", "kind_free", "kind_both"] + [c[0] for c in RANDOM_CASES]


def to_problem(lp, d):
    """The library's Problem of a model dict."""
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), integer_vars=list(d.get("integer_vars", [])),
                      var_bounds=[(b[0], (b[1], b[2])) for b in d.get("bounds", [])],
                      constraints=[(op, list(e), rhs) for op, e, rhs in d["constraints"]])


# ------------------------------------------------------------------ device assembly: bases and node lists
_KIND_BOUNDS = [("v1", F32(2.5), None), ("v2", F32(-1.5), F32(3.25)), ("v3", None, F32(4.5)), ("v4", None, None), ("v5", 2, None)]
_OFFSET = {"v0": 0, "v1": 2.5, "v2": -1.5, "v3": 4.5, "v4": 0, "v5": 2}
_NAMES = ["v%d" % i for i in range(6)]


def assembly_base(node_cols, d, art_bound=False, n_ge=0, n_eq=0, seed=0):
    """A base whose nodes of depth d have `node_cols` main columns, on variables of every mapping kind -- no bounds,
    a float32 lower bound, both bounds, an upper bound only, free, an integer lower bound -- with one base row that
    build-tableau negates (2 v1 + v0 >= 3 with v1 >= 2.5: right-hand side -2; it stays non-artificial), n_ge `>=` and
    n_eq `=` rows (artificial rows behind the node rows) and, with art_bound, a doubly-bounded variable below zero
    whose bound row is artificial and stands in front of the node rows."""
    rng = np.random.default_rng(seed)
    names = _NAMES + (["v6"] if art_bound else [])
    bounds = _KIND_BOUNDS + ([("v6", F32(-5.5), F32(-1.5))] if art_bound else [])
    nb = 2 if art_bound else 1
    extra = node_cols - d - (len(names) + 1 + nb + 2 + n_ge + 1)
    assert extra >= 0, "node_cols too small for this base"
    names = names + ["w%d" % i for i in range(extra)]
    cons = [("<=", [(v, quarters(rng, 1, 4)) for v in names], halves(rng, 30, 40)), (">=", [("v1", 2), ("v0", 1)], 3)]
    for _ in range(n_ge):
        cons.append((">=", [("v0", quarters(rng, 1, 3)), ("v4", quarters(rng, 1, 3))], halves(rng, 1, 6)))
    for _ in range(n_eq):
        cons.append(("=", [("v0", 1), ("v4", F32(0.5))], halves(rng, 1, 5)))
    return dict(type="max" if seed % 2 else "min", vars=names, objective_var="z",
                objective=[(v, quarters(rng, -3, 5)) for v in names], bounds=bounds, constraints=cons,
                integer_vars=list(_NAMES))


def row_artificial(row):
    var, sense, bound = row
    return (1 - sense if bound - _OFFSET[var] < 0 else sense) == 1


def assembly_nodes(seed, depth, count, want_art=None):
    """`count` entries of `depth` rows whose shifted right-hand sides are negative, zero and positive in both senses;
    want_art: exactly that many artificial node rows per entry (None: whatever comes, but the same in every entry)."""
    rng = np.random.default_rng(seed)

    def row():
        v = _NAMES[int(rng.integers(0, 6))]
        b = int(rng.integers(-4, 7))
        if rng.random() < 0.25 and float(_OFFSET[v]).is_integer():
            b = int(_OFFSET[v])                                           # bound = offset: rhs 0, not negated
        return v, int(rng.integers(0, 2)), b
    out = []
    while len(out) < count:
        e = tuple(row() for _ in range(depth))
        n = sum(row_artificial(r) for r in e)
        if want_art is None:
            want_art = n
        if n == want_art:
            out.append(e)
    return out


def big_sum_base():
    """An artificial column holding 2**24, 1, 1: Lisp's sum is 2**24 + 2, a float32 running sum stays at 2**24."""
    return dict(type="min", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", F32(0.5))], bounds=[],
                constraints=[(">=", [("x", 2 ** 24), ("y", 1)], 2), (">=", [("x", 1), ("y", F32(0.5))], 1),
                             (">=", [("x", 1)], 1), ("<=", [("x", 1), ("y", 1)], F32(7.5))],
                integer_vars=["x", "y"])


def guard_case():
    """kind_case("both") with two redundant rows on y alone (no offset: their right-hand sides stay integers) that sum
    past 2**24: every group of its search fails the guard and is built on the host."""
    d = kind_case("both")
    return dict(d, constraints=list(d["constraints"]) + [("<=", [("y", 1)], 2 ** 24), ("<=", [("y", 2)], 100)])


def tall_case():
    """kind_case("both") with 198 redundant rows: a node is 203 x 205 and more, beyond the batch's LDS budget (201 rows
    of 52 quads are 167 KB against 156 KB)."""
    d = kind_case("both")
    return dict(d, constraints=list(d["constraints"]) + [("<=", [("x", 1), ("y", 1)], 100 + i) for i in range(198)])


def tolerance_case():
    """max x, x <= 3 + one ulp, x integer: the root's x is 2**-22 = 4 * 2**-24 off an integer -- within 4 eps_s."""
    return dict(type="max", vars=["x"], objective_var="z", objective=[("x", 1)], bounds=[],
                constraints=[("<=", [("x", 1)], np.nextafter(F32(3), F32(4)))], integer_vars=["x"])


def infeasible_case():
    """0.25 <= x <= 0.75 with x integer: both children of the root are infeasible."""
    return dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", 1)], bounds=[],
                constraints=[("<=", [("x", 1)], F32(0.75)), (">=", [("x", 1)], F32(0.25)), ("<=", [("y", 1)], 2)],
                integer_vars=["x"])


def unbounded_case():
    return dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", 1)], bounds=[],
                constraints=[("<=", [("x", 1), ("y", -1)], F32(1.5))], integer_vars=["x"])
