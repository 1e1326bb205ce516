"""Oracle branch-and-bound: a sequential, literal restatement of simplex-solver with integer
variables (src/simplex.lisp:462-542), shared by the CPU and the GPU tests of the library's
branch-and-bound job (mi355x_simplex_solver_bb_*).

Two node solvers plug into the same depth-first search:
  * f64: node tableaux built by the product's host build-tableau (mi355x_build_tableau, no GPU
    needed), node LPs solved by the C oracle (orc_solve / orc_solve_two_phase), values read the way
    mi355x_solution_variable reads them -- what the GPU job must reproduce bit for bit;
  * exact: oracle/rational_ref.py on Fractions, integrality = integerp.
The trace rows are those of mi355x_simplex_solver_bb_trace: (parent trace index, branching var or
None, sense 0 `<=` / 1 `>=`, bound, outcome, objective or NaN)."""
import dataclasses
import json
import math
import os
from fractions import Fraction

import numpy as np

import oracle
from oracle import rational_ref
from tests.helpers import ROOT, lp_amd

lp = lp_amd()
EPS = 1.1102230246251568e-16
BB_INFEASIBLE, BB_PRUNED, BB_BRANCHED, BB_INCUMBENT, BB_NOT_BETTER, BB_FAILED = range(6)
OPTIMAL, UNBOUNDED, INFEASIBLE = oracle.OPTIMAL, oracle.UNBOUNDED, oracle.INFEASIBLE


def load_cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_ilp_cases.json")) as f:
        return json.load(f)["cases"]


def _num(x):
    return Fraction(x) if isinstance(x, str) else Fraction(x)


def problem_of(case_problem, exact=False):
    """The fixture's problem as a `Problem` with float numbers, or (exact) with Fractions."""
    conv = _num if exact else (lambda x: float(_num(x)))
    d = case_problem
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=[(v, conv(c)) for v, c in d["objective"]],
                      integer_vars=list(d.get("integer_vars", [])),
                      var_bounds=[(b[0], (None if b[1] is None else conv(b[1]), None if b[2] is None else conv(b[2])))
                                  for b in d.get("bounds", [])],
                      constraints=[(op, [(v, conv(c)) for v, c in e], conv(r)) for op, e, r in d["constraints"]])


def node_problem(base, entry, one=1.0):
    """build-and-solve's problem (:489-500): the entry's rows, newest first, before the problem's."""
    rows = [("<=" if s == 0 else ">=", [(v, one)], b) for v, s, b in entry]
    return dataclasses.replace(base, constraints=rows + list(base.constraints))


def solve_node_f64(problem, fp_tolerance=1024.0):
    """-> (status, (objective, {var: value})) with the library's host build-tableau + the C oracle."""
    npb = lp.native.NativeProblem(problem)
    try:
        tabs = npb.build_tableau()
    except lp.UnboundedProblemError:
        return UNBOUNDED, None
    is_max = problem.type == "max"
    if len(tabs) == 1:
        M, b = tabs[0]
        st, _, _ = oracle.solve(M, b, is_max=is_max, factor=fp_tolerance)
    else:
        (A, ab), (M, b) = tabs
        st, _ = oracle.solve_two_phase(A, ab, M, b, main_is_max=is_max, factor=fp_tolerance)
    if st != OPTIMAL:
        return st, None
    basis, rhs = b.tolist(), M[:-1, -1]

    def basic(col):                                   # `position`: the first match
        return float(rhs[basis.index(col)]) if col in basis else 0.0
    vals = {}
    for v in problem.vars:                            # mi355x_solution_variable, simplex.lisp:81-107
        mp = npb.var_mapping(v)
        if mp[0] == "positive":
            vals[v] = mp[2] + basic(mp[1])
        elif mp[0] == "negative":
            vals[v] = mp[2] + (-basic(mp[1]))
        else:
            vals[v] = basic(mp[1]) - basic(mp[1] + 1)
    return OPTIMAL, (float(M[-1, -1]), vals)


def solve_node_exact(problem):
    d = {"type": problem.type, "vars": problem.vars, "objective_var": problem.objective_var,
         "objective": [[v, c] for v, c in problem.objective_func],
         "bounds": [[v, lb, ub] for v, (lb, ub) in problem.var_bounds],
         "constraints": [[op, [[v, c] for v, c in e], r] for op, e, r in problem.constraints]}
    try:
        t = rational_ref.solve_any(rational_ref.build_tableau(d))
    except rational_ref.Unbounded:
        return UNBOUNDED, None
    except rational_ref.Infeasible:
        return INFEASIBLE, None
    return OPTIMAL, (rational_ref.objective_value(t), {v: rational_ref.tableau_variable(t, v) for v in problem.vars})


def f64_integral(int_tolerance=0):
    if int_tolerance > 0:
        return lambda v: abs(v - round(v)) <= int_tolerance * EPS   # fp= v (round v); round = half even
    return lambda v: v == math.floor(v)


def branch_and_bound(problem, exact=False, fp_tolerance=1024.0, int_tolerance=0, max_nodes=None):
    """simplex-solver, :506-542.  -> (status, incumbent (objective, values) or None, trace)."""
    better = (lambda inc, v: inc < v) if problem.type == "max" else (lambda inc, v: inc > v)
    if exact:
        solve, integral = solve_node_exact, (lambda v: Fraction(v).denominator == 1)
        floor, ceil, one = math.floor, math.ceil, Fraction(1)
    else:
        solve, integral = (lambda p: solve_node_f64(p, fp_tolerance)), f64_integral(int_tolerance)
        floor, ceil, one = (lambda v: float(np.floor(v))), (lambda v: float(np.ceil(v))), 1.0
    stack, best, trace = [((), -1)], None, []
    while stack:
        if max_nodes is not None and len(trace) >= max_nodes:
            raise RuntimeError("oracle node cap reached")
        entry, parent = stack.pop()
        st, res = solve(node_problem(problem, entry, one))
        var, sense, bound = entry[0] if entry else (None, 0, 0.0)
        row = [parent, var, sense, float(bound), None, float("nan")]
        if st == INFEASIBLE:
            row[4] = BB_INFEASIBLE
            trace.append(tuple(row))
            continue
        if st != OPTIMAL:
            row[4] = BB_FAILED
            trace.append(tuple(row))
            return st, None, trace
        obj, vals = res
        row[5] = float(obj)
        viol = next((v for v in problem.integer_vars if not integral(vals[v])), None)   # :474-479
        if viol is not None and best is not None and not better(best[0], obj):
            row[4] = BB_PRUNED
        elif viol is not None:                                                        # gen-entries
            me = len(trace)
            stack.append((((viol, 1, ceil(vals[viol])),) + entry, me))
            stack.append((((viol, 0, floor(vals[viol])),) + entry, me))
            row[4] = BB_BRANCHED
        elif best is None or better(best[0], obj):
            best = (obj, vals)
            row[4] = BB_INCUMBENT
        else:
            row[4] = BB_NOT_BETTER
        trace.append(tuple(row))
    return (OPTIMAL if best is not None else INFEASIBLE), best, trace


def trace_key(trace):
    """Rows comparable bit for bit (NaN objectives included)."""
    return [(p, v, s, float(b).hex(), o, float(x).hex()) for p, v, s, b, o, x in trace]


def random_ilp(seed):
    """A seeded random integer program: 3-12 variables of every mapping kind (default >= 0, lower
    bound offset, both bounds, upper bound only, free), 2-8 rows of mixed senses, max or min, a
    shuffled subset of the variables integer."""
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(3, 13)), int(rng.integers(2, 9))
    names = ["v%d" % i for i in range(n)]
    bounds = []
    for v in names:
        k = rng.integers(0, 7)
        if k == 1:
            bounds.append((v, (float(rng.integers(-3, 3)) + 0.5 * float(rng.integers(0, 2)), None)))
        elif k == 2:
            lb = float(rng.integers(-3, 3))
            bounds.append((v, (lb, lb + float(rng.integers(1, 6)) + 0.25 * float(rng.integers(0, 3)))))
        elif k == 3:
            bounds.append((v, (None, float(rng.integers(0, 6)) + 0.5)))
        elif k == 4 and rng.random() < 0.3:
            bounds.append((v, (None, None)))
    cons = []
    # one <= row over every variable keeps most relaxations bounded
    cons.append(("<=", [(v, float(rng.integers(1, 5))) for v in names], float(rng.integers(5, 30)) + 0.5))
    for _ in range(m - 1):
        op = ["<=", ">=", "="][int(rng.choice(3, p=[0.55, 0.3, 0.15]))]
        k = int(rng.integers(1, n + 1))
        vs = rng.choice(n, size=k, replace=False)
        expr = [(names[i], float(rng.integers(-4, 6)) + 0.5 * float(rng.integers(0, 2))) for i in vs]
        rhs = float(rng.integers(-3, 15)) + 0.25 * float(rng.integers(0, 4))
        if op != "=" and rhs < 0:
            rhs = -rhs                       # as after parsing: `<=` / `>=` rows carry rhs >= 0
        cons.append((op, expr, rhs))
    ints = [names[i] for i in rng.permutation(n)[: int(rng.integers(1, n + 1))]]
    kind = "max" if rng.random() < 0.5 else "min"
    obj = [(v, float(rng.integers(-3, 6)) + 0.5 * float(rng.integers(0, 2))) for v in names]
    return lp.Problem(type=kind, vars=names, objective_var=None, objective_func=obj, integer_vars=ints,
                      var_bounds=bounds, constraints=cons)


def random_cases(count=40, max_nodes=80, first_seed=1000):
    """`count` seeded random integer programs whose oracle search processes between 3 and max_nodes
    nodes, plus every tenth seed whatever its search (root infeasible / unbounded / integral ones
    included); chosen deterministically, seeds tried in order."""
    out, seed = [], first_seed
    while len(out) < count:
        p = random_ilp(seed)
        try:
            res = branch_and_bound(p, max_nodes=max_nodes)
        except RuntimeError:
            res = None
        if res is not None and (len(res[2]) >= 3 or seed % 10 == 0):
            out.append((seed, p, res))
        seed += 1
    return out


# ---- base problems and node lists for the node-assembly tests (test_bb_host.py, test_gpu_bb_assembly.py) ----
# Shapes at which k_bb_rows / k_assemble / k_art_objective (linear-programming_amd/csrc/kernels_bb.inc, kernels_assemble.inc)
# make more than one trip of their strided loops, and numbers whose sums and differences round.
_KINDS = [("v1", (2.5, None)), ("v2", (-1.0, 3.25)), ("v3", (None, 4.5)), ("v4", (None, None)), ("v5", (1.0, 2.0))]
_OFFSET = {"v0": 0.0, "v1": 2.5, "v2": -1.0, "v3": 4.5, "v4": 0.0, "v5": 1.0}      # what a row's rhs is shifted by


def _random_nodes(rng, names, depth, count, fractions=(0.0, 0.1, 0.5, 1.0 / 3.0)):
    """`count` entries of `depth` rows (newest first) on random variables, both senses, bounds around the
    offsets so that some shifted right-hand sides are negative."""
    return [tuple((names[int(rng.integers(0, len(names)))], int(rng.integers(0, 2)),
                   float(rng.integers(-4, 6)) + float(fractions[int(rng.integers(0, len(fractions)))]))
                  for _ in range(depth)) for _ in range(count)]


def tall_base(m, seed):
    """m sparse rows on six variables of every mapping kind: plain `<=`, `>=`, `=`, and `<=` / `>=` rows
    whose shifted right-hand side is negative (negated, sense flipped), mixed through the whole range."""
    rng = np.random.default_rng(seed)
    names = ["v%d" % i for i in range(6)]
    cons = []
    for _ in range(m):
        k = int(rng.choice(5, p=[0.35, 0.1, 0.4, 0.1, 0.05]))
        coef = lambda: round(float(rng.uniform(0.1, 3.0)), 3)
        if k < 3:
            vs = rng.choice(6, size=int(rng.integers(1, 4)), replace=False)
            expr = [(names[int(i)], coef()) for i in vs]
            shift = sum(c * _OFFSET[v] for v, c in expr)
            cons.append((["<=", ">=", "="][k], expr, max(shift, 0.0) + round(float(rng.uniform(0.5, 9.0)), 2)))
        else:                                       # 2.5 * coef(v1) >= 5 > rhs: negated
            expr = [("v1", 2.0 + coef()), (("v0", "v4")[int(rng.integers(0, 2))], coef())]
            cons.append((["<=", ">="][k - 3], expr, round(float(rng.uniform(0.0, 4.0)), 2)))
    return lp.Problem(type="max" if seed % 2 else "min", vars=names, integer_vars=list(names),
                      objective_func=[(v, round(float(rng.uniform(-3.0, 5.0)), 2)) for v in names],
                      var_bounds=list(_KINDS), constraints=cons)


def wide_base(n, n_eq, seed):
    """n variables (the first six of every mapping kind) under one `<=` row over all of them, a `>=` row, a
    negated `<=` row and n_eq sparse `=` rows."""
    rng = np.random.default_rng(seed)
    names = ["v%d" % i for i in range(n)]
    cons = [("<=", [(v, float(rng.integers(1, 5))) for v in names], 10.0 * n + 0.5),
            (">=", [("v0", 1.0), ("v1", 0.7), (names[n - 1], 0.1)], 1.5),
            ("<=", [("v1", 2.0), (names[n - 2], 1.0 / 3.0)], 0.5)]
    for _ in range(n_eq):
        vs = rng.choice(n, size=3, replace=False)
        cons.append(("=", [(names[int(i)], round(float(rng.uniform(0.1, 3.0)), 3)) for i in vs],
                     20.0 + round(float(rng.uniform(0.0, 9.0)), 2)))
    return lp.Problem(type="max", vars=names, integer_vars=names[:8],
                      objective_func=[(v, float(rng.integers(-3, 5)) + 0.5) for v in names[:64]],
                      var_bounds=list(_KINDS), constraints=cons)


def inexact_base(seed):
    """Nine dense rows, seven of them artificial, whose columns hold 1e16-scale entries next to 0.1, 0.7 and
    1/3: the artificial objective row depends on the order of its additions."""
    rng = np.random.default_rng(seed)
    names = ["v%d" % i for i in range(6)]
    small = [0.1, 0.7, 1.0 / 3.0, 1.7, 2.9e-3]

    def coef():
        x = small[int(rng.integers(0, len(small)))] * float(rng.integers(1, 4))
        if rng.random() < 0.3:
            x = float(rng.integers(1, 9)) * 1.1e16
        return x if rng.random() < 0.6 else -x
    cons = [(op, [(v, coef()) for v in names], float(rng.integers(1, 9)) * 3.3e16 + 0.1)
            for op in ("=", ">=", "<=", "=", ">=", "=", "<=", ">=", "=")]
    return lp.Problem(type="min", vars=names, integer_vars=list(names),
                      objective_func=[(v, 0.1 * float(rng.integers(1, 9))) for v in names],
                      var_bounds=list(_KINDS), constraints=cons)


_SHIFTED_BOUNDS = [("v1", (0.1, None)), ("v2", (0.3, 7.7)), ("v3", (None, 0.7)), ("v4", (None, None)),
                   ("v5", (1.0 / 3.0, None))]


def shifted_base():
    """Variables with non-dyadic offsets (v0: none, v1: 0.1, v2: 0.3 and a bound row, v3: upper bound 0.7,
    v4: free, v5: 1/3) under a few rows with non-dyadic coefficients, one of them negated."""
    names = ["v%d" % i for i in range(6)]
    cons = [("<=", [(v, 0.1 * (i + 1)) for i, v in enumerate(names)], 30.7),
            (">=", [("v0", 1.0), ("v1", 0.7), ("v3", -1.0 / 3.0)], 1.1),
            ("<=", [("v1", 3.0), ("v5", 1.0)], 0.3),                   # 0.3 - 3 * 0.1 - 1/3 < 0: negated
            ("=", [("v4", 1.0), ("v5", 0.7), ("v2", -0.1)], 0.9)]
    return lp.Problem(type="max", vars=names, integer_vars=list(names),
                      objective_func=[(v, 0.3 * (i + 1)) for i, v in enumerate(names)],
                      var_bounds=list(_SHIFTED_BOUNDS), constraints=cons)


def shifted_nodes():
    """Depth-3 entries over node rows whose `bound - offset` rounds, is +0.0 (bound = offset: no flip), or
    starts from a bound of -0.0 -- on a variable of every mapping kind, the free one included --, each in
    both senses.  -> (entries, the rows they are made of)."""
    rounds = [("v1", 1.0), ("v5", 2.0), ("v2", 3.0), ("v3", 1.0), ("v1", -0.7), ("v5", 0.1)]
    equal = [("v1", 0.1), ("v5", 1.0 / 3.0), ("v2", 0.3), ("v3", 0.7), ("v0", 0.0), ("v4", 0.0)]
    zeros = [("v0", -0.0), ("v1", -0.0), ("v2", -0.0), ("v3", -0.0), ("v4", -0.0), ("v5", -0.0)]
    rows = [(v, s, b) for v, b in rounds + equal + zeros for s in (0, 1)]
    order = np.random.default_rng(7).permutation(len(rows)).tolist()
    rows = [rows[i] for i in order]
    return [tuple(rows[(i + k) % len(rows)] for k in range(3)) for i in range(len(rows))], rows


def deep_base(seed):
    """Seven variables of every mapping kind, rows of all three senses, two of them negated."""
    rng = np.random.default_rng(seed)
    names = ["v%d" % i for i in range(7)]
    cons = [("<=", [(v, float(rng.integers(1, 5))) for v in names], 30.5),
            (">=", [("v0", 1.0), ("v1", 2.0), ("v3", -1.0)], 1.5),
            ("=", [("v4", 1.0), ("v5", 1.5), ("v6", -0.5)], 0.75),
            ("<=", [("v1", 1.0), ("v2", 1.0)], 0.5),                   # 0.5 - 2.5 + 1 < 0: negated
            (">=", [("v1", 1.0), ("v6", 0.7)], 0.1),                   # negated too: becomes a `<=` row
            (">=", [("v6", 1.0), ("v0", 0.5)], 0.0)]
    return lp.Problem(type="max" if seed % 2 else "min", vars=names, integer_vars=list(names),
                      objective_func=[(v, float(rng.integers(-3, 5)) + 0.5) for v in names],
                      var_bounds=list(_KINDS) + [("v6", (-2.5, None))], constraints=cons)


ASSEMBLY_CASES = ("tall_300", "tall_1030", "wide_main", "wide_art", "inexact", "shifted", "deep")
_assembly = {}


def assembly_case(name):
    """(base problem, node entries of one depth) of a named case, made once."""
    if name not in _assembly:
        rng = np.random.default_rng(sum(name.encode()))
        if name == "tall_300":
            p = tall_base(300, 3)
            nodes = _random_nodes(rng, p.vars, 2, 4)
        elif name == "tall_1030":
            p = tall_base(1030, 4)
            nodes = _random_nodes(rng, p.vars, 3, 3)
        elif name == "wide_main":
            p = wide_base(4200, 2, 5)
            nodes = _random_nodes(rng, p.vars[:8], 2, 4)
        elif name == "wide_art":
            p = wide_base(3800, 300, 6)
            nodes = _random_nodes(rng, p.vars[:8], 2, 3)
        elif name == "inexact":
            p = inexact_base(INEXACT_SEED)
            nodes = _random_nodes(rng, p.vars, 2, 12)
        elif name == "shifted":
            p, nodes = shifted_base(), shifted_nodes()[0]
        elif name == "deep":
            p = deep_base(1)
            nodes = _random_nodes(rng, p.vars, 40, 6)
        else:
            raise KeyError(name)
        _assembly[name] = (p, nodes)
    return _assembly[name]


# chosen on the CPU: the first seeds' sums happen to agree in some order for some node; with this one the
# decreasing-order and the pairwise sum each differ from the increasing-order one at every node (pinned by
# tests/test_bb_host.py)
INEXACT_SEED = 19
_host_nodes = {}


def host_node_tableaux(name):
    """Per node of the case: (main, main basis, art or None, art basis or None) from the host
    build-tableau (mi355x_build_tableau) of the node problem; made once, never written to."""
    if name not in _host_nodes:
        p, nodes = assembly_case(name)
        out = []
        for entry in nodes:
            tabs = lp.native.NativeProblem(node_problem(p, entry)).build_tableau()
            (main, mb), art = (tabs[1], tabs[0]) if len(tabs) == 2 else (tabs[0], None)
            out.append((main, mb, None, None) if art is None else (main, mb, art[0], art[1]))
        for t in out:
            for a in t:
                if a is not None:
                    a.setflags(write=False)
        _host_nodes[name] = out
    return _host_nodes[name]


def sum_orders(art, art_basis, num_cols):
    """The artificial objective row of a host-built artificial tableau recomputed in Python floats three
    ways over the artificial rows (those whose basic column is an artificial one, >= num_cols - 1):
    increasing row order from 0.0, decreasing row order from 0.0, and pairwise.  Artificial columns hold 0."""
    m, nac = art.shape[0] - 1, art.shape[1]
    rows = [r for r in range(m) if art_basis[r] >= num_cols - 1]

    def pairwise(xs):
        return xs[0] if len(xs) == 1 else pairwise(xs[:len(xs) // 2]) + pairwise(xs[len(xs) // 2:])
    inc, dec, pair = [0.0] * nac, [0.0] * nac, [0.0] * nac
    for c in list(range(num_cols - 1)) + [nac - 1]:
        xs = [float(art[r, c]) for r in rows]
        s = 0.0
        for x in xs:
            s = s + x
        inc[c] = s
        s = 0.0
        for x in reversed(xs):
            s = s + x
        dec[c] = s
        pair[c] = pairwise(xs)
    return inc, dec, pair, rows


def assert_sum_order_sensitive(name):
    """The precondition of the artificial-objective check, on the host-built tableaux of the case: at every
    node at least five artificial rows, the increasing-order sum from 0.0 IS the host's artificial objective
    row bit for bit, and the decreasing-order sum and the pairwise sum each differ from it in at least one
    column -- a kernel that summed differently cannot pass."""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for hm, hb, ha, hab in host_node_tableaux(name):
        inc, dec, pair, rows = sum_orders(ha, hab, hm.shape[1])
        assert len(rows) >= 5
        assert np.array_equal(bits(inc), bits(ha[-1]))
        assert (bits(dec) != bits(ha[-1])).any() and (bits(pair) != bits(ha[-1])).any()


def restated_node_tableaux(problem, entry):
    """What the header comment of linear-programming_amd/csrc/kernels_bb.inc lists, restated on plain Python
    floats and lists without any library code: (main rows, main basis, artificial rows or None, artificial basis or None).

    Columns: one per variable (two for a free one), then one slack column per row that is not `=`, in row
    order, then the right-hand side.  Rows: the `x <= ub` rows of doubly-bounded variables (the last
    variable's first), the entry's rows newest first, the problem's rows, the objective row.  A row is
    shifted by coef * offset per bounded variable (product rounded, then the difference), negated whole when
    its right-hand side ends up negative (sense flipped; -0.0 is not negative), and then gets slack +1
    (`<=`, basic) or -1 (`>=`); `>=` and `=` rows are artificial: their main-basis entry is the number of
    columns.  Artificial columns are dealt in decreasing row order; the artificial objective row is the sum of
    the artificial rows in increasing row order from 0.0."""
    bounds = dict(problem.var_bounds)
    kind, col, off, ncv, pushed = {}, {}, {}, 0, []
    for v in problem.vars:
        lb, ub = bounds.get(v, (0.0, None))                      # no entry: the default x >= 0
        col[v] = ncv
        if lb is None and ub is None:
            kind[v], off[v], ncv = "free", 0.0, ncv + 2
            continue
        if lb is not None and ub is not None:
            assert 0.0 <= ub                                     # (no case here has a negative upper bound)
            pushed.insert(0, ("<=", [(v, 1.0)], ub))
        kind[v], off[v] = ("upper", ub) if lb is None else ("lower", lb)
        ncv += 1
    rows = pushed + [("<=" if s == 0 else ">=", [(v, 1.0)], b) for v, s, b in entry] + list(problem.constraints)
    m = len(rows)
    num_cols = ncv + sum(op != "=" for op, _, _ in rows) + 1
    M, basis, art_rows, slack = [], [], [], ncv
    for op, expr, rhs in rows:
        row = [0.0] * num_cols
        for v, c in expr:
            c = float(c)
            if kind[v] == "free":
                row[col[v]], row[col[v] + 1] = c, -c
            else:
                row[col[v]] = c if kind[v] == "lower" else -c
                rhs = rhs - c * off[v]
        row[-1] = rhs
        if rhs < 0.0:
            row = [-x for x in row]
            op = {"<=": ">=", ">=": "<=", "=": "="}[op]
        if op != "=":
            row[slack] = 1.0 if op == "<=" else -1.0
        basis.append(slack if op == "<=" else num_cols)
        if op != "<=":
            art_rows.append(len(M))
        slack += op != "="
        M.append(row)
    obj = [0.0] * num_cols
    for v, c in problem.objective_func:
        c = float(c)
        if kind[v] == "free":
            obj[col[v]], obj[col[v] + 1] = -c, c
        else:
            obj[col[v]] = -c if kind[v] == "lower" else c
            obj[-1] = obj[-1] + c * off[v]
    M.append(obj)
    if not art_rows:
        return M, basis, None, None
    n_art = len(art_rows)
    A = [row[:-1] + [0.0] * n_art + row[-1:] for row in M[:m]]
    abasis = list(basis)
    for k, r in enumerate(reversed(art_rows)):
        A[r][num_cols - 1 + k] = 1.0
        abasis[r] = num_cols - 1 + k
    last = [0.0] * (num_cols + n_art)
    for c in list(range(num_cols - 1)) + [num_cols + n_art - 1]:
        s = 0.0
        for r in art_rows:
            s = s + A[r][c]
        last[c] = s
    A.append(last)
    return M, basis, A, abasis
