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
