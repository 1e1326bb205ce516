"""Shared cases of the exact branch-and-bound tests (test_exact_bb_host.py, test_gpu_exact_bb.py,
test_gpu_exact_bb_assembly.py): the oracle `solve_round`, seeded random rational integer programs, and
base problems with node lists for the device assembly."""
import dataclasses
from fractions import Fraction as F

import numpy as np

from oracle import rational_ref
from tests import bb_oracle as B
from tests.exact_cases import to_dict
from tests.helpers import lp_amd

lp = lp_amd()


def oracle_round(problem):
    """exact_bb.search's solve_round on oracle/rational_ref.py."""
    def solve_round(entries):
        out = []
        for e in entries:
            st, res = B.solve_node_exact(B.node_problem(problem, e, F(1)))
            out.append((st, res[0], res[1]) if res else (st, None, None))
        return out
    return solve_round


def random_rational_ilp(seed):
    """bb_oracle.random_ilp's shapes on rationals: variables of every mapping kind, bounds and coefficients
    with denominators 2, 3 and 4."""
    rng = np.random.default_rng(seed)
    q = lambda lo, hi: F(int(rng.integers(lo, hi))) + F(int(rng.integers(0, 4)), int(rng.choice([2, 3, 4])))
    n, m = int(rng.integers(3, 9)), int(rng.integers(2, 7))
    names = ["v%d" % i for i in range(n)]
    bounds = []
    for v in names:
        k = int(rng.integers(0, 7))
        if k == 1:
            bounds.append((v, (q(-3, 3), None)))
        elif k == 2:
            lb = q(-3, 3)
            bounds.append((v, (lb, lb + q(1, 6))))
        elif k == 3:
            bounds.append((v, (None, q(0, 6))))
        elif k == 4 and rng.random() < 0.4:
            bounds.append((v, (None, None)))
    cons = [("<=", [(v, F(int(rng.integers(1, 5)))) for v in names], q(5, 30))]
    for _ in range(m - 1):
        op = ["<=", ">=", "="][int(rng.choice(3, p=[0.55, 0.3, 0.15]))]
        vs = rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False)
        rhs = q(-3, 15)
        cons.append((op, [(names[int(i)], q(-4, 6)) for i in vs], abs(rhs) if op != "=" else rhs))
    ints = [names[int(i)] for i in rng.permutation(n)[: int(rng.integers(1, n + 1))]]
    return lp.Problem(type="max" if rng.random() < 0.5 else "min", vars=names, objective_func=[(v, q(-3, 6)) for v in names],
                      integer_vars=ints, var_bounds=bounds, constraints=cons)


_random = []


def random_cases(count=30, max_nodes=80, first_seed=3000):
    """As bb_oracle.random_cases: programs whose oracle search takes 3 .. max_nodes nodes, plus every tenth
    seed whatever its search; made once.  -> [(seed, problem, (status, best, trace))]"""
    seed = first_seed
    while len(_random) < count:
        p = random_rational_ilp(seed)
        try:
            res = B.branch_and_bound(p, exact=True, max_nodes=max_nodes)
        except RuntimeError:
            res = None
        if res is not None and (len(res[2]) >= 3 or seed % 10 == 0):
            _random.append((seed, p, res))
        seed += 1
    return _random[:count]


def reference_tableaux(problem, entry):
    """rational_ref.build_tableau of the node problem: (main rows, main basis, art rows or None, art basis or None)."""
    tabs = rational_ref.build_tableau(to_dict(B.node_problem(problem, entry, F(1))))
    if isinstance(tabs, tuple):
        return tabs[1].matrix, tabs[1].basis, tabs[0].matrix, tabs[0].basis
    return tabs.matrix, tabs.basis, None, None


def wide_ilp(seed=3):
    """exact_cases.wide_problem (coefficients near 2^40) with its variables integer: node tableaux start at 64
    bits and outgrow them within two pivots.  Its numbers are integers, so the integer scale is 1 and
    exact_cases.Model's widths are the device's (pinned on the CPU in test_exact_bb_host.py)."""
    from tests.exact_cases import wide_problem
    p = wide_problem(lp, seed, 40)
    p.integer_vars = list(p.vars)
    return p


# ---- device assembly: bases and node lists ----
_KINDS = [("v1", (F(5, 2), None)), ("v2", (F(-1), F(13, 4))), ("v3", (None, F(9, 2))), ("v4", (None, None)),
          ("v5", (F(1, 3), F(2))), ("v6", (F(7, 10), None))]
_OFFSET = {"v0": F(0), "v1": F(5, 2), "v2": F(-1), "v3": F(9, 2), "v4": F(0), "v5": F(1, 3), "v6": F(7, 10)}
_NAMES = ["v%d" % i for i in range(7)]


def _base(rows, seed, extra_vars=0, only_le=False):
    """`rows` sparse rows with integer coefficients (the integer scale stays small) on seven variables of every
    mapping kind -- offsets 5/2, -1, 9/2, none (free), 1/3, 7/10 -- of all three senses, some negated (only_le:
    plain `<=` rows only, so that no base row is artificial)."""
    rng = np.random.default_rng(seed)
    names = _NAMES + ["w%d" % i for i in range(extra_vars)]
    cons = [("<=", [(v, F(1)) for v in names], F(40 + extra_vars))]
    for _ in range(rows - 1):
        k = 0 if only_le else int(rng.choice(5, p=[0.4, 0.15, 0.15, 0.2, 0.1]))
        vs = rng.choice(len(names), size=int(rng.integers(1, 4)), replace=False)
        expr = [(names[int(i)], F(int(rng.integers(1, 4)))) for i in vs]
        if k < 3:
            shift = sum(c * _OFFSET.get(v, F(0)) for v, c in expr)
            cons.append((["<=", ">=", "="][k], expr, max(shift, F(0)) + int(rng.integers(1, 9))))
        else:                                        # 2 * 5/2 > rhs: negated, sense flipped
            cons.append((["<=", ">="][k - 3], [("v1", F(2)), ("v0", F(1))], F(int(rng.integers(0, 5)))))
    return lp.Problem(type="max" if seed % 2 else "min", vars=names, integer_vars=list(_NAMES),
                      objective_func=[(v, F(int(rng.integers(-3, 5)), 2)) for v in names], var_bounds=list(_KINDS),
                      constraints=cons)


def _nodes(rng, depth, count, want_art):
    """`count` entries of `depth` rows whose shifted right-hand sides are negative, zero and positive in both
    senses; want_art None: whatever comes, else: exactly that many artificial node rows per entry."""
    def row():
        v = _NAMES[int(rng.integers(0, 7))]
        b = int(rng.integers(-4, 7))
        if rng.random() < 0.25 and _OFFSET[v].denominator == 1:
            b = int(_OFFSET[v])                                       # bound = offset: rhs 0, not negated
        return v, int(rng.integers(0, 2)), b

    def art(r):
        return (1 - r[1] if r[2] - _OFFSET[r[0]] < 0 else r[1]) == 1
    out = []
    while len(out) < count:
        e = tuple(row() for _ in range(depth))
        if want_art is None or sum(art(r) for r in e) == want_art:
            out.append(e)
    return out


def big_scale_base():
    """Db near 2^40 (a row with denominators 1048573 and 1048571), so that bound * Db leaves 64 bits for
    bounds near 2^30."""
    cons = [("<=", [("v0", F(1, 1048573)), ("v1", F(1, 1048571))], F(7)), (">=", [("v0", F(1)), ("v1", F(1))], F(1))]
    return lp.Problem(type="max", vars=["v0", "v1"], integer_vars=["v0", "v1"], objective_func=[("v0", F(1)), ("v1", F(2))],
                      constraints=cons)


def bounds_only_base():
    """An integer program without constraints, doubly-bounded variables only: the general form of
    build_tableau(general=True) instead of build-tableau's special case."""
    return lp.Problem(type="max", vars=["v0", "v1", "v2"], integer_vars=["v0", "v1", "v2"],
                      objective_func=[("v0", F(1)), ("v1", F(-1, 2)), ("v2", F(2, 3))],
                      var_bounds=[("v0", (F(1, 2), F(7, 2))), ("v1", (F(-3, 2), F(5, 3))), ("v2", (F(0), F(9, 4)))])


ASSEMBLY_CASES = ("tall_d1", "tall_d3_art", "wide_d3", "small_d40", "small_d1_art", "big_scale", "bounds_only")
_assembly = {}


def assembly_case(name):
    """(base problem, node entries of one depth and one number of artificial rows), made once."""
    if name not in _assembly:
        rng = np.random.default_rng(sum(name.encode()))
        if name == "tall_d1":                       # about 300 rows: the row loops make two trips
            p, nodes = _base(300, 3, only_le=True), _nodes(rng, 1, 4, 0)
        elif name == "tall_d3_art":
            p, nodes = _base(290, 4), _nodes(rng, 3, 3, 2)
        elif name == "wide_d3":                     # about 300 columns
            p, nodes = _base(6, 5, extra_vars=290), _nodes(rng, 3, 4, 1)
        elif name == "small_d40":
            p, nodes = _base(8, 6), _nodes(rng, 40, 3, 17)
        elif name == "small_d1_art":
            p, nodes = _base(5, 7), _nodes(rng, 1, 6, 1)
        elif name == "big_scale":
            p = big_scale_base()
            nodes = [(("v0", 0, (1 << 30) + 5), ("v1", 1, 3)), (("v1", 0, (1 << 30) - 7), ("v0", 1, 2)), (("v0", 0, 9), ("v1", 1, 1))]
        elif name == "bounds_only":
            p = bounds_only_base()
            nodes = [(("v0", 0, 2), ("v1", 1, -1)), (("v2", 1, 1), ("v0", 0, 3)), (("v1", 0, -1), ("v2", 1, 2))]
        else:
            raise KeyError(name)
        _assembly[name] = (p, nodes)
    return _assembly[name]
