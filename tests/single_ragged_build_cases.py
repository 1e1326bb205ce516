"""Lists for the ragged single-float batches BUILT ON THE DEVICE (tests/test_single_ragged_build_host.py and
tests/test_gpu_single_ragged_build.py): members of different shapes and senses given as problem rows, and
branch-and-bound nodes of different depths over one base.

The yardstick is the float32 model: tests/single_cases.py (`build`, `solve`, `two_phase`), tests/single_lps_cases.py
(`assemble_rows`, `member`, `feasible_member`, `fits`) and tests/single_bb_cases.py (`assembly_base`,
`assembly_nodes`, `build_node`, `search`).  Every member is a problem dict of single_cases, so the model builds and
solves it by itself.  Nothing here touches the library.
"""
import functools

import numpy as np

from tests import single_bb_cases as B
from tests import single_cases as sc
from tests import single_lps_cases as C

F32 = np.float32
CAP = 200                                           # pivots per member, both phases together; far above every count here

SWEEP_M, SWEEP_NCV = (1, 2, 3, 5, 7), (1, 2, 5)
#: a fixed shuffle of the 15 (m, ncv) pairs: neighbours differ in shape
_ORDER = (7, 2, 11, 0, 13, 5, 9, 14, 3, 8, 1, 12, 6, 10, 4)
_TWO_PHASE_ROWS = ((">=", False), ("<=", False), ("=", False), ("<=", True), (">=", True), ("=", True), ("<=", False))


def shape_of(d):
    """(m, ncv) of a problem dict without bounds: constraint rows and variables."""
    return len(d["constraints"]), len(d["vars"])


def sweep_pairs():
    pairs = [(m, ncv) for m in SWEEP_M for ncv in SWEEP_NCV]
    return [pairs[k] for k in _ORDER]


@functools.lru_cache(maxsize=None)
def sweep_single():
    """15 members, m in {1, 2, 3, 5, 7} x ncv in {1, 2, 5}, shuffled, alternating senses, no artificial row: `<=` rows
    and `>=` rows with a negative right-hand side, which the flip turns into `<=` rows."""
    out = []
    for k, (m, ncv) in enumerate(sweep_pairs()):
        rows = [("<=", False) if (i + k) % 3 else (">=", True) for i in range(m)]
        out.append(C.feasible_member(4000 + k, ncv, rows, "max" if k % 2 else "min"))
    return out


@functools.lru_cache(maxsize=None)
def sweep_two_phase():
    """The same sweep with `>=`, `=` and negative-right-hand-side rows mixed: every member has at least one artificial
    row (row 0), the counts differ from member to member."""
    out = []
    for k, (m, ncv) in enumerate(sweep_pairs()):
        rows = [_TWO_PHASE_ROWS[(i + k) % len(_TWO_PHASE_ROWS)] if i else ((">=", False), ("=", False))[k % 2] for i in range(m)]
        out.append(C.feasible_member(5000 + k, ncv, rows, "min" if k % 2 else "max"))
    return out


def counts_of(d):
    """(`=` rows, artificial rows) of a member by the model's build."""
    b = sc.build(d)
    n_eq = sum(op == "=" for op, _, _ in d["constraints"])
    return n_eq, (0 if b["art"] is None else b["art"][0].shape[1] - b["main"][0].shape[1])


def main_cols(d):
    return sc.build(d)["main"][0].shape[1]


def art_cols(d):
    return sc.build(d)["art"][0].shape[1]


@functools.lru_cache(maxsize=None)
def ld_steps_main():
    """Single-phase members whose main tableaux have 31 / 32 / 33 / 64 / 65 columns (5 `<=` rows each but the last two,
    of 6 and 7 rows: distinct shapes): the leading dimension steps at 32 and 64."""
    out = []
    for k, (cols, m) in enumerate(((31, 5), (32, 5), (33, 5), (64, 6), (65, 7))):
        out.append(C.member(6000 + k, cols - m - 1, [("<=", False)] * m, "max" if k % 2 else "min"))
    return out


@functools.lru_cache(maxsize=None)
def ld_steps_art():
    """A pair whose main tableaux all have 30 columns (ld 32) and whose members have 1 to 4 artificial rows: artificial
    tableaux of 31 to 34 columns, so the artificial leading dimension steps to 64 where the main one does not."""
    out = []
    for n_art in (1, 2, 3, 4):
        m = 4 + n_art                                                    # (distinct m: distinct shapes)
        rows = [(">=", False)] * n_art + [("<=", False)] * (m - n_art)
        out.append(C.member(6100 + n_art, 30 - m - 1, rows, "max" if n_art % 2 else "min"))
    return out


TALL_M = (63, 64, 65, 129, 196)


@functools.lru_cache(maxsize=None)
def tall_members():
    """m in {63, 64, 65, 129, 196} with ncv = 1, single-phase, beside an m = 1 member: the slack prefix crosses waves,
    and 197 x 198 is the largest shape that fits.  Every third row is a `>=` row with a negative right-hand side."""
    out = []
    for k, m in enumerate((63, 1, 64, 65, 129, 196)):
        rows = [(">=", True) if i % 3 == 1 else ("<=", False) for i in range(m)]
        out.append(C.feasible_member(6200 + k, 1, rows, "min" if k in (1, 4) else "max"))    # (max: the solve pivots)
    return out


def negated_zero_member():
    """x + 0 y (an INTEGER zero) <= -3 beside a row that does not mention z: the negated row keeps +0.0."""
    return dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", -1), ("y", -1), ("z", -1)], bounds=[],
                constraints=[("<=", [("x", 1), ("y", 0)], -3), ("<=", [("x", 1), ("y", 1), ("z", 1)], 10)])


@functools.lru_cache(maxsize=None)
def outcome_pair():
    """Two-phase members of every outcome and different shapes: infeasible, optimal, unbounded, an artificial stuck at a
    non-zero value (m = 2), the drive-out members (m = 2, ncv = 3) and members that pivot in both phases (m = 12)."""
    return (list(C.outcome_group()) + list(C.driveout_group()) + list(C.medium_group("max"))[:2] +
            list(C.medium_group("min"))[2:])


@functools.lru_cache(maxsize=None)
def outcome_single():
    """Single-phase members: optimal ones, an unbounded one (m = 3), and synthetic ones of other shapes."""
    out = list(C.single_phase_group())
    for k, (n, m) in enumerate(((7, 5), (9, 6), (11, 3), (40, 24))):
        out.append(C._synthetic_problem(n, m, 7000 + k, False))
    return out


@functools.lru_cache(maxsize=None)
def solution(key, q, cap=CAP):
    """The model's build and solve of member q of the list `key` (a function of this module), computed once."""
    d = globals()[key]()[q]
    b = sc.build(d)
    is_max = d["type"] == "max"
    if b["art"] is None:
        st, tr, M, basis = sc.solve(b["main"][0], b["main"][1], is_max, 1024, cap)
        return dict(build=b, status=st, n=(len(tr),), main_trace=tr, M=M, mbasis=basis)
    r = sc.two_phase(b["art"][0], b["art"][1], b["main"][0], b["main"][1], is_max)
    return dict(build=b, status=r["status"], n=(len(r["art_trace"]), r["n2"]), art_trace=r["art_trace"],
                main_trace=r["main_trace"], M=r["M"], mbasis=r["mbasis"], A=r["A"], abasis=r["abasis"])


SOLVED_LISTS = ("sweep_single", "sweep_two_phase", "outcome_single", "outcome_pair", "ld_steps_art", "ld_steps_main",
                "tall_members")


# ------------------------------------------------------------------ nodes
@functools.lru_cache(maxsize=None)
def node_base(art_base=False):
    """A base on variables of every mapping kind (a free one among them: v4, kind 2) whose deepest node here (depth 5)
    has 24 main columns; art_base: with a `>=` and an `=` row and an artificial bound row, so every node is two-phase."""
    return B.assembly_base(24 + (4 if art_base else 0), 5, art_bound=art_base, n_ge=1 if art_base else 0,
                           n_eq=1 if art_base else 0, seed=3 if art_base else 2)


DEPTHS = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def node_entries(want_art):
    """Two entries per depth in {1, 2, 3, 5}, interleaved.  want_art False: no artificial node row anywhere; True: at
    least one per entry, and the counts differ."""
    out = []
    for j in range(2):
        for d in DEPTHS:
            if not want_art:
                out.append(B.assembly_nodes(100 * j + d, d, 1, want_art=0)[0])
            else:
                out.append(B.assembly_nodes(200 * j + d, d, 1, want_art=1 + (d + j) % min(d, 3) if d > 1 else 1)[0])
    return out


def free_variable_rows(entries):
    """Does some entry bound the free variable v4 (mapping kind 2)?"""
    return any(v == "v4" for e in entries for v, _, _ in e)


# ------------------------------------------------------------------ searches
#: (seed, shape) of single_bb_cases.random_ilp: searches that settle within 64 nodes at depth 8 or less AND have, at
#: bb_width 4, a round whose TWO-PHASE nodes are of two or more depths (found by scanning seeds with the model; asserted
#: in the host test).  The single-phase nodes of a round never are, on these problems: a node is single-phase only while
#: every one of its rows is a `<=` row on a variable with lower bound 0, those nodes lie on ONE path of the tree, one
#: per depth, and a node is solved a round before its child -- the host test asserts that as well.
SEARCH_MIXED_TWO = ((53, 0), (26, 1))


@functools.lru_cache(maxsize=None)
def search_problem(seed, shape):
    """-> (problem dict, the model's Result), computed once per process."""
    p = B.random_ilp(seed, shape)
    r = B.search(p, max_nodes=65)
    assert r.status in (sc.OPTIMAL, sc.INFEASIBLE) and len(r.trace) <= 64 and r.depth <= 8, (seed, shape, r.status, len(r.trace))
    return p, r


@functools.lru_cache(maxsize=None)
def rounds_of(seed, shape, width):
    """The entries of every round of that search at that width: the library's search loop (host Python, no device) over
    the MODEL's node LPs -- what a DeviceRounds is handed, round by round."""
    from tests.helpers import lp_amd
    lp = lp_amd()
    d = B.random_ilp(seed, shape)
    seen = []

    def solve_round(entries):
        seen.append([tuple(e) for e in entries])
        out = []
        for e in entries:
            st, M, basis, mapping = B.solve_node(d, e)
            if st != sc.OPTIMAL:
                out.append((int(st), None, None))
            else:
                out.append((sc.OPTIMAL, sc.objective(M), {v: sc.variable(M, basis, mapping, v) for v in d["vars"]}))
        return out
    lp.exact_bb.search(B.to_problem(lp, d), solve_round, width, 0, fractional=lp.single_bb.fractional(0),
                       floor=lp.single_bb.floor, ceil=lp.single_bb.ceil)
    return seen


def round_depth_sets(seed, shape, width):
    """Per round: (depths of its single-phase nodes, depths of its two-phase nodes), by the model's build; the root
    (no rows) is left out, it never goes through a node batch."""
    d = B.random_ilp(seed, shape)
    out = []
    for entries in rounds_of(seed, shape, width):
        one, two = [], []
        for e in entries:
            if e:
                (two if B.build_node(d, e)[2] is not None else one).append(len(e))
        out.append((one, two))
    return out

