"""Cases of the device-built single-float batches in the GLOBAL form (tests/test_single_global_build_host.py and
tests/test_gpu_single_global_build.py): mi355x_sbatch_create_lps_global and mi355x_sbatch_create_nodes_global.

The yardsticks are the ones the LDS-form routes have: the float32 model of tests/single_cases.py (`build`, `solve`,
`two_phase`) for problems, tests/single_lps_cases.assemble_rows for arrays, tests/single_bb_cases (`build_node`,
`search`) for nodes.  Nothing here touches the library, and nothing is generated from the new route's output.

    row_kinds / rows_arrays     one group as arrays, ncv = 3, m rows whose kinds -- slack rows, `=` rows, rows with a
                                slack column that are artificial -- stand on both sides of the row pass's chunk
                                boundaries (a thread of its 256-thread workgroup owns ceil(m / 256) consecutive rows)
    wide_arrays                 m = 5 and as many structural columns as asked for
    kinds_problem               the same row kinds as a problem dict (single_lps_cases.member), for the model
    beyond_group                sc.synthetic's numbers as in single_lps_cases.big_group, at any m
    big_bb_problem              200 constraint rows over three integer variables: node tableaux beyond the LDS budget
"""
import functools

import numpy as np

from tests import single_bb_cases as B
from tests import single_cases as sc
from tests import single_lps_cases as C

F32 = np.float32
ROW_THREADS = 256                                            # the row passes' workgroup (kSgaThreads)

#: (op, negative right-hand side?) -> what the row is after the flip
SLACK, EQ, ART = "slack", "eq", "art"
KIND_OF = {("<=", False): SLACK, (">=", True): SLACK, ("=", False): EQ, ("=", True): EQ, (">=", False): ART, ("<=", True): ART}
_SENSE = {"<=": 0, ">=": 1, "=": 2}


def chunk_of(m):
    return (m + ROW_THREADS - 1) // ROW_THREADS


def chunk_boundaries(m):
    """The first rows of the threads' chunks but the first."""
    return list(range(chunk_of(m), m, chunk_of(m)))


@functools.lru_cache(maxsize=None)
def row_kinds(m, two_phase, seed=0):
    """Two members' row lists [(op, negative?)] with the same numbers of `=` and of artificial rows: member 1 is member
    0 rolled by one row.  two_phase: all six kinds, the first row (`>=`) and the last row (`=`, negated) of member 0
    artificial; otherwise slack rows only, flipped and not."""
    rng = np.random.default_rng(7000 + 10 * m + seed)
    pool = sorted(KIND_OF) if two_phase else [("<=", False), (">=", True)]
    kinds = [pool[int(k)] for k in rng.integers(len(pool), size=m)]
    if two_phase:
        kinds[0], kinds[-1] = (">=", False), ("=", True)
    members = [kinds, kinds[-1:] + kinds[:-1]]
    assert C.counts(members[0]) == C.counts(members[1])
    return members


def kinds_at_boundaries(members, m):
    """(the kinds that stand on the last row of a chunk, those on the first row of the next chunk), over the members."""
    last, first = set(), set()
    for kinds in members:
        for i0 in chunk_boundaries(m):
            last.add(KIND_OF[kinds[i0 - 1]])
            first.add(KIND_OF[kinds[i0]])
    return last, first


_EIGHTHS = np.array([-20, -9, -4, -3, 0, 3, 5, 8, 12, 17, 33], dtype=np.float32) / F32(8)


def arrays_of(members, ncv, seed):
    """(lps n x (m + 1) x (ncv + 1) float32, sense n x m int32): coefficients in eighths, zero among them (a zero of a
    negated row is read as Lisp's integer zero: +0.0), a right-hand side < 0 exactly where the kind says so, some of
    the others exactly 0 and one -0.0 (not flipped)."""
    rng = np.random.default_rng(seed)
    n, m = len(members), len(members[0])
    L = _EIGHTHS[rng.integers(len(_EIGHTHS), size=(n, m + 1, ncv + 1))]
    sense = np.zeros((n, m), dtype=np.int32)
    for q, kinds in enumerate(members):
        for i, (op, negative) in enumerate(kinds):
            sense[q, i] = _SENSE[op]
            mag = F32(int(rng.integers(0 if not negative else 1, 40))) / F32(8)
            L[q, i, ncv] = -mag if negative else mag
        zero = [i for i, (_, negative) in enumerate(kinds) if not negative]
        if zero:
            L[q, zero[len(zero) // 2], ncv] = F32(-0.0)
    return np.ascontiguousarray(L, dtype=F32), sense


@functools.lru_cache(maxsize=None)
def rows_arrays(m, two_phase, ncv=3):
    members = row_kinds(m, two_phase)
    return arrays_of(members, ncv, 100 * m + two_phase)


@functools.lru_cache(maxsize=None)
def expected_rows(m, two_phase, ncv=3):
    """single_lps_cases.assemble_rows of every member of rows_arrays (computed once, shared)."""
    L, sense = rows_arrays(m, two_phase, ncv)
    return [C.assemble_rows(L[q], sense[q]) for q in range(L.shape[0])]


WIDE_KINDS = [("<=", False), (">=", False), ("<=", True), ("=", False), ("<=", False)]      # 4 slack columns, 3 artificial rows


@functools.lru_cache(maxsize=None)
def wide_arrays(ncv):
    """m = 5, two members: the main tableau has ncv + 5 columns, the artificial one ncv + 8."""
    members = [WIDE_KINDS, WIDE_KINDS[-1:] + WIDE_KINDS[:-1]]
    assert C.counts(members[0]) == C.counts(members[1]) == (1, 3)
    return arrays_of(members, ncv, ncv)


def kinds_problem(m, seed, ncv=3):
    """Member 0 of row_kinds(m, two_phase=True) as a problem dict of the model."""
    return C.member(seed, ncv, row_kinds(m, True)[0])


@functools.lru_cache(maxsize=None)
def beyond_group(two_phase):
    """The first shapes the LDS form declines, with sc.synthetic's numbers as in single_lps_cases.big_group: 98 x 300
    single-phase (main 99 x 399: 160 000 bytes against 159 744) and 84 x 300 two-phase (artificial 85 x 469)."""
    m = C.BIG_TWO_PHASE_M + 1 if two_phase else 98
    return [C._synthetic_problem(300, m, seed, two_phase) for seed in (3, 4)]


@functools.lru_cache(maxsize=None)
def config4_group():
    """Two members of 256 x 512, single-phase (main 257 x 769)."""
    return [C._synthetic_problem(512, 256, seed, False) for seed in (1, 2)]


@functools.lru_cache(maxsize=None)
def two_phase_102_group():
    """sc.synthetic(300, 98)'s `<=` rows plus x_j >= 0.125 for j < 3: artificial 102 x 405, main 102 x 402."""
    out = []
    names = ["x%d" % j for j in range(300)]
    for seed in (1, 2):
        M0, _ = sc.synthetic(300, 98, seed=seed)
        cons = [("<=", [(names[j], M0[i, j]) for j in range(300)], M0[i, 398]) for i in range(98)]
        cons += [(">=", [(names[j], 1)], F32(0.125)) for j in range(3)]
        out.append(dict(type="max", vars=names, objective_var="w", objective=[(names[j], F32(-M0[98, j])) for j in range(300)],
                        bounds=[], constraints=cons))
    return out


def many_member():
    """m = 63, ncv = 1: 64 rows of 96 stored floats -- the member the many-members case repeats."""
    kinds = row_kinds(63, True)[0]
    return C.member(63, 1, kinds, zeros=False)


# ------------------------------------------------------------------ branch-and-bound beyond the budget
def big_bb_problem(two_phase=False):
    """Three integer variables, z free (two columns), 200 constraint rows: a node of depth d is 201 + d x 205 + d,
    beyond the LDS budget (202 rows of 52 quads are 168 KB against 156 KB).  two_phase: two of the rows are `>=` rows,
    so every node has artificial rows."""
    rng = np.random.default_rng(3)                           # (the model's search ends within 15 nodes at depth 4)
    names = ["x", "y", "z"]
    cons = [("<=", [(v, B.quarters(rng, 1, 5)) for v in names], B.halves(rng, 8, 20)) for _ in range(3)]
    cons += [("<=", [("z", 1)], F32(2.5)), ("<=", [("z", -1)], F32(1.5))]
    if two_phase:
        cons += [(">=", [("x", 1), ("y", 1)], F32(0.5)), (">=", [("x", 1), ("z", F32(0.5))], F32(0.25))]
    cons += [("<=", [("x", 1), ("y", 1)], 100 + i) for i in range(200 - len(cons))]
    return dict(type="max", vars=names, objective_var="w", objective=[(v, B.quarters(rng, 1, 6)) for v in names],
                bounds=[("z", None, None)], constraints=cons, integer_vars=names)


@functools.lru_cache(maxsize=None)
def big_bb_search(two_phase):
    """(problem dict, the model's Result), computed once per process."""
    d = big_bb_problem(two_phase)
    r = B.search(d)
    assert r.status == sc.OPTIMAL and 5 <= len(r.trace) <= 64, (r.status, len(r.trace))
    return d, r


def big_bb_nodes(depth):
    """Entries of one depth and one number of artificial node rows over x, y and the free z (a negative bound on z
    flips its row)."""
    if depth == 1:
        return [(("x", 0, 2),), (("y", 0, 3),), (("z", 1, -1),), (("z", 0, 1),)]          # no artificial node row
    return [(("x", 1, 1), ("y", 0, 3)), (("z", 0, -1), ("x", 0, 2)), (("y", 1, 2), ("z", 1, -1))]   # one artificial row each
