"""Two-phase tableaux whose basic columns are NOT unit vectors (host only, numpy + the C oracle).

Between the phases the reference copies the rows and re-eliminates the main objective row one basic row after
the other (src/simplex.lisp:437-451); the scale of step i is the objective entry of basis[i] AS THE STEPS BEFORE
IT LEFT IT.  On build-tableau's output the basic columns are exact unit vectors, the reduced scale is the
original coefficient, and a kernel that takes all scales up front cannot be told from the sequential loop.  The
entry points accept any tableau, so here are tableaux on which the two differ:

  * DIRECT cases: the artificial tableau has an all-(+0.0) objective row, so phase 1 is optimal after 0 pivots,
    the feasibility test passes and the hand-over sees exactly the arrays written here.  Entries are dyadic
    (k / 8); the basic block B[i][k] = entry of row i in column basis[k] has a unit diagonal, a full
    superdiagonal and a sparse rest -- entries ABOVE the diagonal, in rows whose own scale is non-zero, are what
    changes a later scale.  The off-diagonal entries are at most 1/2 in size and few enough per column that the
    chain of scales does not grow with the number of rows.
  * `unbounded=True` ("unbounded at once"): one non-basic main column has all-zero constraint rows and the
    objective coefficient -2**20 of a max problem.  Every product against it is a zero, it wins pricing, the
    ratio test finds no row: phase 2 ends UNBOUNDED after 0 pivots and the main tableau read back is the pure
    hand-over output -- for entry points that cannot stop before phase 2.
  * LIVED cases: build-tableau pairs of random_mixed_problem with 30 % of the off-diagonal entries of the basic
    columns set to small dyadics; phase 1 really pivots (on the dense representation) before the hand-over.

replay_handover is the plain transcription of :437-451 the GPU tests compare against where they stop before
phase 2; tests/test_handover_cases_host.py shows on the oracle alone that it IS the oracle's hand-over, and that
on every case the shortcut (original coefficients as scales) gives other bits -- conditions on the inputs, not
measurements.  No case holds a basis entry outside [0, number of artificial-tableau variables) or a repeated
one: the device loops index with it."""
import functools
from collections import namedtuple

import numpy as np

import oracle
from tests.helpers import lp_amd, random_mixed_problem

F = 1024.0                                                 # fp-tolerance factor of every case
Case = namedtuple("Case", "name art art_basis main main_basis ingredients")
Prepared = namedtuple("Prepared", "status art art_basis n_phase1 driveout_elements")
Expected = namedtuple("Expected", "status npv art art_basis main main_basis")
Census = namedtuple("Census", "scales objective driveouts zero_flips")


def replay_handover(A, art_basis, main, shortcut=False):
    """src/simplex.lisp:437-451 on float64 arrays, in orc_solve_two_phase's operation order (prod = scale *
    row[c]; obj[c] = obj[c] - prod; a step whose scale == 0.0 is skipped) -> (main tableau, scales).
    shortcut=True reads every scale from the ORIGINAL objective row instead: what a column-parallel kernel
    does, right on unit basic columns only (the census uses it to show that such a kernel would be seen)."""
    M = np.array(main, dtype=np.float64, copy=True)
    m, nv = M.shape[0] - 1, M.shape[1] - 1
    M[:m, :nv] = A[:m, :nv]
    M[:m, nv] = A[:m, -1]
    c0 = M[m].copy()
    scales = np.zeros(m)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(m):
            scale = c0[art_basis[i]] if shortcut else M[m, art_basis[i]]
            scales[i] = scale
            if scale != 0.0:
                prod = scale * M[i]
                M[m] = M[m] - prod
    return M, scales


def prepare(case):
    """Phase 1, the feasibility test and the drive-out pivots (:403-434) on copies -> Prepared; status OPTIMAL
    means the hand-over is next, on (.art, .art_basis)."""
    A, ab = case.art.copy(), case.art_basis.copy()
    m, nv = A.shape[0] - 1, case.main.shape[1] - 1
    st, n1, _ = oracle.solve(A, ab, is_max=False, factor=F)
    elements = []
    if st == oracle.OPTIMAL and not abs(0.0 - A[m, -1]) <= F * oracle.EPSILON:
        st = oracle.INFEASIBLE
    for i in range(m if st == oracle.OPTIMAL else 0):
        if ab[i] < nv:
            continue
        if A[i, -1] != 0.0:
            st = oracle.ART_NONZERO
            break
        new = [j for j in range(nv) if A[i, j] != 0.0 and j not in ab]
        if not new:
            st = oracle.ART_STUCK
            break
        elements.append(float(A[i, new[0]]))
        oracle.pivot(A, ab, new[0], i)
    return Prepared(st, A, ab, n1 + len(elements), tuple(elements))


@functools.lru_cache(maxsize=None)
def _expected(name):
    case = CASES[name]
    A, ab, M, mb = case.art.copy(), case.art_basis.copy(), case.main.copy(), case.main_basis.copy()
    with np.errstate(all="ignore"):
        st, npv = oracle.solve_two_phase(A, ab, M, mb, main_is_max=True, factor=F)
    for a in (A, ab, M, mb):
        a.setflags(write=False)
    return Expected(st, (int(npv[0]), int(npv[1])), A, ab, M, mb)


def expected(case):
    """The oracle's two-phase solve of the case (computed once, read-only)."""
    return _expected(case.name)


@functools.lru_cache(maxsize=None)
def _handed_over(name):
    case = CASES[name]
    p = prepare(case)
    M = None
    if p.status == oracle.OPTIMAL:
        M, _ = replay_handover(p.art, p.art_basis, case.main)
        M.setflags(write=False)
    for a in (p.art, p.art_basis):
        a.setflags(write=False)
    return p, M


def handed_over(case):
    """(Prepared, main tableau right after the hand-over or None) -- computed once, read-only."""
    return _handed_over(case.name)


def same_bits(G, M):
    """Bit for bit, except that any NaN equals any NaN (the payload of inf * 0 is the hardware's choice)."""
    G, M = np.asarray(G), np.asarray(M)
    if G.shape != M.shape:
        return False
    nan = np.isnan(M)
    return bool(np.array_equal(np.isnan(G), nan) and np.array_equal(G.view(np.int64)[~nan], M.view(np.int64)[~nan]))


def census(case):
    """(scales that differ between the reference's replay and the shortcut's, main objective entries that
    differ, drive-out pivots, scales that are zero in one replay and non-zero in the other), on the arrays the
    hand-over sees; None where the case does not reach it."""
    p = prepare(case)
    if p.status != oracle.OPTIMAL:
        return None
    M, s = replay_handover(p.art, p.art_basis, case.main)
    Ms, ss = replay_handover(p.art, p.art_basis, case.main, shortcut=True)
    differ = lambda a, b: int(np.sum(~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))))
    return Census(differ(s, ss), differ(M[-1], Ms[-1]), len(p.driveout_elements), int(np.sum((s == 0.0) != (ss == 0.0))))


# ------------------------------------------------------------------------------------------ direct cases
def _dyadic(rng, shape, lo=-16, hi=16):
    return rng.integers(lo, hi + 1, shape).astype(np.float64) / 8.0


def _nonzero_dyadic(rng, shape):                           # +-1/8 .. +-1/2
    return rng.integers(1, 5, shape).astype(np.float64) / 8.0 * rng.choice([-1.0, 1.0], shape)


def direct(name, m, nv, seed, density, na=2, unbounded=False, ingredients=(), art_objective=0.0):
    """m rows, nv main variables, na artificial columns; basic columns = m distinct main columns in shuffled
    order (never column 0, nor the column of the unbounded-at-once switch)."""
    rng = np.random.default_rng(seed)
    cols = 1 + rng.permutation(nv - 2)[:m]                 # column 0 and column nv - 1 stay non-basic
    A = np.zeros((m + 1, nv + na + 1))
    A[:m, :nv] = _dyadic(rng, (m, nv))
    A[:m, nv:nv + na] = _dyadic(rng, (m, na))              # non-basic artificial columns: never copied
    A[:m, -1] = rng.integers(1, 33, m) / 8.0
    B = np.where(rng.uniform(size=(m, m)) < density, _nonzero_dyadic(rng, (m, m)), 0.0)
    i = np.arange(m - 1)
    B[i, i + 1] = _nonzero_dyadic(rng, m - 1)              # full superdiagonal: every later scale changes
    np.fill_diagonal(B, 1.0)
    A[:m, cols] = B
    A[m, -1] = art_objective
    M = np.zeros((m + 1, nv + 1))
    M[:m] = 7.0                                            # (the copy overwrites every constraint row)
    c = rng.integers(1, 17, nv + 1) / 8.0 * rng.choice([-1.0, 1.0], nv + 1)
    M[m] = c
    if unbounded:
        A[:m, nv - 1] = 0.0
        M[m, nv - 1] = -2.0 ** 20
    return Case(name, A, cols.astype(np.int64), M, np.arange(m, dtype=np.int64), frozenset(ingredients))


def _small(name, seed, ingredients=("a", "b", "c"), unbounded=False, **kw):
    """5 x 9 by hand on top of direct(): with s_k the scale of step k and c the main objective row,
      c[b0] = 2, B[0][1] = 1/2, c[b1] = 1      -> s1 = 1 - 2 * 1/2 = 0: skipped; the shortcut uses 1      (a)
      c[b2] = +0.0, B[0][2] = 1/4              -> s2 = 0 - 2 * 1/4 = -1/2: a zero that became non-zero    (b)
      c[b3] = -0.0, B[0][3] = B[2][3] = 0      -> s3 is a zero (the only entry above it is in skipped row 1) (c)
      c[b4] = 3/2, B[2][4] = 1/4               -> s4 differs as well."""
    case = direct(name, 5, 9, seed, 0.0, na=4, unbounded=unbounded, ingredients=ingredients, **kw)
    A, b, c = case.art, case.art_basis, case.main[-1]
    B = np.eye(5)
    B[0, 1], B[0, 2], B[1, 2], B[1, 3], B[2, 4], B[3, 4], B[0, 4] = 0.5, 0.25, -0.375, 0.375, 0.25, -0.5, 0.125
    B[3, 0], B[4, 1] = 0.25, -0.125                        # below the diagonal: changes no scale
    A[:5, b] = B
    c[b[0]], c[b[1]], c[b[2]], c[b[3]], c[b[4]] = 2.0, 1.0, 0.0, -0.0, 1.5
    return case


def _small_inf(name, seed, sign):
    """(d): c[b0] = +-inf on top of the 5 x 9 block; column 0 is non-basic with a zero in row 0, so its objective
    entry becomes inf * 0 = NaN at step 0 and stays one: phase 2 prices column 0 first, nothing compares below
    a NaN, it ends OPTIMAL after 0 pivots.  Later scales are NaNs or infinities through real off-diagonals."""
    case = _small(name, seed, ingredients=("d",))
    case.art[0, 0] = 0.0
    case.main[-1, case.art_basis[0]] = sign * np.inf
    return case


def _small_driveout(name, seed, stuck=False, nonzero=False):
    """(e): rows 1 and 3 hold basic ARTIFICIAL columns at level 0; the only eligible main columns of row 1 are
    the last two non-basic ones (+1/2 in the first of them), and -- once that pivot is made -- the only one
    of row 3 is the last (-3/4).  Basic main columns with non-zero entries in these rows come before them
    and must be skipped.
    (f) stuck=True: row 3 alone, and its only non-zero main entries sit in basic columns: ART_STUCK.
    (g) nonzero=True: (e) with 2**-60 as the level of row 3's artificial -- tiny, and no exact zero (:423 tests
    /= 0, not fp=): row 1 is driven out, then row 3 ends the step with ART_NONZERO."""
    case = _small(name, seed, ingredients=("f",) if stuck else ("g",) if nonzero else ("e",))
    A, b = case.art, case.art_basis
    nv = case.main.shape[1] - 1
    for r, art_col in ((3, nv + 2),) if stuck else ((1, nv + 1), (3, nv + 2)):
        A[:5, art_col] = 0.0
        A[r, art_col] = 1.0
        A[(r + 1) % 5, art_col] = 0.25                     # the artificial basic column is no unit column either
        b[r] = art_col
        A[r, -1] = 0.0
    free = [j for j in range(nv) if j not in b]            # non-basic main columns, the former basic ones included
    if stuck:
        A[3, free] = 0.0
        assert np.count_nonzero(A[3, :nv]) > 0
    else:
        A[1, free], A[3, free] = 0.0, 0.0
        A[1, free[-2]], A[1, free[-1]] = 0.5, 0.25
        A[3, free[-1]] = -0.75                             # (a zero in free[-2]: the first pivot leaves row 3 as it is)
    if nonzero:
        A[3, -1] = 2.0 ** -60
    return case


def _boundary(name, m, nv, seed, sign, beyond, na=2):
    """Feasibility boundary (:405-407, |0 - objective| <= f * eps): artificial objective value sign * f * eps
    (passes) or the next double beyond it (INFEASIBLE)."""
    edge = F * oracle.EPSILON
    value = sign * (np.nextafter(edge, np.inf) if beyond else edge)
    return direct(name, m, nv, seed, 0.3, na=na, art_objective=value, ingredients=("beyond" if beyond else "edge",))


def _with_unit_basis(name, m, nv, seed, na=2):
    """The one batch member whose basic columns ARE unit vectors (same shape, same kind of data)."""
    case = direct(name, m, nv, seed, 0.0, na=na, ingredients=("unit",))
    case.art[:m, case.art_basis] = np.eye(m)
    return case


# ------------------------------------------------------------------------------------------ lived cases
def lived(name, shape, problem_seed, seed):
    """build-tableau's pair for random_mixed_problem(*shape, problem_seed) with 30 % of the off-diagonal entries
    of the basic SLACK columns in the rows WITHOUT an artificial variable set to +-1/8 .. +-1/2 (generator
    `seed`).  (Entries in artificial rows, or in artificial columns, would have to be carried into the phase-1
    objective row: left out of it they end phase 1 far from 0 -- INFEASIBLE before the hand-over -- on every
    seed tried.)  The slack columns then couple the <= rows, phase 1 pivots on the dense representation, and
    those of them still basic at the hand-over are no unit columns."""
    lp = lp_amd()
    art, main = lp.build_tableau(random_mixed_problem(lp, *shape, problem_seed))
    A, ab = art.matrix.copy(), art.basis_columns.copy()
    M, m = main.matrix.copy(), len(ab)
    nv = M.shape[1] - 1
    rng = np.random.default_rng(seed)
    hit = (rng.uniform(size=(m, m)) < 0.3) & ~np.eye(m, dtype=bool)
    values = _nonzero_dyadic(rng, (m, m))
    hit[:, ab >= nv] = False                               # no artificial column,
    hit[ab >= nv, :] = False                               # no artificial row
    A[:m, ab] = np.where(hit, values, A[:m, ab])
    return Case(name, A, ab, M, np.arange(m, dtype=np.int64), frozenset(("lived",)))


# Lived seeds, found on the oracle: problem seeds 2 .. 39 x generator seeds 0 .. 2 were run through prepare(),
# replay_handover() and oracle.solve with a pivot cap, and kept where phase 1 ends within f * eps of 0 (most
# problems of the larger shape end it a few hundred ulp away, as tests/test_gpu_parity.py notes), the whole solve
# ends OPTIMAL or UNBOUNDED, phase 1 pivots and at least 3 scales differ between the two replays.
LIVED = {"lived-30": ((30, 10, 8, 4), 2, 2), "lived-80": ((80, 30, 20, 10), 5, 2), "lived-80-b": ((80, 30, 20, 10), 25, 0)}


def _build_cases():
    cases = [
        _small("5x9", 11),
        _small("5x9-unbounded", 11, unbounded=True),
        _small_inf("5x9-inf", 12, +1.0),
        _small_inf("5x9-minus-inf", 12, -1.0),
        _small_driveout("5x9-driveout", 13),
        _small_driveout("5x9-stuck", 13, stuck=True),
        _small_driveout("5x9-nonzero", 13, nonzero=True),
        _with_unit_basis("5x9-unit", 5, 9, 14, na=4),
        _boundary("5x9-beyond", 5, 9, 15, -1.0, True, na=4),
        direct("40x70", 40, 70, 21, 0.05),
        direct("40x70-unbounded", 40, 70, 21, 0.05, unbounded=True),
        direct("40x70-b", 40, 70, 22, 0.05),
        _with_unit_basis("40x70-unit", 40, 70, 23),
        direct("3x1023-unbounded", 3, 1023, 31, 0.5, unbounded=True),
        direct("3x1024-unbounded", 3, 1024, 32, 0.5, unbounded=True),
        direct("130x1100", 130, 1100, 41, 0.02),
        direct("130x1100-unbounded", 130, 1100, 41, 0.02, unbounded=True),
        direct("3x16500-unbounded", 3, 16500, 51, 0.5, unbounded=True),
        direct("1030x1100-unbounded", 1030, 1100, 61, 0.01, unbounded=True),
        _boundary("3x7-minus-edge", 3, 7, 71, -1.0, False),
        _boundary("3x7-minus-beyond", 3, 7, 71, -1.0, True),
        _boundary("3x7-plus-edge", 3, 7, 72, +1.0, False),
        _boundary("3x7-plus-beyond", 3, 7, 72, +1.0, True),
    ]
    cases += [lived(name, shape, pseed, seed) for name, (shape, pseed, seed) in LIVED.items()]
    for c in cases:
        for a in (c.art, c.art_basis, c.main, c.main_basis):
            a.setflags(write=False)
    return {c.name: c for c in cases}


CASES = _build_cases()
DIRECT = [n for n, c in CASES.items() if "lived" not in c.ingredients]
LIVED_NAMES = [n for n, c in CASES.items() if "lived" in c.ingredients]
UNBOUNDED_AT_ONCE = [n for n in DIRECT if n.endswith("-unbounded")]
BOUNDARY = [n for n in DIRECT if n.startswith("3x7-")]
SHAPE = {n: (c.art.shape[0] - 1, c.main.shape[1] - 1) for n, c in CASES.items()}
# Batches: members of one shape; exactly one of each has unit basic columns.
BATCHES = {"5x9": ["5x9-unit", "5x9", "5x9-driveout", "5x9-stuck", "5x9-beyond"],
           "5x9-nonzero": ["5x9-unit", "5x9-nonzero", "5x9-driveout"],      # ART_NONZERO between members that go on
           "40x70": ["40x70", "40x70-unit", "40x70-b"]}
