"""NaN, infinity and subnormal inputs of the single-float kernels at shapes with several waves, trips and workgroups,
and the float32 model's answers to them (host only: tests/test_single_edge_cases_host.py asserts the conditions,
tests/test_gpu_single_edges.py runs the kernels).

Everything is built from tests/single_cases.py (`solve`, `price`, `ratio`, `two_phase`, `build`, `same_bits`); nothing
here touches the library.  Every function is cached and what it returns is read-only.

    pricing_case     P1-P3: 3 rows with slack columns, n = 4200 (the LDS form and the batches) or 8300 (the pair's
                     1024-thread select); integer-valued entries, the special values only where placed
    ratio_case       R1-R4 (and R2b): 1100 rows (or 300: the pair's 256-thread select), n = 6, only column 2 priced in
    extreme_case     uniform(0.5, 2) * 10 ** integers(lo, hi), random signs, as float32: 8 fixed members per shape
    subnormal_case   synthetic(n, m) with the right-hand side scaled by 2 ** e, e = -130, -140, -147
    handover_*       H1-H4: (art, art basis, main, main basis) pairs for the step between the phases

Geometry the directed cases rely on (kernels_single.inc): pricing gives thread t the quads t, t + THREADS, ... of the
objective row (quad p = columns 4p .. 4p + 3), so at 256 threads columns 1024 .. 1027 are the second trip of thread 0
and at 1024 threads columns 4096 .. 4099 are; a wave is 64 threads = 256 columns.  The ratio test gives thread t the
rows t, t + THREADS, ...; a wave is 64 rows."""
import functools

import numpy as np

from tests import single_cases as sc

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
TINY = np.finfo(F32).tiny                                    # the smallest normal float32
PRICING_CAP, RATIO_CAP, EXTREME_CAP = 2, 3, 60


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _case(M0, b0, is_max, cap):
    """-> (M0, b0, is_max, cap, (status, trace, M, basis)): an input and the model's answer, read-only."""
    st, tr, M, b = sc.solve(M0, b0, is_max, 1024, cap)
    _frozen(M0, b0, M, b)
    return M0, b0, is_max, cap, (st, [tuple(int(v) for v in x) for x in tr], M, b)


def census(M):
    """(subnormals, infinities, NaNs) of a tableau."""
    a = np.abs(M)
    return int(((a > 0) & (a < TINY)).sum()), int(np.isinf(M).sum()), int(np.isnan(M).sum())


# ------------------------------------------------------------------ a. directed pricing cases
#: P1: the minimum -7 tied at the last column of wave 0 (255), the first of wave 1 (256), the first of the second trip
#: at 256 threads (1024) and at 1024 threads (4096); NaNs beside each of them and in the winner's own quad (252)
P1_TIED, P1_NANS = (255, 256, 1024, 4096), (252, 254, 257, 1022, 1025, 4097)
P2_INF, P3_INF, P3_NANS = 4100, 4096, (1, 2, 3)
PRICING = ("P1", "P2", "P3")


@functools.lru_cache(maxsize=None)
def pricing_case(name, n, is_max=True):
    """[A | I | b ; -c | 0 | 0] with 3 rows: A integers 1 .. 4, b = 64, c integers 1 .. 5 (a max problem; the min
    version is the mirrored objective row: the same pivots).
    P1  column 255 enters: the lowest of the tied -7s; no NaN is a candidate (under min, NaN * -1 neither).
    P2  a NaN in column 0 and -inf in column 4100: nothing beats the NaN in column 0 -- OPTIMAL, 0 pivots.
    P3  -3 in column 0, NaNs in its quad mates 1 .. 3, -inf in column 4096, which enters: -inf * 0 = NaN and
        x - -inf = inf go through the whole update; capped at PRICING_CAP pivots."""
    m = 3
    rng = np.random.default_rng(7 * n + 1)
    M = np.zeros((m + 1, n + m + 1), dtype=F32)
    M[:m, :n] = rng.integers(1, 5, size=(m, n)).astype(F32)
    M[np.arange(m), n + np.arange(m)] = 1
    M[:m, -1] = 64
    M[m, :n] = -rng.integers(1, 6, size=n).astype(F32)
    if name == "P1":
        M[m, list(P1_TIED)] = -7
        M[m, list(P1_NANS)] = NAN
    elif name == "P2":
        M[m, 0], M[m, P2_INF] = NAN, -INF
    else:
        assert name == "P3"
        M[m, 0], M[m, list(P3_NANS)], M[m, P3_INF] = -3, NAN, -INF
    if not is_max:
        M[m] = -M[m]
    return _case(M, np.arange(n, n + m, dtype=np.int64), is_max, PRICING_CAP)


# ------------------------------------------------------------------ b. directed ratio cases
RATIO = ("R1", "R2", "R2b", "R3", "R4")
#: per rows: {case: (pivot row, {row: (entry of column 2, right-hand side)}, first eligible row)}
_R = {
    1100: {"R1": (700, {700: (2, NAN), 1090: (1, NAN)}, 700),
           "R2": (1035, {10: (2, 10), 11: (1, NAN), 267: (4, 4), 1035: (4, 2)}, 10),
           "R2b": (267, {10: (2, 10), 11: (1, NAN), 267: (4, 4)}, 10),
           "R3": (900, {700: (2, 64), 701: (1, NAN), 1099: (2, NAN), 900: (4, 8)}, 700),
           "R4": (64, {64: (INF, INF), 319: (INF, INF)}, 64)},
    300: {"R1": (70, {70: (2, NAN), 290: (1, NAN)}, 70),
          "R2": (267, {10: (2, 10), 11: (1, NAN), 267: (4, 4)}, 10),
          "R2b": (139, {10: (2, 10), 11: (1, NAN), 139: (4, 4)}, 10),
          "R3": (200, {70: (2, 64), 71: (1, NAN), 299: (2, NAN), 200: (4, 8)}, 70),
          "R4": (64, {64: (INF, INF), 127: (INF, INF)}, 64)},
}


def ratio_geometry(name, rows=1100):
    """(pivot row, {placed row: (entry, right-hand side)}, first eligible row) of a ratio case."""
    return _R[rows][name]


@functools.lru_cache(maxsize=None)
def ratio_case(name, rows=1100, slack=False):
    """`rows` constraint rows, n = 6, a max problem whose objective row is -1 in column 2 and 0 elsewhere.  Column 2 is
    -1 (not eligible) in every row before the case's first eligible row; behind it every seventh row is eligible with
    the quotient 64 / 1.  The other columns hold integers from -2 .. 4 without 0, the right-hand side is 64.
    R1   the first eligible row (700) has the right-hand side NaN: it wins as a NaN; another NaN at 1090.
    R2   first eligible row 10 (quotient 5), NaN quotient in row 11, quotient 1 in row 267 = 11 + 256, 0.5 in row
         1035 = 11 + 1024: row 1035.  At 256 and at 1024 threads thread 11's own first eligible row is the NaN and a
         later row of the same thread is the minimum.
    R2b  R2 without row 1035: row 267.
    R3   first eligible row 700, finite; NaN quotients in rows 701 and 1099; the strict minimum in row 900.
    R4   inf / inf in the first eligible row 64 and again in row 63 + 256: row 64 wins as a NaN.
    The 300-row versions keep the pattern inside 300 rows (ratio_geometry).  Capped at RATIO_CAP pivots: the NaN
    goes through the pivot row's scaling and a whole update."""
    n, m = 6, rows
    winner, placed, first = _R[rows][name]
    ns = m if slack else 0
    rng = np.random.default_rng(rows)
    M = np.zeros((m + 1, n + ns + 1), dtype=F32)
    M[:m, :n] = rng.choice(np.array([-2, -1, 1, 2, 3, 4]), size=(m, n)).astype(F32)
    if slack:
        M[np.arange(m), n + np.arange(m)] = 1
    M[:m, -1] = 64
    M[:m, 2] = -1
    later = np.arange(first + 1, m)
    M[later[later % 7 == 0], 2] = 1
    for r, (a, b) in placed.items():
        M[r, 2], M[r, -1] = a, b
    M[m, 2] = -1
    basis = np.arange(n, n + m, dtype=np.int64) if slack else np.zeros(m, dtype=np.int64)
    return _case(M, basis, True, RATIO_CAP)


# ------------------------------------------------------------------ c. seeded extreme-magnitude tableaux
#: (lo, hi, seed) per shape (m, n), found by a search over seeds on the model for members that make at least 8 pivots,
#: end with a subnormal, an infinity and a NaN, and hold one of them before the last pivot
EXTREME = {
    (24, 40): ((-12, 30, 4), (-10, 30, 3), (-14, 28, 1), (-8, 32, 10), (-16, 30, 2), (-12, 26, 0), (-6, 34, 16),
               (-20, 24, 5)),
    (61, 97): ((-12, 30, 1), (-10, 30, 1), (-14, 28, 4), (-8, 32, 20), (-16, 30, 15), (-12, 26, 35), (-6, 34, 24),
               (-20, 24, 4)),
    (130, 203): ((-12, 30, 1), (-10, 30, 5), (-14, 28, 20), (-8, 32, 1), (-16, 30, 5), (-12, 26, 38), (-6, 34, 1),
                 (-20, 24, 16)),
}


def extreme_tableau(m, n, lo, hi, seed):
    """The float32 twin of test_extreme_magnitudes_bitwise's generator (A, signs, b, c drawn in that order)."""
    rng = np.random.default_rng(seed)

    def mag(shape):
        return rng.uniform(0.5, 2.0, shape) * 10.0 ** rng.integers(lo, hi + 1, shape)
    M = np.zeros((m + 1, n + m + 1))
    A = mag((m, n))
    M[:m, :n] = A * rng.choice([1.0, 1.0, -1.0], (m, n))
    M[np.arange(m), n + np.arange(m)] = 1.0
    M[:m, -1] = mag(m)
    M[m, :n] = -mag(n)
    with np.errstate(all="ignore"):
        return M.astype(F32), np.arange(n, n + m, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def extreme_case(m, n, k):
    return _case(*extreme_tableau(m, n, *EXTREME[(m, n)][k]), True, EXTREME_CAP)


# ------------------------------------------------------------------ d. subnormal right-hand sides
SUBNORMAL_EXPONENTS = (-130, -140, -147)


def subnormal_tableau(m, n, e):
    M0, b0 = sc.synthetic(n, m)
    M0 = M0.copy()
    M0[:m, -1] = np.ldexp(M0[:m, -1].astype(np.float64), e).astype(F32)
    return M0, b0


@functools.lru_cache(maxsize=None)
def subnormal_case(m, n, e):
    return _case(*subnormal_tableau(m, n, e), True, EXTREME_CAP)


# ------------------------------------------------------------------ e. hand-over cases
H1_VARS, H1_BASIC, H1_ROW1, H1_ROW2 = 600, 40, (40, 290, 300, 520), (255, 256)


def h1_problem(k=0):
    """The wide relative of sc.DRIVEOUT_LP: 600 variables, 6 rows (k: a second member with other numbers).
      row 0  `<=`  x40 <= 0                          x40 enters here in phase 1 (quotient 0, tied with row 1: the
                                                     lower row wins), so column 40 is basic after phase 1
      row 1  `=`   x40 - x290 - x300 - x520 = 0      its artificial stays basic at zero
      row 2  `=`   -x255 - x256 = 0                  ... and this one's
      row 3  `>=`  x41 + x100 >= 2                   an ordinary phase-1 pivot
      rows 4, 5    `<=` rows that bound phase 2
    Phase 1 prices no other column of rows 1 and 2 in (their artificial objective entries are negative); the
    hand-over drives the artificial of row 1 out at column 290 (40 is basic, 300 and 520 are higher) and the one of
    row 2 at column 255 (the last column of the first trip at 256 threads; 256 is the first of the second)."""
    x = ["x%d" % j for j in range(H1_VARS)]
    c = F32(0.7) if k == 0 else F32(1.25)
    cons = [("<=", [(x[H1_BASIC], 1)], 0),
            ("=", [(x[H1_BASIC], 1)] + [(x[j], -1) for j in H1_ROW1[1:]], 0),
            ("=", [(x[H1_ROW2[0]], -1), (x[H1_ROW2[1]], -2 if k else -1)], 0),
            (">=", [(x[41], 1), (x[100], 1)], 2 + k),
            ("<=", [(x[41], 1), (x[100], 2), (x[599], c)], F32(3.5) + F32(k)),
            ("<=", [(x[100], 1), (x[310], 1), (x[599], 2)], 5)]
    return dict(type="max", vars=x, objective_var="w", bounds=[], constraints=cons,
                objective=[(x[41], 1), (x[100], F32(0.5)), (x[310], 2), (x[599], 1), (x[520], 1)])


def _pair_case(A, ab, M, mb):
    _frozen(A, ab, M, mb)
    want = sc.two_phase(A, ab, M, mb, True)
    for key in ("art_trace", "main_trace"):
        want[key] = [tuple(int(v) for v in x) for x in want[key]]
    _frozen(want["A"], want["abasis"], want["M"], want["mbasis"])
    return (A, ab, M, mb), want


@functools.lru_cache(maxsize=None)
def handover_h1(k=0):
    b = sc.build(h1_problem(k))
    return _pair_case(b["art"][0], b["art"][1], b["main"][0], b["main"][1])


def _small_pair():
    """sc.small_pairs()' OPTIMAL member (3 x 6 artificial, 3 x 5 main; the artificial of row 1 in column 4), copied."""
    return [np.array(a) for a in sc.small_pairs()[2]]


@functools.lru_cache(maxsize=None)
def handover_small(name):
    """H2  phase 1 ends OPTIMAL at once (nothing priced in) with a NaN artificial objective: (fp= 0 NaN) is false --
           INFEASIBLE.
       H3  phase 1 ends OPTIMAL at once with objective 0 and the artificial basic in a row whose last column is NaN:
           (/= NaN 0) is true -- ART_NONZERO.
       H4  the main objective row holds inf on column 1, which phase 1 makes basic in row 1: the elimination subtracts
           inf * row -- inf - inf in column 1, inf * 0 = NaN, -inf in column 0 -- and phase 2 pivots under the NaN
           rules (column 0 enters as -inf).
       H0  the unchanged pair, so that a batch holds an ordinary member beside them."""
    A, ab, M, mb = _small_pair()
    if name == "H4":                                         # (0.5 x + y >= 0.5: y, column 1, enters in phase 1)
        b = sc.build(sc.hand_problem([("<=", [("x", 1), ("y", 1)], F32(3.5)), (">=", [("x", F32(0.5)), ("y", 1)], F32(0.5))],
                                     [("x", 1), ("y", F32(0.5))]))
        A, ab, M, mb = [np.array(a) for a in b["art"] + b["main"]]
    m, nav = A.shape[0] - 1, A.shape[1] - 1
    art_row = int(np.where(ab >= M.shape[1] - 1)[0][0])
    if name in ("H2", "H3"):
        A[m, :nav] = -np.abs(A[m, :nav])
        A[m, nav] = NAN if name == "H2" else 0
        if name == "H3":
            A[art_row, nav] = NAN
    elif name == "H4":
        M[m, 1] = INF
    else:
        assert name == "H0"
    return _pair_case(A, ab, M, mb)


HANDOVER_SMALL = ("H2", "H3", "H4", "H0")
