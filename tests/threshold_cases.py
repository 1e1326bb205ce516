"""Tableaux in which an entry sits exactly AT a threshold of the two scans, or one ulp beyond it, at a CHOSEN pivot of
the solve (host only).

The reference decides by strict comparisons against two thresholds (find-entering-column / find-pivoting-row,
src/simplex.lisp:370-372, :386-387): a row is eligible only if 0 + (f/2) eps < a, a column enters only if
key < 0 - (f/8) eps.  Uniform floats never come near either, so everywhere else in the suite `<=` for `<`, or a
threshold one ulp off, decides nothing.  The planting machinery is that of tests/nonfinite_cases.py (the base data,
target / place / r_start, the row and column swaps that only relabel the trace).

Events ("step j" = pivot index j of the oracle's trace on the planted tableau; before it the trace is the base's):
  T   ratio threshold at step j.  Row R is ISOLATED (structural entries 0) in the last look-ahead workgroup (or
      row 0 / row m - 1); X, the column that enters at step j for the first time, gets M[R, X] = thr (`at`) or
      nextafter(thr, inf) (`beyond`), and b[R] = M[R, X] * 2**-10: R's quotient would be 2**-10, far below every
      other row's.  `at`: R is not eligible, step j is the base's.  `beyond`: step j pivots on (X, R), a pivot
      element of about 5.7e-14 (f = 1024), and the solve goes on with finite numbers.
  P   pricing threshold at the LAST step.  All structural keys but a handful (6 to 10) are made unattractive, so the
      LP ends after j = k_end pivots; column Y is zero but for its key, -ptol (`at`) or nextafter(-ptol, -inf)
      (`beyond`).  Y is zero in every pivot row: its key stays bit-exact through every pivot and every look-ahead
      chain.  `at`: OPTIMAL after k_end pivots.  `beyond`: Y enters at step k_end and has no eligible row:
      UNBOUNDED after the same k_end pivots -- the same trace, another status.  `pos` names where k_end falls in
      the block of the path that runs the case: "first" (k_end % block == 0), "mid", "last".

Every case carries the tolerance factor f; both thresholds are computed as the library computes them, in float64.
tests/test_threshold_cases_host.py asserts on the oracle alone that every case is what it claims."""
import functools
from collections import namedtuple

import numpy as np

import oracle
from tests.nonfinite_cases import (BATCH_SHAPES, CAP, SEEDS, Reference, _base, _swap_cols, _swap_rows,  # noqa: F401
                                   _trace, place, r_start, solve, target)

F = 1024.0
F_SMALL, F_LARGE, F_ROUNDS = 16.0, 2.0 ** 20, 1000.0       # (1000 / 2 and 1000 / 8 times epsilon are no doubles: the products round)

# T: where the shape's seed (nonfinite_cases.SEEDS) does not give, at step j, an entering column that has not entered
# before and a winning quotient above 2**-10, the first seed that does -- (n, m, dense, j, row)
TSEEDS = {(1100, 600, False, 27, "last"): 2, (1100, 600, False, 24, "target"): 2, (1100, 600, False, 27, "target"): 2,
          (700, 333, False, 27, "target"): 3, (512, 256, False, 2, "last"): 2}
# P: seeds whose LP ends OPTIMAL after exactly j pivots, found once with the oracle -- (n, m, dense, shard, j); a min
# case is its max twin with the objective row negated: the same trace
PSEEDS = {(1100, 600, False, None, 15): 80, (1100, 600, False, None, 16): 119, (1100, 600, False, None, 17): 3,
          (1100, 600, False, None, 19): 5, (1100, 600, False, None, 23): 139, (1100, 600, False, None, 24): 259,
          (1100, 600, False, None, 27): 54, (1100, 600, False, None, 32): 580,
          (64, 4200, False, None, 24): 34, (8300, 40, False, None, 31): 11, (16500, 40, False, None, 24): 6,
          (64, 8300, False, None, 27): 4, (1024, 512, False, None, 13): 3, (1024, 512, False, None, 16): 27,
          (2048, 200, False, None, 17): 3,
          (700, 333, False, None, 27): 149, (700, 333, False, (8, 7), 15): 27, (700, 333, False, (3, 1), 24): 36,
          (700, 333, True, (2, 1), 16): 9, (700, 333, True, (8, 5), 15): 31,
          (60, 30, False, None, 7): 5, (60, 30, False, None, 8): 3, (300, 40, False, None, 7): 8, (300, 40, False, None, 8): 4,
          (33, 200, False, None, 7): 11, (33, 200, False, None, 8): 7, (512, 256, False, None, 7): 6, (512, 256, False, None, 8): 3}

# n, m, event, variant, j, kind, f, row (T: "target" | "first" | "last"), dense (basic columns doubled), shard (P:
# (shards, r), Y = the first column of shard r), pos (P on a blocked path: where k_end falls in the block)
Case = namedtuple("Case", "n m ev var j kind f row dense shard pos", defaults=("max", F, "target", False, None, None))
Planted = namedtuple("Planted", "M basis R X Y base_trace")


def case_id(c):
    return "%dx%d-%s(%s)-j%d-%s-f%g%s%s%s%s" % (c.n, c.m, c.ev, c.var, c.j, c.kind, c.f, "" if c.row == "target" else "-" + c.row,
                                               "-dense" if c.dense else "", "-shard%dof%d" % c.shard[::-1] if c.shard else "",
                                               "-" + c.pos if c.pos else "")


def thresholds(f):
    """(thr, ptol) as kernels_launch.inc and the oracle compute them."""
    return 0.0 + (f / 2.0) * oracle.EPSILON, (f / 8.0) * oracle.EPSILON


def position(k_end, block):
    return "first" if k_end % block == 0 else "last" if k_end % block == block - 1 else "mid"


def p_base(seed, n, m, kind, dense, shard):
    """Event P without its key: (M, basis, Y).  6 to 10 structural columns keep their keys, every other one gets
    +(|key| + 0.1) in key space; Y is zero."""
    rng = np.random.default_rng(seed)
    M, basis, _ = _base(rng, n, m, kind)
    sgn = 1.0 if kind == "max" else -1.0
    fixed = r_start(n + m if dense else n, *shard) if shard else None
    pool = np.array([c for c in range(n) if c != fixed])
    attractive = rng.choice(pool, size=int(rng.integers(6, 11)), replace=False)
    dull = np.ones(n, dtype=bool)
    dull[attractive] = False
    M[m, :n][dull] = sgn * (np.abs(M[m, :n][dull]) + 0.1)
    Y = fixed if shard else target(n, 2, set(int(c) for c in attractive))
    assert 0 < Y < n
    M[:, Y] = 0.0
    if dense:
        M[np.arange(m), basis] *= 2.0
    return M, basis, Y


@functools.lru_cache(maxsize=4)
def planted(case):
    """The planted tableau of a case (read-only, shared) with the indices of its event and, for T, the BASE trace
    (the same tableau without the planted entries) up to and including step j."""
    n, m, ev, var, j, kind, f, row, dense, shard, _ = case
    thr, ptol = thresholds(f)
    sgn = 1.0 if kind == "max" else -1.0
    omp = (m + 1) * (n + m + 1) > 4_000_000
    R = X = Y = base_trace = None
    if ev == "T":
        rng = np.random.default_rng(TSEEDS.get((n, m, dense, j, row), SEEDS[(n, m)]))
        M, basis, _ = _base(rng, n, m, kind)
        R = {"first": 0, "last": m - 1}.get(row, target(m))
        M[R, :n] = 0.0
        tr = _trace(M, basis, kind, j + 1, omp)
        X = target(n, 2, set(int(c) for c in tr[:j, 0]))   # (not a column that entered before)
        _swap_cols(M, int(tr[j][0]), X)
        w = int(tr[j][1])                                  # the ordinary winner: into another workgroup than R's
        if m > 256 and w // 256 == R // 256:
            _swap_rows(M, n, w, 1 + w % 200 if R >= 256 else target(m, 1, {R}))
        if dense:
            M[np.arange(m), basis] *= 2.0
        base_trace = _trace(M, basis, kind, j + 1, omp)
        base_trace.setflags(write=False)
        M[R, X] = thr if var == "at" else np.nextafter(thr, np.inf)
        M[R, -1] = M[R, X] * 2.0 ** -10
    else:
        M, basis, Y = p_base(PSEEDS[(n, m, dense, shard, j)], n, m, kind, dense, shard)
        M[m, Y] = sgn * ((0.0 - ptol) if var == "at" else np.nextafter(0.0 - ptol, -np.inf))
    M.setflags(write=False)
    basis.setflags(write=False)
    return Planted(M, basis, R, X, Y, base_trace)


def cap_of(case):
    return 40 if (case.n, case.m) == (64, 8300) else CAP


@functools.lru_cache(maxsize=4)
def reference(case, cap=None):
    """oracle.solve on the planted tableau with the case's factor, capped at CAP (40 on the largest shape) or `cap`:
    computed once, read-only."""
    p = planted(case)
    return solve(p.M, p.basis, case.kind, cap_of(case) if cap is None else cap, case.f)


# ---- the cases -------------------------------------------------------------------------------------------------
def _t(n, m, var, j, **kw):
    return Case(n, m, "T", var, j, **kw)


def _p(n, m, var, j, **kw):
    return Case(n, m, "P", var, j, **kw)


S3 = (1100, 600)
PER_PIVOT = [_t(*S3, "at", 5), _t(*S3, "beyond", 5, kind="min", f=F_SMALL), _t(*S3, "at", 16, row="first", f=F_ROUNDS),
             _t(*S3, "beyond", 16, row="last"), _p(*S3, "at", 19), _p(*S3, "beyond", 17, kind="min", f=F_ROUNDS)]
# (case, block, request sequences too)
TWO_LAUNCH = [(_t(*S3, "at", 15), 16, True), (_t(*S3, "beyond", 16, f=F_ROUNDS), 16, False), (_p(*S3, "at", 16, pos="first"), 16, True),
              (_t(*S3, "at", 23, kind="min", f=F_SMALL), 24, False), (_t(*S3, "beyond", 27, f=F_LARGE), 24, True),
              (_p(*S3, "beyond", 23, kind="min", pos="last"), 24, True)]
# (case, workgroups, block, request sequences too)
PERSISTENT = [
    (_t(*S3, "at", 0), 3, 24, False), (_t(*S3, "beyond", 5, kind="min", f=F_SMALL), 3, 24, False), (_t(*S3, "at", 23, f=F_ROUNDS), 3, 24, True),
    (_t(*S3, "beyond", 24), 3, 24, True), (_t(*S3, "at", 27, row="last"), 3, 24, False),
    (_p(*S3, "at", 24, pos="first"), 3, 24, True), (_p(*S3, "beyond", 23, kind="min", pos="last"), 3, 24, True),
    (_p(*S3, "at", 27, f=F_ROUNDS, pos="mid"), 3, 24, False),
    (_t(*S3, "at", 15), 3, 16, True), (_t(*S3, "beyond", 16, row="first", f=F_LARGE), 3, 16, False),
    (_p(*S3, "at", 15, pos="last"), 3, 16, True), (_p(*S3, "beyond", 32, f=F_SMALL, pos="first"), 3, 16, False),
    (_t(64, 4200, "at", 23), 17, 24, True), (_t(64, 4200, "beyond", 16, f=F_LARGE), 17, 16, False),
    (_p(64, 4200, "at", 24, pos="first"), 17, 24, True),
    (_t(8300, 40, "at", 5, kind="min"), 17, 24, False), (_t(8300, 40, "beyond", 24, f=F_ROUNDS), 17, 24, True),
    (_p(8300, 40, "beyond", 31, pos="last"), 17, 16, True),
    (_t(16500, 40, "at", 24), 33, 24, True), (_t(16500, 40, "beyond", 19, f=F_SMALL), 33, 24, False),
    (_p(16500, 40, "at", 24, f=F_ROUNDS, pos="first"), 33, 24, True),
    (_t(64, 8300, "at", 23), 33, 24, False), (_p(64, 8300, "at", 27, pos="mid"), 33, 24, False),
]
# (P: k_end = 27 is three steps into the second block of 24 and the LAST step of a block of 28)
WIDE = [_t(700, 333, "at", 27), _p(700, 333, "at", 27, f=F_ROUNDS)]
# (case, resident_lds)
RESIDENT = [(_t(1024, 512, "at", 5), 0), (_t(1024, 512, "beyond", 16, f=F_ROUNDS), 0), (_p(1024, 512, "at", 13), 0),
            (_p(1024, 512, "beyond", 16, kind="min", f=F_SMALL), 0)] + \
           [(c, lds) for lds in (0, 1) for c in (_t(2048, 200, "at", 19), _t(2048, 200, "beyond", 5, kind="min", row="first"),
                                                 _p(2048, 200, "at", 17, f=F_ROUNDS))]
SINGLE = sorted(set(PER_PIVOT + [c for c, _, _ in TWO_LAUNCH] + [c for c, _, _, _ in PERSISTENT] + WIDE + [c for c, _ in RESIDENT]),
                key=case_id)

# batches: eight members of one shape with ONE factor (the call's) -- T-at, T-beyond in row 0, T-beyond in the last row,
# P-at, P-beyond, two untouched ones, T-at in row 0 -- (event, variant, j, row); the P members' j: BATCH_P
BATCH_MEMBERS = [("T", "at", 3, "target"), ("T", "beyond", 5, "first"), ("T", "beyond", 2, "last"), ("P", "at", None, "target"),
                 ("P", "beyond", None, "target"), None, None, ("T", "at", 4, "first")]
BATCH_P = {"at": 7, "beyond": 8}
BATCH_KIND_FACTOR = {(60, 30): ("max", F), (300, 40): ("min", F_ROUNDS), (33, 200): ("max", F_SMALL), (512, 256): ("min", F_LARGE)}
BATCH_CAP = 200


@functools.lru_cache(maxsize=8)
def batch(n, m, kind):
    """(Ms, Bs, cases): the untouched members are plain uniform tableaux."""
    assert kind == BATCH_KIND_FACTOR[(n, m)][0]
    f = BATCH_KIND_FACTOR[(n, m)][1]
    Ms, Bs, cases = [], [], []
    for k, ev in enumerate(BATCH_MEMBERS):
        if ev is None:
            M, b, _ = _base(np.random.default_rng(100 + k), n, m, kind)
            cases.append(None)
        else:
            e, var, j, row = ev
            cases.append(Case(n, m, e, var, BATCH_P[var] if e == "P" else j, kind, f, row))
            p = planted(cases[-1])
            M, b = p.M, p.basis
        Ms.append(M)
        Bs.append(b)
    Ms, Bs = np.stack(Ms), np.stack(Bs)
    Ms.setflags(write=False)
    Bs.setflags(write=False)
    return Ms, Bs, tuple(cases)


@functools.lru_cache(maxsize=16)
def batch_reference(n, m, kind, cap):
    Ms, Bs, _ = batch(n, m, kind)
    f = BATCH_KIND_FACTOR[(n, m)][1]
    return tuple(solve(Ms[k], Bs[k], kind, cap, f) for k in range(Ms.shape[0]))


# column partitions: (shards, case); compact shards deal out the slots, dense ones all columns.  T: X lies in the LAST
# shard; P: Y is the first column of shard r > 0 -- every other shard's local winner says optimal
CP = (700, 333)
COLPART = [(2, _t(*CP, "at", 19)), (3, _t(*CP, "beyond", 5, f=F_ROUNDS)), (8, _t(*CP, "at", 16, kind="min")),
           (8, _p(*CP, "at", 15, shard=(8, 7))), (3, _p(*CP, "beyond", 24, kind="min", shard=(3, 1), f=F_SMALL)),
           (3, _t(*CP, "at", 15, dense=True, f=F_LARGE)), (2, _p(*CP, "beyond", 16, kind="min", shard=(2, 1), dense=True)),
           (8, _p(*CP, "at", 15, shard=(8, 5), dense=True, f=F_ROUNDS)),
           # ONE shard: the only partition whose split look-ahead step runs as k_shard_p2p_step on a single GPU
           (1, _t(*CP, "at", 19)), (1, _t(*CP, "beyond", 5, f=F_ROUNDS))]
