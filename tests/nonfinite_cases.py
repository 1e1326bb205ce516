"""Tableaux in which an infinity or a NaN first matters at a CHOSEN pivot of the solve (host only).

The double-precision kernels keep the reference's behaviour on non-finite tableaux by rules of their own:
a NaN objective entry is no pricing candidate except in logical column 0, where it ends the solve
(find-entering-column, src/simplex.lisp:362-379); a NaN quotient wins only in the first eligible row
(find-pivoting-row, :382-389); and a compact representation that meets a non-finite entering column hands the
pivot over to the dense tableau.  tests/test_gpu_nan_rules.py pins these rules at step 0 of shapes that one wave
or one workgroup decides.  Here the event falls at step j of the oracle's trace -- in the middle of a block of
pending pivots, at its last step, at the first step of the next block -- of tableaux that take 3, 17 and 33
look-ahead workgroups, several resident strips, a batch member larger than a wave, or a column shard.

Base data: the uniform floats of tests/test_gpu_property.py `_random_tableau` (non-degenerate, density 1).
Uniform floats never tie, so swapping two rows or two columns of the base only relabels the trace: that is how
the row and the column that carry an event are put where the case wants them (last look-ahead workgroup, not
lane 0, not the first wave where the workgroup has a second one).

Events ("step j" = pivot index j of the oracle's trace on the planted tableau; before it the trace is the base's):
  C   row R is ISOLATED (structural entries 0: never eligible, never changed while the entering columns hold 0
      there); X, the column that enters at step j for the first time, gets M[R, X] = +inf / -inf / NaN.  At step
      j the entering column is non-finite: a compact representation must hand over to the dense one.
  Q   the same row with M[R, X] = 1 and b[R] = NaN (or inf and inf): a NaN quotient at step j, in row 0 (the
      first eligible row: it is the pivot row), in row m - 1 or in a row between eligible ones (ignored).
  Z0  column 0 is zero but for its objective entry, +inf in key space, and M[Rj, 0] = -inf in step j's pivot
      row: pivot j leaves inf - inf = NaN in column 0's objective entry, the next pricing step says optimal.
  ZY  the same in a column Y != 0: it never enters, the solve goes on, and the sweeps carry a column of
      infinities and NaNs through the rest of the block -- without any hand-over.
  `basic0`: logical column 0 is the BASIC unit column of row 0, so slot 0 of the compact representation holds
      logical column 1; ZY with Y = 1 then plants the NaN in SLOT 0, where a pricing rule keyed on the slot and
      not on the logical column would stop as optimal.

tests/test_nonfinite_cases_host.py asserts on the oracle alone that every case is what it claims."""
import functools
from collections import namedtuple

import numpy as np

import oracle

CAP = 60
NAN, INF = float("nan"), float("inf")
SEEDS = {(1100, 600): 1, (64, 4200): 2, (8300, 40): 1, (16500, 40): 1, (64, 8300): 1,
         (1024, 512): 1, (2048, 200): 1, (700, 333): 2,
         (60, 30): 2, (300, 40): 1, (33, 200): 1, (512, 256): 1,
         # Z0 / ZY need a pivot row at step j that was none before, C / Q an entering column that has not entered
         # before: where the shape's seed does not give that at step j, the first seed that does
         (1100, 600, "Z0", 24): 4, (2048, 200, "Z0", 19): 3, (64, 4200, "Z0", 24): 1, (8300, 40, "Z0", 15): 4,
         (700, 333, "Z0", 27): 3, (1024, 512, "ZY", 19): 3, (1100, 600, "ZY", 15): 2, (700, 333, "C", 27): 1,
         (8300, 40, "ZY", 24): 2}

# n, m, event, variant, j, kind, basic0, dense (basic columns doubled: keeps a column partition on dense shards)
Case = namedtuple("Case", "n m ev var j kind basic0 dense", defaults=("max", False, False))
Planted = namedtuple("Planted", "M basis R X Y Rj base_trace")
Reference = namedtuple("Reference", "status pivots trace M basis")


def case_id(c):
    return "%dx%d-%s%s-j%d-%s%s%s" % (c.n, c.m, c.ev, "" if c.var is None else "(%s)" % (c.var if isinstance(c.var, str) else "-".join(map(str, c.var))), c.j, c.kind,
                                      "-basic0" if c.basic0 else "", "-dense" if c.dense else "")


def place(index, per=1):
    """(workgroup, wave, lane) of the look-ahead thread that owns row `index` (per = 1) or slot `index` (per = 2:
    a thread per column pair); 256 threads per workgroup."""
    t = index // per
    return t // 256, (t % 256) // 64, t % 64


def target(size, per=1, avoid=()):
    """The highest index below size - 1 (and not in `avoid`) whose thread sits in the LAST workgroup, not in lane
    0 and, where that workgroup has a second wave, not in its first."""
    last = place(size - 1, per)[0]
    ok = [i for i in range(size - 1) if place(i, per)[0] == last and place(i, per)[2] != 0 and i not in avoid]
    later = [i for i in ok if place(i, per)[1] != 0]
    return (later or ok)[-1]


def r_start(count, shards, r):
    """First of the `count` columns that shard r holds (contiguous parts, the first count % shards one longer)."""
    return r * (count // shards) + min(r, count % shards)


def _base(rng, n, m, kind, basic_row=None):
    """[A | I | b ; -+c | 0 | 0] with the slack basis.  basic_row = r: logical column 0 is the basic unit column of
    row r instead, the structural columns are 1 .. n and the other rows' unit columns follow."""
    A = rng.uniform(-0.5, 1.5, (m, n))
    rng.uniform(size=(m, n))                               # (_random_tableau's density draw: the same stream)
    b = rng.uniform(0.5, 5.0, m)
    c = rng.uniform(-0.5, 2.0, n)
    M = np.zeros((m + 1, n + m + 1))
    s0 = 0 if basic_row is None else 1                     # structural columns s0 .. s0 + n - 1
    M[:m, s0:s0 + n] = A
    M[m, s0:s0 + n] = -c if kind == "max" else c
    M[:m, -1] = b
    basis = np.arange(n, n + m, dtype=np.int64)
    if basic_row is not None:
        basis[np.arange(m) != basic_row] = n + 1 + np.arange(m - 1)
        basis[basic_row] = 0
    M[np.arange(m), basis] = 1.0
    return M, basis, s0


S0_PIVOTS = 3
S0_K = 1.2e308


def _s0_gadget(M, basis, rows, cols, sgn):
    """Three rows and three columns of their own (zero everywhere else), keys near 1e308: they run first.
    u = the basic unit column of row r1.
      0. D1 (key -K) enters in r1 (quotients 1 against 5 in r3): u leaves INTO D1'S SLOT -- the last one -- with
         the key +K and the entries 1 in r2 and -1 in r3 (D1 holds -1 and 1 there).
      1. D2 (key -0.9 K) enters in r2 (its only entry): u's key K + 0.9 K overflows to +inf.
      2. E (key -K / 4) enters in r3 (entry 0.01): the pivot row holds -100 in u, the product with E's key
         overflows to +inf, and u's key is inf - inf = NaN.  (The unit columns that left keep keys >= 0.)
    u = logical column 0: the next pricing step says optimal after 3 pivots -- whatever slot column 0 sits in.
    u = another column: it never enters, the solve goes on."""
    r1, r2, r3 = rows
    d1, d2, e = cols
    m = M.shape[0] - 1
    for r in rows:
        M[r, :-1] = 0.0
        M[r, basis[r]] = 1.0
    M[:, list(cols)] = 0.0
    M[r1, d1], M[r2, d1], M[r3, d1], M[m, d1] = 1.0, -1.0, 1.0, -sgn * S0_K
    M[r2, d2], M[m, d2] = 1.0, -sgn * 0.9 * S0_K
    M[r3, e], M[m, e] = 0.01, -sgn * S0_K / 4
    M[r1, -1], M[r2, -1], M[r3, -1] = 1.0, 1.0, 5.0


def _trace(M0, b0, kind, cap, omp=False):
    M, b = M0.copy(), b0.copy()
    with np.errstate(all="ignore"):
        return oracle.solve(M, b, is_max=(kind == "max"), max_pivots=cap, trace_cap=cap, omp=omp)[2]


def _swap_rows(M, n_struct_end, a, b):
    """Rows a and b trade their structural entries and their RHS (the unit columns stay)."""
    if a != b:
        cols = list(range(n_struct_end)) + [M.shape[1] - 1]
        M[np.ix_([a, b], cols)] = M[np.ix_([b, a], cols)]


def _swap_cols(M, a, b):
    if a != b:
        M[:, [a, b]] = M[:, [b, a]]


@functools.lru_cache(maxsize=4)
def planted(case):
    """The planted tableau of a case (read-only, shared) with the indices of its event and the BASE trace (the
    same tableau without the non-finite entries) up to CAP."""
    n, m, ev, var, j, kind, basic0, dense = case
    rng = np.random.default_rng(SEEDS.get((n, m, ev, j), SEEDS[(n, m)]))
    r3 = target(m)
    M, basis, s0 = _base(rng, n, m, kind, r3 - 2 if (ev, var) == ("S0", "col0") else 0 if basic0 else None)
    s1 = s0 + n                                            # end of the structural columns
    omp = M.size > 4_000_000
    sgn = 1.0 if kind == "max" else -1.0
    R = X = Y = Rj = None
    if ev in ("C", "Q"):
        R = {"first": 0, "last": m - 1}.get(var[1] if ev == "Q" else None, target(m))
        if ev == "Q" and var[1] == "mid":                  # (eligible rows behind it: not among the last ones)
            R = target(m, 1, set(range(m - 9, m)))
        M[R, s0:s1] = 0.0
        tr = _trace(M, basis, kind, j + 1, omp)
        X = s0 + target(n, 2, set(int(c) - s0 for c in tr[:j, 0]))     # (not a column that entered before)
        _swap_cols(M, int(tr[j][0]), X)
        w = int(tr[j][1])                                  # the ordinary winner: into another workgroup than R's
        if m > 256 and w // 256 == R // 256:
            _swap_rows(M, s1, w, 1 + w % 200 if R >= 256 else target(m, 1, {R}))
    elif ev == "S0":                                       # u = column 0 ("col0") or the unit column of r1 ("twin")
        rows = (r3 - 2, r3 - 1, r3)
        _s0_gadget(M, basis, rows, (s1 - 1, s1 - 2, s1 - 3), sgn)
        R, X, Y, Rj = rows[0], s1 - 1, int(basis[rows[0]]), r3
        assert j == S0_PIVOTS - 1
    else:
        if ev == "Z0":
            Y = 0
        elif var is not None:                              # ("shard", shards, r): the first column of shard r
            count = n + m if dense else n
            Y = r_start(count, var[1], var[2])
            assert 0 < Y < n
        else:
            Y = 1 if basic0 else target(n, 2)
        M[:, Y] = 0.0
        tr = _trace(M, basis, kind, j + 1, omp)
        Rj = target(m, 1, set(int(r) for r in tr[:j, 1]))  # (not a pivot row before j)
        _swap_rows(M, s1, int(tr[j][1]), Rj)
    if dense:
        M[np.arange(m), basis] *= 2.0
    base_trace = _trace(M, basis, kind, CAP, omp)
    if ev == "C":
        M[R, X] = {"+inf": INF, "-inf": -INF, "nan": NAN}[var]
    elif ev == "Q":
        M[R, X], M[R, -1] = (1.0, NAN) if var[0] == "nan" else (INF, INF)
    elif ev != "S0":
        M[m, Y] = sgn * INF                                # never the most negative key
        M[Rj, Y] = -INF
    M.setflags(write=False)
    basis.setflags(write=False)
    base_trace.setflags(write=False)
    return Planted(M, basis, R, X, Y, Rj, base_trace)


def solve(M0, b0, kind, cap, factor=1024.0):
    M, b = M0.copy(), b0.copy()
    with np.errstate(all="ignore"):
        st, npiv, trace = oracle.solve(M, b, is_max=(kind == "max"), factor=factor, max_pivots=cap, trace_cap=max(cap, 1),
                                       omp=M.size > 4_000_000)
    for a in (trace, M, b):
        a.setflags(write=False)
    return Reference(st, npiv, trace, M, b)


def cap_of(case):
    return 40 if (case.n, case.m) == (64, 8300) else CAP


@functools.lru_cache(maxsize=4)
def reference(case, cap=None):
    """oracle.solve on the planted tableau, capped at CAP (40 on the largest shape) or `cap`: computed once, read-only."""
    p = planted(case)
    return solve(p.M, p.basis, case.kind, cap_of(case) if cap is None else cap)


# ---- the cases -------------------------------------------------------------------------------------------------
def _c(n, m, ev, var, j, **kw):
    return Case(n, m, ev, var, j, **kw)


S3 = (1100, 600)
PER_PIVOT = [_c(*S3, "C", "nan", 5), _c(*S3, "C", "+inf", 5, kind="min"), _c(*S3, "C", "-inf", 16),
             _c(*S3, "Q", ("nan", "first"), 5), _c(*S3, "Q", ("nan", "mid"), 5, kind="min"),
             _c(*S3, "Q", ("infinf", "last"), 16), _c(*S3, "Z0", None, 5), _c(*S3, "Z0", None, 16, kind="min"),
             _c(*S3, "ZY", None, 5, basic0=True), _c(*S3, "S0", "col0", 2), _c(*S3, "S0", "twin", 2, kind="min")]
# (case, block)
TWO_LAUNCH = [(_c(*S3, "C", "nan", 15), 16), (_c(*S3, "Q", ("nan", "mid"), 16), 16), (_c(*S3, "Z0", None, 19), 16),
              (_c(*S3, "ZY", None, 5), 16),
              (_c(*S3, "C", "-inf", 27), 24), (_c(*S3, "Q", ("nan", "first"), 23), 24), (_c(*S3, "Z0", None, 24), 24),
              (_c(*S3, "ZY", None, 23, kind="min"), 24)]
# (case, workgroups, block)
PERSISTENT = [
    (_c(*S3, "C", "nan", 0), 3, 24), (_c(*S3, "C", "+inf", 5, kind="min"), 3, 24), (_c(*S3, "C", "-inf", 23), 3, 24),
    (_c(*S3, "Q", ("nan", "first"), 24), 3, 24), (_c(*S3, "Q", ("nan", "mid"), 27), 3, 24),
    (_c(*S3, "Q", ("infinf", "last"), 5), 3, 24), (_c(*S3, "Z0", None, 23), 3, 24), (_c(*S3, "Z0", None, 24, kind="min"), 3, 24),
    (_c(*S3, "ZY", None, 5), 3, 24), (_c(*S3, "ZY", None, 27), 3, 24), (_c(*S3, "ZY", None, 23, basic0=True), 3, 24),
    (_c(*S3, "C", "nan", 15), 3, 16), (_c(*S3, "Q", ("nan", "mid"), 16), 3, 16), (_c(*S3, "Z0", None, 19), 3, 16),
    (_c(*S3, "ZY", None, 15), 3, 16), (_c(*S3, "S0", "col0", 2), 3, 24), (_c(*S3, "S0", "twin", 2), 3, 16),
    (_c(64, 4200, "C", "nan", 23), 17, 24), (_c(64, 4200, "Q", ("nan", "mid"), 5), 17, 24),
    (_c(64, 4200, "Z0", None, 24), 17, 24), (_c(64, 4200, "ZY", None, 27), 17, 24), (_c(64, 4200, "C", "-inf", 16), 17, 16),
    (_c(8300, 40, "C", "nan", 5), 17, 24), (_c(8300, 40, "Q", ("nan", "first"), 23), 17, 24),
    (_c(8300, 40, "Z0", None, 27), 17, 24), (_c(8300, 40, "ZY", None, 24), 17, 24), (_c(8300, 40, "Z0", None, 15), 17, 16),
    (_c(16500, 40, "C", "+inf", 24), 33, 24), (_c(16500, 40, "Q", ("nan", "last"), 27), 33, 24),
    (_c(16500, 40, "Z0", None, 5), 33, 24), (_c(16500, 40, "ZY", None, 23), 33, 24), (_c(16500, 40, "S0", "col0", 2, kind="min"), 33, 24),
    (_c(8300, 40, "S0", "col0", 2), 17, 24),
    (_c(64, 8300, "Q", ("nan", "mid"), 23), 33, 24),
]
WIDE = [_c(700, 333, "ZY", None, 5), _c(700, 333, "C", "nan", 27)]      # (C at j = B + 3 for B = 24; inside the second block for 28 too)
# (case, resident_lds)
RESIDENT = [(_c(1024, 512, "C", "nan", 5), 0), (_c(1024, 512, "Q", ("nan", "mid"), 16), 0), (_c(1024, 512, "Z0", None, 15), 0),
            (_c(1024, 512, "ZY", None, 19), 0), (_c(1024, 512, "ZY", None, 5, basic0=True), 0),
            (_c(1024, 512, "S0", "col0", 2), 0), (_c(1024, 512, "S0", "twin", 2), 0)] + \
           [(c, lds) for lds in (0, 1) for c in (_c(2048, 200, "C", "-inf", 16), _c(2048, 200, "Q", ("nan", "first"), 5),
                                                 _c(2048, 200, "Z0", None, 19), _c(2048, 200, "ZY", None, 15),
                                                 _c(2048, 200, "S0", "col0", 2, kind="min"))]
SINGLE = sorted(set(PER_PIVOT + [c for c, _ in TWO_LAUNCH] + [c for c, _, _ in PERSISTENT] + WIDE + [c for c, _ in RESIDENT]),
                key=case_id)

# batches: six members of one shape -- C, Q in row 0, Q in the last row, Z0 and two untouched ones
BATCH_SHAPES = [(60, 30), (300, 40), (33, 200), (512, 256)]
BATCH_MEMBERS = [("C", "nan", 3), ("Q", ("nan", "first"), 5), ("Q", ("nan", "last"), 2), ("Z0", None, 4), None, None]
BATCH_CAP = 200                                            # every member's solve ends before this many pivots, but for a
                                                           # Q member that cycles on its NaN right-hand sides


@functools.lru_cache(maxsize=8)
def batch(n, m, kind):
    """(Ms, Bs, cases): the members' events at different steps; the untouched members are plain uniform tableaux."""
    Ms, Bs, cases = [], [], []
    for k, ev in enumerate(BATCH_MEMBERS):
        if ev is None:
            M, b, _ = _base(np.random.default_rng(100 + k), n, m, kind)
            cases.append(None)
        else:
            cases.append(Case(n, m, *ev, kind=kind))
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
    return tuple(solve(Ms[k], Bs[k], kind, cap) for k in range(Ms.shape[0]))


# column partitions: (shards, case); compact shards deal out the slots, dense ones all columns
CP = (700, 333)
COLPART = [(2, _c(*CP, "C", "nan", 19)), (3, _c(*CP, "Q", ("nan", "mid"), 5)), (2, _c(*CP, "Q", ("nan", "first"), 16)), (8, _c(*CP, "Z0", None, 27)),
           (8, _c(*CP, "ZY", ("shard", 8, 7), 16)), (3, _c(*CP, "Z0", None, 15, dense=True)),
           (2, _c(*CP, "ZY", ("shard", 2, 1), 23, dense=True)), (8, _c(*CP, "ZY", ("shard", 8, 5), 19, dense=True)), (8, _c(*CP, "C", "-inf", 5, dense=True))]
