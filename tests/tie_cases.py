"""Tableaux on which pricing and the ratio test meet EXACT ties at a chosen index distance (host only).

find-entering-column and find-pivoting-row (src/simplex.lisp:362-389) take the first of several equal keys
(iterate's `finding ... minimizing`, strict comparison).  Uniform random floats never tie, so on them a
kernel may break a tie any way it likes without the suite noticing.  Here the data are the uniform floats
of tests/test_gpu_property.py `_random_tableau` with DUPLICATED rows and columns: a duplicated pair keeps
bit-identical keys and quotients until one partner is chosen, so every step whose winner still has a living
partner is an exact tie -- with a non-zero quotient, generic arithmetic and a long LP -- between two indices
exactly `row_d` (`col_d`) apart.  The lower one must win; if it does not, the trace and the tableau differ.

Pairing: index i is a copy of index i - d when i // d is odd.  For d >= size / 2 that is "rows d .. m - 1
are copies of rows 0 .. m - 1 - d"; for smaller d it keeps every index with at most ONE partner, at distance
exactly d (copying row i - d into row i for every i >= d would leave rows d apart equal in chains -- for
d = 1 a tableau of rank one).

Slots.  The compact representation stores the non-basic columns in SLOTS: at upload in the order of their
logical indices; at a pivot the leaving column takes the entering column's slot.  Twins never move before one
of them enters, so between twins the lower logical column always sits in the lower slot, and a reduction that
broke ties on the slot would pass.  Every tableau therefore carries `gadgets` small independent blocks, each of
which ends in ONE tied pricing step whose lower logical column sits in the LAST slots and its partner in the
FIRST (see _gadget): there the logical index, not the slot, must decide.

The seeds below are fixed: tests/test_tie_cases_host.py asserts on the oracle alone that every case the GPU
tests use really has the ties it claims (these are conditions on the inputs, not measurements)."""
import functools
from collections import namedtuple

import numpy as np

import oracle

CAP = 80                                                   # pivots of a capped run (or the LP's end)
Census = namedtuple("Census", "pivots status price_ties ratio_ties ratio_ties_nonzero "
                              "price_dist ratio_dist trace price_pairs inverted")


def _pair(a, d, axis):
    """Along `axis`: index i becomes a copy of index i - d when i // d is odd (d <= 0: nothing)."""
    if d <= 0:
        return
    size = a.shape[axis]
    idx = np.arange(size)
    dst = idx[(idx // d) % 2 == 1]
    src = dst - d
    if axis == 0:
        a[dst] = a[src]
    else:
        a[:, dst] = a[:, src]


GADGET_PIVOTS = 3                                          # pivots a gadget takes before the duplicates' turn


def _gadget(M, basis, g, G, n, m, sgn):
    """Gadget g of G in the last rows (r, r2) of the tableau, all entries dyadic (its arithmetic is exact) and
    its rows and columns zero everywhere else, so it runs on its own -- first, its keys being far larger than
    any other.  Logical columns: u = g, the BASIC unit column of row r; j = G + g, a non-basic copy of it (slot
    g); D2 and D1, the last structural columns (D1 in slot n - G + g).
      1. D1 (key -K) enters in row r (quotients 1 against 2): u leaves INTO D1'S SLOT, key +K, and stays
         bit-identical to j for good; D2's key goes from -K/2 to -1.25 K, its entry in row r2 from 0.25 to 1.
      2. D2 enters in row r2 (its entry in row r is negative): u and j get the key -0.25 K.
      3. u and j tie as the most negative columns: u, the lower LOGICAL column, sits in one of the last slots,
         j in one of the first.  u must enter (row r; D1 leaves); a reduction that prefers the lower slot
         takes j."""
    r, r2 = m - 2 * G + 2 * g, m - 2 * G + 2 * g + 1
    K = 4096.0 + 64.0 * g                                  # distinct: the gadgets run in a fixed order
    d2, d1 = n - G + g, n + g                              # logical; slots n - 2 G + g and n - G + g
    M[r, g] = 1.0
    basis[r] = g
    M[r, G + g] = 1.0
    M[r, d1], M[r2, d1], M[m, d1] = 1.0, 1.0, -sgn * K
    M[r, d2], M[r2, d2], M[m, d2] = -0.75, 0.25, -sgn * K / 2
    M[r, -1], M[r2, -1] = 1.0, 2.0
    slack = n + G + (m - 2 * G) + g                        # the basic unit column of row r2
    M[r2, slack] = 1.0
    basis[r2] = slack


def dup_tableau(rng, n, m, row_d, col_d, kind, gadgets=0):
    """[A | I | b ; -+c | 0 | 0] with the slack basis; A ~ U(-0.5, 1.5), b ~ U(0.5, 5), c ~ U(-0.5, 2);
    rows paired at distance row_d (RHS included), columns at distance col_d (objective entry included);
    0 = no duplicates.

    gadgets = G > 0: the same n + m logical columns and m rows, of which 3 G structural columns and 2 G rows
    belong to the gadgets (_gadget); the duplicated block has n - 3 G columns and m - 2 G rows.  Logical
    columns: [u_0 .. u_G-1 (basic) | j_0 .. | the block's columns | D2_0 .. | D1_0 .. | the other basic unit
    columns]: n non-basic ones in this order in the slots 0 .. n - 1."""
    G = gadgets
    n1, m1 = n - 3 * G, m - 2 * G
    A = rng.uniform(-0.5, 1.5, (m1, n1))
    b = rng.uniform(0.5, 5.0, m1)
    c = rng.uniform(-0.5, 2.0, n1)
    Ab = np.concatenate([A, b[:, None]], axis=1)
    _pair(Ab, row_d, 0)
    A, b = Ab[:, :n1], Ab[:, n1]
    Ac = np.concatenate([A, c[None, :]], axis=0)
    _pair(Ac, col_d, 1)
    A, c = Ac[:m1], Ac[m1]
    sgn = 1.0 if kind == "max" else -1.0
    M = np.zeros((m + 1, n + m + 1))
    basis = np.empty(m, dtype=np.int64)
    M[:m1, 2 * G:2 * G + n1] = A
    M[np.arange(m1), n + G + np.arange(m1)] = 1.0
    basis[:m1] = n + G + np.arange(m1)
    M[:m1, -1] = b
    M[m, 2 * G:2 * G + n1] = -sgn * c
    for g in range(G):
        _gadget(M, basis, g, G, n, m, sgn)
    return M, basis


def census(M0, b0, cap=CAP, is_max=True, factor=1024.0):
    """Replay the oracle step by step (oracle.price / ratio / pivot) for at most `cap` pivots and count the
    steps whose pricing winner was tied with a LATER column, whose ratio winner was tied with a later
    eligible row (and how many of those at a non-zero quotient), and the smallest and largest index distance
    between a winner and its nearest later tied partner ((0, 0) when there was no tie).  It keeps the compact
    representation's slot map (non-basic columns in logical order at the start; the leaving column takes the
    entering column's slot): price_pairs holds (winner, nearest later partner, winner's slot, partner's slot)
    of every tied pricing step, `inverted` counts those where a tied partner sat in a LOWER slot than the
    winner -- where the slot order and the logical order disagree."""
    M, b = M0.copy(), b0.copy()
    m, vc = M.shape[0] - 1, M.shape[1] - 1
    thr = 0.0 + (factor / 2.0) * oracle.EPSILON
    pt = rt = rnz = 0
    pd, rd, pairs = [], [], []
    inverted = 0
    slot = np.full(vc, -1, dtype=np.int64)
    nonbasic = np.setdiff1d(np.arange(vc), b)
    slot[nonbasic] = np.arange(len(nonbasic))
    trace = []
    status = oracle.MAX_PIVOTS
    while True:
        ec = oracle.price(M, is_max=is_max, factor=factor)
        if ec < 0:
            status = oracle.OPTIMAL
            break
        if len(trace) >= cap:
            break
        cr = oracle.ratio(M, ec, factor=factor)
        if cr < 0:
            status = oracle.UNBOUNDED
            break
        obj = M[m, :vc]
        later = np.flatnonzero(obj[ec + 1:] == obj[ec])
        if len(later):
            pt += 1
            pd.append(int(later[0]) + 1)
            partner = ec + 1 + int(later[0])
            pairs.append((ec, partner, int(slot[ec]), int(slot[partner])))
            inverted += int((slot[ec + 1 + later] < slot[ec]).any())
        a = M[:m, ec]
        with np.errstate(all="ignore"):
            q = np.where(thr < a, M[:m, vc] / np.where(thr < a, a, 1.0), np.nan)
        later = np.flatnonzero(q[cr + 1:] == q[cr])
        if len(later):
            rt += 1
            rnz += int(q[cr] != 0.0)
            rd.append(int(later[0]) + 1)
        slot[b[cr]], slot[ec] = slot[ec], -1
        oracle.pivot(M, b, ec, cr)
        trace.append((ec, cr))
    span = lambda d: (min(d), max(d)) if d else (0, 0)     # noqa: E731
    return Census(len(trace), status, pt, rt, rnz, span(pd), span(rd),
                  np.array(trace, dtype=np.int64).reshape(-1, 2), pairs, inverted)


# ---- the cases: (n, m, row_d, col_d) -> seed --------------------------------------------------------------
# single tableaux and column partitions; both senses use the same seed (the min form is the same LP with the
# objective row negated: the same pivots, the same ties)
SEEDS = {
    (1100, 600, 300, 550): 1, (1100, 600, 64, 64): 1, (1100, 600, 1, 1): 1,
    (2000, 900, 450, 1000): 1,
    (64, 4200, 2100, 32): 2, (8300, 40, 20, 4150): 1,
    (64, 8300, 4150, 32): 1, (16500, 40, 20, 8250): 1,
    (64, 4200, 256, 32): 2, (8300, 40, 20, 512): 1,
    (300, 257, 128, 128): 1, (1024, 512, 256, 512): 1, (2048, 200, 100, 1024): 1, (2048, 200, 100, 1): 1,
    (700, 333, 166, 350): 2, (700, 333, 166, 234): 2, (700, 333, 166, 88): 1,
}
# batches: 6 members of one shape, member k drawn from BATCH_SEEDS[shape][k]; the LAST member has no duplicates
GADGETS, MEMBER_GADGETS = 6, 2                             # per single tableau / per batch member with duplicates


def gadgets_of(case):
    """Gadgets of a single-tableau case: 6, or 4 where there are only 40 rows (a gadget takes two of them, and
    the 16 row pairs left must still give 12 tied ratio steps)."""
    return 4 if case[1] == 40 else GADGETS


BATCH_MEMBERS = 6
BATCH_SEEDS = {
    (60, 30, 15, 30): (2, 3, 4, 5, 6, 8),
    (300, 40, 20, 150): (1, 2, 3, 4, 5, 6),
    (33, 200, 100, 16): (1, 2, 3, 5, 7, 8),
    (512, 256, 128, 256): (1, 2, 3, 4, 5, 8),
}
BATCH_UNCAPPED_LIMIT = 400                                 # every member's LP ends before this many pivots
# column partitions: shards -> case; col_d = ceil(700 / shards), so that the partner of every low column lies
# in a LATER shard of the compact form (the structural columns dealt out in contiguous, nearly equal parts).
# Dense shards deal out ALL columns, slack block included: there some pairs share a shard and some do not.
COLPART = {2: (700, 333, 166, 350), 3: (700, 333, 166, 234), 8: (700, 333, 166, 88)}


def shard_of(column, n_columns, shards):
    """The shard that holds `column` when n_columns are dealt out in contiguous parts, the first
    n_columns % shards of them one longer -- how mi355x_colpart_create distributes columns."""
    base, extra = divmod(n_columns, shards)
    cut = extra * (base + 1)
    return column // (base + 1) if column < cut else extra + (column - cut) // base


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=4)
def single(n, m, row_d, col_d, kind, dense=False):
    """(M0, b0) of a single-tableau case, read-only and shared: copy before handing it to the oracle.
    dense: the basic columns doubled -- basis columns that are no unit vectors, which keeps a column partition
    on dense shards (as tests/test_gpu_shard_block.py does)."""
    rng = np.random.default_rng(SEEDS[(n, m, row_d, col_d)])
    M0, b0 = dup_tableau(rng, n, m, row_d, col_d, kind, gadgets_of((n, m, row_d, col_d)))
    if dense:
        M0[np.arange(m), b0] *= 2.0
    return _frozen(M0, b0)


Reference = namedtuple("Reference", "status pivots trace M basis")


@functools.lru_cache(maxsize=4)
def single_reference(n, m, row_d, col_d, kind, dense=False, cap=CAP):
    """oracle.solve on the case, capped: computed once, shared by the tests of the case, read-only."""
    M0, b0 = single(n, m, row_d, col_d, kind, dense)
    M, b = M0.copy(), b0.copy()
    st, npiv, trace = oracle.solve(M, b, is_max=(kind == "max"), max_pivots=cap, trace_cap=cap,
                                   omp=M.size > 4_000_000)
    return Reference(st, npiv, *_frozen(trace, M, b))


@functools.lru_cache(maxsize=8)
def batch(n, m, row_d, col_d, kind):
    """(Ms, Bs) of a batch case: BATCH_MEMBERS members, the last one without duplicates; read-only."""
    seeds = BATCH_SEEDS[(n, m, row_d, col_d)]
    tabs = []
    for k, seed in enumerate(seeds):
        last = k == len(seeds) - 1
        tabs.append(dup_tableau(np.random.default_rng(seed), n, m, 0 if last else row_d, 0 if last else col_d, kind,
                                0 if last else MEMBER_GADGETS))
    return _frozen(np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]))


@functools.lru_cache(maxsize=32)
def batch_reference(n, m, row_d, col_d, kind, cap):
    """Per member: oracle.solve with the cap (0 = to the LP's end); read-only, shared."""
    Ms, Bs = batch(n, m, row_d, col_d, kind)
    out = []
    for k in range(Ms.shape[0]):
        M, b = Ms[k].copy(), Bs[k].copy()
        st, npiv, trace = oracle.solve(M, b, is_max=(kind == "max"), max_pivots=cap, trace_cap=1 << 12)
        out.append(Reference(st, npiv, *_frozen(trace, M, b)))
    return tuple(out)


# ---- signed zeros ------------------------------------------------------------------------------------------
SZ_N, SZ_M, SZ_COL, SZ_LO = 8, 70, 2, 3
SZ_HIGHER = (35, 67)                                       # the other row: in row 3's wave (one v_min_f64 butterfly and one
                                                           # `==` ballot see both zeros) / in another wave (the fold across waves does)


@functools.lru_cache(maxsize=None)
def signed_zero_case(negative_in_lower_row, hi=SZ_HIGHER[1]):
    """Column SZ_COL enters first; rows SZ_LO and hi are eligible in it with RHS +0.0 and -0.0 (or the
    other way round), every other row has a positive RHS: the two quotients are +0.0 and -0.0, which compare
    EQUAL, so the lower row wins -- and the pivot row's RHS, 0 / pivot, keeps the sign it was given, as does
    the other row's (x - a * 0 with the signs as they fall).  A reduction that orders -0.0 before +0.0
    (a hardware minimum does) picks the higher row in one of the two cases."""
    rng = np.random.default_rng(7)
    n, m = SZ_N, SZ_M
    A = rng.uniform(0.25, 1.5, (m, n))
    b = rng.uniform(0.5, 5.0, m)
    c = rng.uniform(0.5, 1.0, n)
    c[SZ_COL] = 3.0
    b[SZ_LO], b[hi] = (-0.0, 0.0) if negative_in_lower_row else (0.0, -0.0)
    M = np.zeros((m + 1, n + m + 1))
    M[:m, :n] = A
    M[np.arange(m), n + np.arange(m)] = 1.0
    M[:m, -1] = b
    M[m, :n] = -c
    return _frozen(M, np.arange(n, n + m, dtype=np.int64))
