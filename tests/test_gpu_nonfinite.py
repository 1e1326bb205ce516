"""Infinities and NaNs that first matter in the MIDDLE of a solve, on every double-precision path.

The reference's scans decide sequentially (find-entering-column / find-pivoting-row, src/simplex.lisp:362-389): a
NaN objective entry never enters, a NaN in column 0's objective entry ends the solve as optimal, a NaN quotient
wins only in the first eligible row.  The kernels restate that for trees over lanes, waves, workgroups, exchange
records, strips and shards (price_cand / price_says_optimal, block_gather_ratio, the `poison` bits of the gather
kernels, k_resident's own copy), and a compact representation that meets a non-finite entering column or a NaN
quotient in a look-ahead step stops its block there (kNeedDense), applies the pending pivots and redoes the
step on the dense tableau.  tests/test_gpu_nan_rules.py pins the rules at step 0 of shapes one workgroup decides.

The tableaux of tests/nonfinite_cases.py meet their event at step j of the oracle's trace -- step 5 of a block,
its last step, the first step of the next block, three steps into it -- at 3, 17 and 33 look-ahead workgroups, in
several resident strips, behind the wide sweeps, in batch members larger than a wave and on column shards
(tests/test_nonfinite_cases_host.py proves on the oracle what every case claims, and that a kernel following
another rule would give another trace):
  C   the entering column of step j holds +inf / -inf / NaN in an isolated row: hand-over at step j;
  Q   a NaN quotient at step j, in the first eligible row (it wins) or behind it (ignored);
  Z0  column 0's objective entry turns inf - inf = NaN at pivot j: optimal after j + 1 pivots;
  ZY  the same in another column: the solve goes on and the sweeps carry a column of infinities and NaNs through
      the rest of the block -- no hand-over (asserted from the path counts: no per-pivot launch);
  S0  logical column 0 leaves the basis into the LAST slot and its objective entry turns NaN there: optimal --
      and its twin on another column goes on; `basic0`: the NaN arises in SLOT 0, which holds logical column 1.

Every comparison is with oracle.solve on the same arrays: status, pivot count, the whole trace, the basis, the
positions of the NaNs and the int64 bits of everything else (x86 and gfx950 differ only in the default NaN's
sign, as in test_gpu_nan_rules.py).  Every case asserts that the path it names is the one that ran."""
import ctypes
import importlib

import numpy as np
import pytest

import oracle
from tests import nonfinite_cases as nc
from tests.helpers import lp_amd
from tests.test_gpu_ties import (BATCH_PATHS, B_RESIDENT, LA_PERSISTENT, LA_TWO_LAUNCH, PER_PIVOT, RESIDENT, SELECT_SPLIT,
                                 _batch_block_fits, _batch_counts, _la_workgroups, _path, knobs)   # noqa: F401 (knobs: fixture)

pytestmark = pytest.mark.gpu
lp = lp_amd()
WIDE_SWEEP = 4                                             # mi355x_tab_path_counts: k_sweepw + k_sweepw_rest


def _hands_over(case):
    """The compact blocked and resident paths stop at step j and go on densely: a non-finite entering column, or
    a NaN quotient whichever row it sits in (the dense path decides whether it wins)."""
    return case.ev in ("C", "Q")


def _same_bits(G, M, what):
    for r0 in range(0, G.shape[0], 1024):
        g, o = G[r0:r0 + 1024], M[r0:r0 + 1024]
        nan_g, nan_o = np.isnan(g), np.isnan(o)
        assert np.array_equal(nan_g, nan_o), (what, "NaN positions", r0)
        assert np.array_equal(g[~nan_g].view(np.int64), o[~nan_o].view(np.int64)), (what, "bits", r0)


def _same(t, ref, what):
    tr = t.pivot_trace()[:ref.pivots]
    if not np.array_equal(tr, ref.trace):
        k = min(len(tr), len(ref.trace))
        bad = np.where((tr[:k] != ref.trace[:k]).any(axis=1))[0]
        raise AssertionError("%s: pivot trace (%d pivots) differs from the oracle's (%d), first at %s: got %s, oracle %s"
                             % (what, len(tr), len(ref.trace), bad[:3], tr[bad[:3]].tolist(), ref.trace[bad[:3]].tolist()))
    assert np.array_equal(t.basis_columns, ref.basis), what
    _same_bits(t.matrix, ref.M, what)


def _tableau(case, cases=nc):
    p = cases.planted(case)
    return lp.Tableau(None, lp.Problem(type=case.kind), p.M, p.basis, case.n + case.m, case.m, {})


def _capped_run(L, case, prepare=False, factor=1024.0, cases=nc):
    """`cases`: the module that plants the case (planted, reference, cap_of); `factor`: the call's tolerance factor."""
    ref = cases.reference(case)
    t = _tableau(case, cases)
    k = ctypes.c_int64(0)
    is_max = int(case.kind == "max")
    if prepare:                                            # -> the compact representation, nothing solved
        lp.capi.check(L.mi355x_tab_solve_async(t._h, is_max, factor, 0, 1), "prepare")
        L.mi355x_tab_sync(t._h, ctypes.byref(k))
        assert L.mi355x_tab_resident(t._h) == 1
    rc = L.mi355x_tab_solve(t._h, is_max, factor, cases.cap_of(case), ctypes.byref(k))
    path = _path(L, t._h)
    t._touch()
    assert (rc, k.value) == (ref.status, ref.pivots), (rc, k.value, ref.status, ref.pivots, path.counts)
    _same(t, ref, "capped run")
    return path, ref


def _request_sequence(L, case, first_piece, factor=1024.0, cases=nc):
    """The same solve as two requests, the first of `first_piece` pivots.  A request that meets the hand-over
    answers MI_RUNNING with exactly j pivots applied -- short of what was asked --, and the next request goes on
    from there; nothing else may cut a request short, and no solve is cut twice.  With the piece boundary before
    or behind step j some request crosses the event and MUST be cut; with the boundary AT step j the first
    request ends there on its cap and the second one may be cut before its first pivot.  -> what ran."""
    ref, j, cap = cases.reference(case), case.j, cases.cap_of(case)
    t = _tableau(case, cases)
    is_max = int(case.kind == "max")
    k = ctypes.c_int64(0)
    done = short = calls = 0
    rc = lp.capi.MI_RUNNING
    for goal in (first_piece, cap):
        while rc == lp.capi.MI_RUNNING:
            lp.capi.check(L.mi355x_tab_solve_async(t._h, is_max, factor, goal - done, 1 if calls == 0 else 0), "solve_async")
            rc = L.mi355x_tab_sync(t._h, ctypes.byref(k))
            calls += 1
            done = k.value
            if done == min(goal, ref.pivots):
                break
            assert _hands_over(case) and (rc, done) == (lp.capi.MI_RUNNING, j) and short == 0, (rc, done, j, goal, short)
            short += 1
    if rc == lp.capi.MI_RUNNING and ref.status != oracle.MAX_PIVOTS:     # the LP's last pivot was a request's last: one more look
        lp.capi.check(L.mi355x_tab_solve_async(t._h, is_max, factor, 1, 0), "solve_async")
        rc = L.mi355x_tab_sync(t._h, ctypes.byref(k))
    assert k.value == ref.pivots and rc == (lp.capi.MI_RUNNING if ref.status == oracle.MAX_PIVOTS else ref.status), (rc, k.value)
    if _hands_over(case):
        assert short == 1 or (short == 0 and first_piece == j), (short, first_piece, j)
    else:
        assert short == 0
    path = _path(L, t._h)
    t._touch()
    _same(t, ref, "requests %d + rest" % first_piece)
    return path


def _blocked_then_dense(case, path, ref, blocked, others):
    """C, Q: the blocked path up to step j, per-pivot launches from there.  Z0, ZY, S0: the blocked path alone."""
    c = path.counts
    assert c[blocked] > 0 and all(c[o] == 0 for o in others), c
    if _hands_over(case):
        assert c[PER_PIVOT] >= ref.pivots - case.j > 0, (c, ref.pivots, case.j)
    else:
        assert c[PER_PIVOT] == 0, c


def _pieces(case):
    """First-request sizes: the piece boundary one pivot before the event, at it, one pivot after it."""
    return [b for b in (case.j - 1, case.j, case.j + 1) if 0 < b < nc.cap_of(case)]


# =========================================================================== 1. per-pivot kernels (block 1)
@pytest.mark.parametrize("compact", [1, 0], ids=["compact", "dense"])
@pytest.mark.parametrize("select_mode", [1, 2], ids=["one-workgroup-select", "split-select"])
@pytest.mark.parametrize("case", nc.PER_PIVOT, ids=nc.case_id)
def test_per_pivot_kernels(knobs, case, select_mode, compact):
    """k_select (block_gather_ratio) and k_select_gather / k_select_scale (poison bits, block_ratio_from_snapshot):
    the NaN row and the first eligible row sit in different workgroups of the split gather, in both orders."""
    L = knobs
    L.mi355x_tune_set_block(1)
    L.mi355x_tune_set_select_mode(select_mode)
    L.mi355x_tune_set_compact(compact)
    path, ref = _capped_run(L, case)
    c = path.counts
    assert c[PER_PIVOT] >= ref.pivots and c[LA_PERSISTENT] == c[LA_TWO_LAUNCH] == c[RESIDENT] == 0, c
    assert (c[SELECT_SPLIT] > 0) == (select_mode == 2), c


# =========================================================================== 2. two-launch look-ahead
@pytest.mark.parametrize("case,block", nc.TWO_LAUNCH, ids=["%s-b%d" % (nc.case_id(c), b) for c, b in nc.TWO_LAUNCH])
def test_two_launch_lookahead(knobs, case, block):
    """k_la_gather / k_la_scale behind pending pivots, 16 and 24 per sweep: one capped solve, and two requests
    whose boundary falls at the event."""
    L = knobs
    L.mi355x_tune_set_lookahead_mode(1)
    L.mi355x_tune_set_select_mode(2)
    L.mi355x_tune_set_block(block)
    path, ref = _capped_run(L, case)
    assert path.block == block or _hands_over(case)
    _blocked_then_dense(case, path, ref, LA_TWO_LAUNCH, (LA_PERSISTENT, RESIDENT))
    path = _request_sequence(L, case, max(case.j, 1))
    _blocked_then_dense(case, path, ref, LA_TWO_LAUNCH, (LA_PERSISTENT, RESIDENT))


# =========================================================================== 3. persistent look-ahead
@pytest.mark.parametrize("case,wg,block", nc.PERSISTENT, ids=["%s-wg%d-b%d" % (nc.case_id(c), w, b) for c, w, b in nc.PERSISTENT])
def test_persistent_lookahead(knobs, case, wg, block):
    """k_la_block at 3, 17 and 33 workgroups (by rows and by column pairs; from 33 on one exchange record per
    workgroup): one capped solve, then two requests with the boundary one pivot before the event, at it and one
    pivot after it.  The request that meets kNeedDense answers MI_RUNNING with j pivots, the next one goes on."""
    L = knobs
    assert _la_workgroups(case.n, case.m) == wg
    L.mi355x_tune_set_lookahead_mode(2)
    L.mi355x_tune_set_block(block)
    path, ref = _capped_run(L, case)
    _blocked_then_dense(case, path, ref, LA_PERSISTENT, (LA_TWO_LAUNCH, RESIDENT))
    assert path.lost == 0 and path.workgroups == wg
    pieces = _pieces(case) if case.m < 8000 else [case.j]   # (the 555 MB tableau: one request sequence)
    for piece in pieces:
        path = _request_sequence(L, case, piece)
        _blocked_then_dense(case, path, ref, LA_PERSISTENT, (LA_TWO_LAUNCH, RESIDENT))
        assert path.lost == 0 and path.workgroups == wg


# =========================================================================== 4. wide sweeps
WIDE_FORMS = {"24-ring": (24, 1), "28-ring": (28, 1), "24-registers": (24, 0)}


@pytest.mark.parametrize("form", sorted(WIDE_FORMS))
@pytest.mark.parametrize("case", nc.WIDE, ids=nc.case_id)
def test_wide_sweeps(knobs, case, form):
    """k_sweepw_ring / k_sweepw apply 24 / 28 pending pivot rows in one pass: ZY's column of infinities and NaNs goes
    through the chained rank-1 updates of a whole block; C stops the second block after three steps."""
    L = knobs
    block, ring = WIDE_FORMS[form]
    try:
        assert L.mi355x_tune_set_block(block) == block
        L.mi355x_tune_set_sweepw_ring(ring)
        L.mi355x_tune_set_select_mode(2)                   # small shapes too: the blocked path
        path, ref = _capped_run(L, case)
        c = path.counts
        assert c[WIDE_SWEEP] > 0 and c[RESIDENT] == 0, c
        assert (c[PER_PIVOT] >= ref.pivots - case.j) if _hands_over(case) else (c[PER_PIVOT] == 0 and path.block == block), c
    finally:
        L.mi355x_tune_set_sweepw_ring(1)


# =========================================================================== 5. resident solve
@pytest.mark.parametrize("case,lds", nc.RESIDENT, ids=["%s-lds%d" % (nc.case_id(c), s) for c, s in nc.RESIDENT])
def test_resident_solve(knobs, case, lds):
    """k_resident's own copy of the rules (pnan0, bit 31 of the index word), the tableau in registers over several
    64-column strips; lds 1: the event's column among the last 24 of its strip, which live in LDS."""
    L = knobs
    L.mi355x_tune_set_resident(2)
    assert L.mi355x_tune_set_resident_lds(lds) == lds
    path, ref = _capped_run(L, case, prepare=True)
    _blocked_then_dense(case, path, ref, RESIDENT, (LA_PERSISTENT, LA_TWO_LAUNCH))
    path = _request_sequence(L, case, max(case.j, 1))
    _blocked_then_dense(case, path, ref, RESIDENT, (LA_PERSISTENT, LA_TWO_LAUNCH))


# =========================================================================== 6. batches
def _check_batch(batch, st, npv, refs, what):
    for k, ref in enumerate(refs):
        G, gb = batch.download(k)
        assert (int(st[k]), int(npv[k])) == (ref.status, ref.pivots), (what, k, int(st[k]), int(npv[k]), ref.status, ref.pivots)
        assert np.array_equal(gb, ref.basis), (what, k)
        _same_bits(G, ref.M, (what, k))


def _batch_case(L, shape, kind, path, factor=1024.0, cases=nc):
    Ms, Bs, _ = cases.batch(*shape, kind)
    for cap in (cases.BATCH_CAP, 4):                       # to the members' ends; a cap between the members' events
        batch = lp.TableauBatch.from_arrays(Ms, Bs)
        st, npv = batch.solve(is_max=(kind == "max"), fp_tolerance=factor, max_pivots=cap)
        c = _batch_counts(L, batch)
        assert c[path] > 0, (cap, c)
        _check_batch(batch, st, npv, cases.batch_reference(*shape, kind, cap), "cap %d" % cap)


@pytest.mark.parametrize("kind", ["max", "min"])
@pytest.mark.parametrize("mode,batch_block,compact,path", BATCH_PATHS,
                         ids=["mode%d-bb%d-%s" % (a, b, "compact" if c else "dense") for a, b, c, _ in BATCH_PATHS])
@pytest.mark.parametrize("shape", nc.BATCH_SHAPES[:3], ids=["%dx%d" % s for s in nc.BATCH_SHAPES[:3]])
def test_batches(knobs, shape, mode, batch_block, compact, path, kind):
    """Six members: C at step 3, Q in row 0 at step 5, Q in the last row at step 2, Z0 at step 4, two untouched
    ones.  A member's hand-over takes the whole batch to the dense tableaux while the others are in the middle
    of their solves: every member must end where the oracle ends on it alone."""
    L = knobs
    L.mi355x_tune_set_batch_mode(mode)
    L.mi355x_tune_set_batch_block(batch_block)
    L.mi355x_tune_set_compact(compact)
    if compact and (mode == 3 or batch_block > 1):
        assert _batch_block_fits(shape[0], shape[1], batch_block or 16)
    _batch_case(L, shape, kind, path)


@pytest.mark.parametrize("kind", ["max", "min"])
def test_resident_batch_with_default_knobs(knobs, kind):
    """512 x 256 members with every knob at its default: the batch starts RESIDENT (k_resident, every LP on chip)."""
    _batch_case(knobs, nc.BATCH_SHAPES[3], kind, B_RESIDENT)


# =========================================================================== 7. column partitions
EXCHANGES = [(0, 0), (2, 0), (2, 1), (3, 0)]
# (shards, case, exchange, shard_la_block off, block, shard_la_split); Q with the one-workgroup and the split step
COLPART = [(shards, case, ex, lab, 16 if (i + k) % 2 else 24, split)
           for i, (shards, case) in enumerate(nc.COLPART) for k, (ex, lab) in enumerate(EXCHANGES)
           for split in ((1, 2) if case.ev == "Q" else (0,))]


@pytest.mark.parametrize("shards,case,exchange,la_block_off,block,split", COLPART,
                         ids=["s%d-%s-x%d%s-b%d%s" % (s, nc.case_id(c), x, "-steps" if o else "", b, ("", "-one-workgroup-step", "-split-step")[p])
                              for s, c, x, o, b, p in COLPART])
def test_column_partitions(knobs, shards, case, exchange, la_block_off, block, split):
    """mi355x_colpart_*: C on compact shards moves the tableau to DENSE shards in place and ends as the oracle
    does; Z0 in global column 0 and ZY in the first local column of a later shard behave as on one tableau.
    Q meets a documented limit (mi355x_simplex.h, MI_NONFINITE; k_shard_la_ratio and k_shard_la_block say so where
    they test the quotient): the split look-ahead step and the persistent block launch do not reproduce the
    first-eligible-row rule and end the solve with MI_NONFINITE -- the pivots reported are a prefix of the
    oracle's trace, at most j of them, and the download is the oracle's tableau after that many pivots.  The
    one-workgroup step (k_shard_la_prepare) takes its ratio test from block_gather_ratio, which does reproduce
    the rule: there the solve goes on and must end as the oracle does."""
    L = knobs
    cp = importlib.import_module("linear-programming_amd.colpart")
    p, ref, j = nc.planted(case), nc.reference(case), case.j
    is_max = case.kind == "max"
    L.mi355x_tune_set_block(block)
    L.mi355x_tune_set_colpart_exchange(exchange)
    L.mi355x_tune_set_shard_la_block(la_block_off)
    try:
        L.mi355x_tune_set_shard_la_split(split)
        tab = cp.NativeColumnPartition.from_arrays(p.M, p.basis, shards)
    except BaseException:
        L.mi355x_tune_set_shard_la_split(0)
        raise
    try:
        assert tab.info()["n_shards"] == shards and tab.block_size() == block and tab.is_compact() == (not case.dense)
        st, k = tab.solve(is_max=is_max, max_pivots=nc.CAP)
        if case.ev == "Q" and (split == 2 or (exchange == 2 and not la_block_off)):
            assert st == lp.capi.MI_NONFINITE and k <= j, (st, k, j)
            ref = nc.reference(case, k) if k else nc.Reference(oracle.MAX_PIVOTS, 0, ref.trace[:0], p.M, p.basis)
        else:
            assert (st, k) == (ref.status, ref.pivots), (st, k, ref.status, ref.pivots)
        if case.ev != "Q":
            assert tab.is_compact() == (not case.dense and case.ev != "C")           # C: dense shards from step j on
        tr = tab.trace(ref.pivots) if ref.pivots else ref.trace
        assert tr.shape == ref.trace.shape and np.array_equal(tr, ref.trace), (tr[:3].tolist(), ref.trace[:3].tolist())
        G, gb, last_row, last_col = tab.download()
        assert np.array_equal(gb, ref.basis)
        _same_bits(G, ref.M, "download")
        _same_bits(last_row[None, :], ref.M[-1:], "last row")
        _same_bits(last_col[None, :], ref.M[:, -1].copy()[None, :], "last column")
        stats = tab.la_stats()
        if exchange == 2 and not la_block_off and (j > 0 or case.ev not in ("C", "Q")):
            assert stats["blocks"] > 0 and stats["losses"] == 0, stats
        elif exchange != 2 or la_block_off:
            assert stats["blocks"] == 0, stats
    finally:
        L.mi355x_tune_set_shard_la_split(0)
        tab.close()
