"""The thresholds of the two scans, met exactly in the MIDDLE of a solve, on every double-precision path.

The reference decides by strict comparisons (find-entering-column / find-pivoting-row, src/simplex.lisp:370-372,
:386-387): a row is eligible only if 0 + (f/2) eps < a, a column enters only if key < 0 - (f/8) eps.  The kernels
write the row test out by hand in eleven places (block_gather_ratio, k_select_gather, k_la_gather, k_la_block,
k_resident, k_batch_solve, k_batch_block, k_shard_p2p_step, k_shard_la_ratio, k_shard_la_block,
block_ratio_from_snapshot) and call price_says_optimal from nine, on winners that came through different reductions
and exchange records; every launch path computes its own two thresholds from the call's factor.  Uniform floats never
come within 1e-2 of either threshold, so elsewhere `<=` for `<`, or a threshold one ulp off, passes.

The tableaux of tests/threshold_cases.py hold an entry bitwise AT a threshold or one ulp BEYOND it, at step j of the
oracle's trace -- in the middle of a block of pending pivots, at its last step, at the first step of the next
block -- at 3, 17 and 33 look-ahead workgroups, in several resident strips, behind the wide sweeps, in batch members
larger than a wave and on column shards, with factors 1024, 16, 2**20 and 1000 (whose products with epsilon round);
tests/test_threshold_cases_host.py proves on the oracle what every case claims:
  T   M[R, X] = thr / nextafter(thr, inf) in an isolated row whose quotient would be 2**-10, X entering at step j:
      `at` R is not eligible (a `<=` kernel pivots on it), `beyond` it is the pivot row (a threshold one ulp higher
      misses it), a pivot element of about 5.7e-14 after which the solve goes on with finite numbers;
  P   a zero column whose key is -ptol / its predecessor, the strict minimum at the LP's last step k_end: OPTIMAL
      against UNBOUNDED after the same pivots, with k_end on a block's first step, inside it and on its last.

Every comparison is with oracle.solve on the same arrays with the same factor: status, pivot count, the whole
trace, the basis, the final tableau as int64 bits (batches: status, count, bits, basis).  Every case asserts that
the path it names is the one that ran, and on the blocked paths that no per-pivot launch happened: a finite
threshold event is no reason for the dense hand-over.

Not reached: block_ratio_from_snapshot (kernels_common.inc) runs only on k_select_scale's poison path, which takes
a non-finite entry in the gathered column or a NaN quotient; no finite tableau gets there, so that one copy of the
row test is pinned by tests/test_gpu_nonfinite.py alone."""
import importlib

import numpy as np
import pytest

from tests import threshold_cases as tc
from tests.test_gpu_nonfinite import (EXCHANGES, WIDE_SWEEP, _batch_case, _blocked_then_dense, _capped_run, _request_sequence,
                                      _same_bits)
from tests.test_gpu_ties import (BATCH_PATHS, B_RESIDENT, LA_PERSISTENT, LA_TWO_LAUNCH, PER_PIVOT, RESIDENT, SELECT_SPLIT,
                                 _batch_block_fits, _la_workgroups, knobs)   # noqa: F401 (knobs: fixture)

pytestmark = pytest.mark.gpu


def _run(L, case, **kw):
    return _capped_run(L, case, factor=case.f, cases=tc, **kw)


def _requests(L, case, blocked, others):
    """Two requests with the boundary AT step j (the event's step is the first of a freshly requested block) and one
    pivot behind it (it is the last step of a block cut short by the request)."""
    ref = tc.reference(case)
    for piece in (case.j, case.j + 1):
        if 0 < piece < tc.cap_of(case):
            path = _request_sequence(L, case, piece, factor=case.f, cases=tc)
            _blocked_then_dense(case, path, ref, blocked, others)
            yield path


# =========================================================================== 1. per-pivot kernels (block 1)
@pytest.mark.parametrize("compact", [1, 0], ids=["compact", "dense"])
@pytest.mark.parametrize("select_mode", [1, 2], ids=["one-workgroup-select", "split-select"])
@pytest.mark.parametrize("case", tc.PER_PIVOT, ids=tc.case_id)
def test_per_pivot_kernels(knobs, case, select_mode, compact):
    """k_select (block_gather_ratio) and k_select_gather / k_select_scale: R and the step's winner sit in different
    workgroups of the split gather."""
    L = knobs
    L.mi355x_tune_set_block(1)
    L.mi355x_tune_set_select_mode(select_mode)
    L.mi355x_tune_set_compact(compact)
    path, ref = _run(L, case)
    c = path.counts
    assert c[PER_PIVOT] >= ref.pivots and c[LA_PERSISTENT] == c[LA_TWO_LAUNCH] == c[RESIDENT] == 0, c
    assert (c[SELECT_SPLIT] > 0) == (select_mode == 2), c


# =========================================================================== 2. two-launch look-ahead
@pytest.mark.parametrize("case,block,requests", tc.TWO_LAUNCH, ids=["%s-b%d" % (tc.case_id(c), b) for c, b, _ in tc.TWO_LAUNCH])
def test_two_launch_lookahead(knobs, case, block, requests):
    """k_la_gather / k_la_scale behind pending pivots, 16 and 24 per sweep."""
    L = knobs
    L.mi355x_tune_set_lookahead_mode(1)
    L.mi355x_tune_set_select_mode(2)
    L.mi355x_tune_set_block(block)
    path, ref = _run(L, case)
    assert path.block == block
    _blocked_then_dense(case, path, ref, LA_TWO_LAUNCH, (LA_PERSISTENT, RESIDENT))
    if requests:
        assert len(list(_requests(L, case, LA_TWO_LAUNCH, (LA_PERSISTENT, RESIDENT)))) == 2


# =========================================================================== 3. persistent look-ahead
@pytest.mark.parametrize("case,wg,block,requests", tc.PERSISTENT,
                         ids=["%s-wg%d-b%d" % (tc.case_id(c), w, b) for c, w, b, _ in tc.PERSISTENT])
def test_persistent_lookahead(knobs, case, wg, block, requests):
    """k_la_block at 3, 17 and 33 workgroups (by rows and by column pairs; from 33 on one exchange record per
    workgroup): its own copy of the row test, and price_says_optimal on the winner of the exchange."""
    L = knobs
    assert _la_workgroups(case.n, case.m) == wg
    L.mi355x_tune_set_lookahead_mode(2)
    L.mi355x_tune_set_block(block)
    path, ref = _run(L, case)
    _blocked_then_dense(case, path, ref, LA_PERSISTENT, (LA_TWO_LAUNCH, RESIDENT))
    assert path.block == block and path.lost == 0 and path.workgroups == wg
    if requests:
        paths = list(_requests(L, case, LA_PERSISTENT, (LA_TWO_LAUNCH, RESIDENT)))
        assert len(paths) == 2 and all(p.lost == 0 and p.workgroups == wg for p in paths)


# =========================================================================== 4. wide sweeps
WIDE_FORMS = {"24-ring": (24, 1), "28-ring": (28, 1)}
WIDE = [(case, "24-ring") for case in tc.WIDE] + [(tc.WIDE[1], "28-ring")]


@pytest.mark.parametrize("case,form", WIDE, ids=["%s-%s" % (tc.case_id(c), f) for c, f in WIDE])
def test_wide_sweeps(knobs, case, form):
    """k_sweepw_ring applies 24 / 28 pending pivot rows in one pass; the event falls three steps into the second
    block of 24, P's also on the last step of a block of 28."""
    L = knobs
    block, ring = WIDE_FORMS[form]
    try:
        assert L.mi355x_tune_set_block(block) == block
        L.mi355x_tune_set_sweepw_ring(ring)
        L.mi355x_tune_set_select_mode(2)                   # small shapes too: the blocked path
        path, ref = _run(L, case)
        c = path.counts
        assert c[WIDE_SWEEP] > 0 and c[RESIDENT] == 0 and c[PER_PIVOT] == 0 and path.block == block, c
    finally:
        L.mi355x_tune_set_sweepw_ring(1)


# =========================================================================== 5. resident solve
@pytest.mark.parametrize("case,lds", tc.RESIDENT, ids=["%s-lds%d" % (tc.case_id(c), s) for c, s in tc.RESIDENT])
def test_resident_solve(knobs, case, lds):
    """k_resident's own copy of the row test, the tableau in registers over several 64-column strips."""
    L = knobs
    L.mi355x_tune_set_resident(2)
    assert L.mi355x_tune_set_resident_lds(lds) == lds
    path, ref = _run(L, case, prepare=True)
    _blocked_then_dense(case, path, ref, RESIDENT, (LA_PERSISTENT, LA_TWO_LAUNCH))
    if lds == 0:
        assert len(list(_requests(L, case, RESIDENT, (LA_PERSISTENT, LA_TWO_LAUNCH)))) == 2


# =========================================================================== 6. batches
@pytest.mark.parametrize("mode,batch_block,compact,path", BATCH_PATHS,
                         ids=["mode%d-bb%d-%s" % (a, b, "compact" if c else "dense") for a, b, c, _ in BATCH_PATHS])
@pytest.mark.parametrize("shape", tc.BATCH_SHAPES[:3], ids=["%dx%d" % s for s in tc.BATCH_SHAPES[:3]])
def test_batches(knobs, shape, mode, batch_block, compact, path):
    """Eight members with the call's one factor: T-at, T-beyond in row 0 and in the last row, P-at, P-beyond, two
    untouched ones and T-at in row 0, their events at different steps (k_batch_solve, k_batch_block, the lockstep
    launches and the split form); to the members' ends and with a cap between the events."""
    L = knobs
    L.mi355x_tune_set_batch_mode(mode)
    L.mi355x_tune_set_batch_block(batch_block)
    L.mi355x_tune_set_compact(compact)
    if compact and (mode == 3 or batch_block > 1):
        assert _batch_block_fits(shape[0], shape[1], batch_block or 16)
    kind, f = tc.BATCH_KIND_FACTOR[shape]
    _batch_case(L, shape, kind, path, factor=f, cases=tc)


def test_resident_batch_with_default_knobs(knobs):
    """512 x 256 members with every knob at its default: the batch starts RESIDENT (k_resident, every LP on chip)."""
    shape = tc.BATCH_SHAPES[3]
    kind, f = tc.BATCH_KIND_FACTOR[shape]
    _batch_case(knobs, shape, kind, B_RESIDENT, factor=f, cases=tc)


# =========================================================================== 7. column partitions
# (shards, case, exchange, shard_la_block off, block, shard_la_split); T with the one-workgroup and the split step
COLPART = [(shards, case, ex, lab, 16 if (i + k) % 2 else 24, split)
           for i, (shards, case) in enumerate(tc.COLPART) for k, (ex, lab) in enumerate(EXCHANGES)
           for split in ((1, 2) if case.ev == "T" else (0,))]


@pytest.mark.parametrize("shards,case,exchange,la_block_off,block,split", COLPART,
                         ids=["s%d-%s-x%d%s-b%d%s" % (s, tc.case_id(c), x, "-steps" if o else "", b, ("", "-one-workgroup-step", "-split-step")[p])
                              for s, c, x, o, b, p in COLPART])
def test_column_partitions(knobs, shards, case, exchange, la_block_off, block, split):
    """mi355x_colpart_*: k_shard_prepare / k_shard_la_prepare (block_gather_ratio), k_shard_p2p_step, k_shard_la_ratio
    (the split look-ahead step) and k_shard_la_block each test the row themselves; T's entering column belongs to
    the last shard.  P's column is the first one of a later shard: every other shard's local winner says optimal,
    the exchanged winner decides -- k_shard_la_block asks price_says_optimal about both.  (k_shard_p2p_step runs where
    a shard has its stream to itself: on one GPU that is the partition of ONE shard, exchange 2, split step.)"""
    L = knobs
    cp = importlib.import_module("linear-programming_amd.colpart")
    p, ref = tc.planted(case), tc.reference(case)
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
        st, k = tab.solve(is_max=(case.kind == "max"), fp_tolerance=case.f, max_pivots=tc.CAP)
        assert (st, k) == (ref.status, ref.pivots), (st, k, ref.status, ref.pivots)
        assert tab.is_compact() == (not case.dense)        # no move to dense shards
        tr = tab.trace(ref.pivots)
        bad = np.where((tr != ref.trace).any(axis=1))[0] if tr.shape == ref.trace.shape else [-1]
        assert not len(bad), "pivot trace differs from the oracle's, first at %s: got %s, oracle %s" % (
            bad[:3], tr[bad[:3]].tolist(), ref.trace[bad[:3]].tolist())
        G, gb, last_row, last_col = tab.download()
        assert np.array_equal(gb, ref.basis)
        _same_bits(G, ref.M, "download")
        _same_bits(last_row[None, :], ref.M[-1:], "last row")
        _same_bits(last_col[None, :], ref.M[:, -1].copy()[None, :], "last column")
        stats = tab.la_stats()
        # (a lone shard asked for the all-reduce form exchanges with nobody: it takes exchange mode 2's self-push form)
        if (exchange == 2 or (exchange == 0 and shards == 1)) and not la_block_off:
            assert stats["blocks"] > 0 and stats["losses"] == 0, stats
        else:
            assert stats["blocks"] == 0, stats
    finally:
        L.mi355x_tune_set_shard_la_split(0)
        tab.close()
