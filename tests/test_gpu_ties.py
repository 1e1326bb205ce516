"""Exact ties in pricing and in the ratio test, on every double-precision solve path: the lowest index wins
(find-entering-column / find-pivoting-row, src/simplex.lisp:362-389: `finding ... minimizing`, strict
comparison, first index) -- across lanes, waves, workgroups, exchange records, column strips, shards and the
members of a batch; in the compact representation the lowest LOGICAL column, whatever slot it sits in.

Uniform random floats never tie, so everywhere else in the suite wave_argmin (kernels_la_common.inc) takes
its unique-minimum fast path and the tie branches of k_la_block, k_shard_la_block, k_batch_block and
k_resident never run.  The tableaux of tests/tie_cases.py have duplicated rows and columns: a pair keeps
bit-identical keys and quotients until one partner is chosen, so dozens of steps per solve are exact ties
at a NON-ZERO quotient between indices a chosen distance apart (tests/test_tie_cases_host.py counts them
on the oracle).  A kernel that prefers the higher index, the later wave, record or shard takes the partner:
another trace, another tableau.  Twins keep their upload slots, where slot order and logical order agree; so
every compact tableau and every batch member with duplicates also carries the gadgets of tie_cases.py (6, 4
on the 40-row shapes, 2 per member), each ending in a tied pricing step whose lower LOGICAL column sits in one
of the LAST slots and its partner in one of the first -- a reduction that prefers the lower slot takes the
partner there.

Every comparison is with oracle.solve on the same arrays: status, pivot count, the whole pivot trace, the
final tableau as int64 bits, the basis (a batch hands out no trace: status, count, bits, basis) -- for a
run capped at 80 pivots (or the LP's end) and, on the blocked paths, for a sequence of requests that cuts
a block short.  Every case asserts that the path it names is the one that ran."""
import collections
import ctypes
import importlib

import numpy as np
import pytest

import oracle
from tests import tie_cases as tc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
PER_PIVOT, LA_PERSISTENT, LA_TWO_LAUNCH, RESIDENT, SELECT_SPLIT = 0, 1, 2, 6, 7       # mi355x_tab_path_counts
B_RESIDENT, B_SPLIT, B_PER_LP, B_LOCKSTEP = 0, 1, 2, 3                                # mi355x_batch_path_counts
KINDS = ["max", "min"]


@pytest.fixture
def knobs():
    L = lp.capi.lib()
    yield L
    L.mi355x_tune_set_select_mode(0)
    L.mi355x_tune_set_compact(1)
    L.mi355x_tune_set_block(0)
    L.mi355x_tune_set_lookahead_mode(0)
    L.mi355x_tune_set_resident(0)
    L.mi355x_tune_set_resident_lds(0)
    L.mi355x_tune_set_batch_mode(0)
    L.mi355x_tune_set_batch_block(0)
    L.mi355x_tune_set_colpart_exchange(0)
    L.mi355x_tune_set_shard_la_block(0)


Path = collections.namedtuple("Path", "counts block lost workgroups resident")


def _path(L, h):
    """What ran on the handle, read BEFORE the download (which takes the handle back to the dense tableau)."""
    out = (ctypes.c_int64 * 8)()
    lp.capi.check(L.mi355x_tab_path_counts(h, out), "path_counts")
    return Path(list(out), L.mi355x_tab_block_size(h), L.mi355x_tab_la_lost(h), L.mi355x_tab_la_workgroups(h),
                L.mi355x_tab_resident(h))


def _la_workgroups(n, m):
    return (max(m, (n + 1) // 2) + 255) // 256             # as tests/test_gpu_la_launch_count.py: a thread per row and per column pair


def _same(t, ref, what):
    """Trace, bits and basis of handle t against the shared reference (never modified)."""
    tr = t.pivot_trace()[:ref.pivots]
    if not np.array_equal(tr, ref.trace):
        k = min(len(tr), len(ref.trace))
        bad = np.where((tr[:k] != ref.trace[:k]).any(axis=1))[0]
        raise AssertionError("%s: pivot trace (%d pivots) differs from the oracle's (%d), first at %s: got %s, oracle %s"
                             % (what, len(tr), len(ref.trace), bad[:3], tr[bad[:3]].tolist(), ref.trace[bad[:3]].tolist()))
    assert np.array_equal(t.basis_columns, ref.basis), what
    G = t.matrix
    for r0 in range(0, G.shape[0], 2048):
        assert np.array_equal(G[r0:r0 + 2048].view(np.int64), ref.M[r0:r0 + 2048].view(np.int64)), (what, r0)


def _tableau(case, kind):
    n, m = case[0], case[1]
    M0, b0 = tc.single(*case, kind)
    return lp.Tableau(None, lp.Problem(type=kind), M0, b0, n + m, m, {})


def _capped_run(L, case, kind, prepare=False):
    """One solve capped at tc.CAP on a fresh handle, compared with the shared reference -> (what ran, reference)."""
    ref = tc.single_reference(*case, kind)
    t = _tableau(case, kind)
    k = ctypes.c_int64(0)
    if prepare:                                            # -> the compact representation, nothing solved
        lp.capi.check(L.mi355x_tab_solve_async(t._h, int(kind == "max"), 1024.0, 0, 1), "prepare")
        L.mi355x_tab_sync(t._h, ctypes.byref(k))
        assert L.mi355x_tab_resident(t._h) == 1
    rc = L.mi355x_tab_solve(t._h, int(kind == "max"), 1024.0, tc.CAP, ctypes.byref(k))
    path = _path(L, t._h)
    t._touch()
    assert (rc, k.value) == (ref.status, ref.pivots), (rc, k.value, ref.status, ref.pivots)
    _same(t, ref, "capped run")
    return path, ref


def _request_sequence(L, case, kind, block):
    """5, block, 2 * block + 3 and what is left of tc.CAP pivots (24 after blocks of 16, nothing after blocks
    of 24) as separate requests on a fresh handle: a short block, a full one, two full ones and a short one --
    the same 80 pivots (or the LP's end) -> what ran."""
    ref = tc.single_reference(*case, kind)
    t = _tableau(case, kind)
    requests = [5, block, 2 * block + 3]
    requests += [tc.CAP - sum(requests)] if sum(requests) < tc.CAP else []
    assert sum(requests) == tc.CAP
    k = ctypes.c_int64(0)
    done = 0
    for i, q in enumerate(requests):
        lp.capi.check(L.mi355x_tab_solve_async(t._h, int(kind == "max"), 1024.0, q, 1 if i == 0 else 0), "solve_async")
        rc = L.mi355x_tab_sync(t._h, ctypes.byref(k))
        done += q
        assert k.value == min(done, ref.pivots), (i, k.value, done, ref.pivots)
        if done < ref.pivots:
            assert rc == lp.capi.MI_RUNNING, (i, rc)
    assert rc == (lp.capi.MI_RUNNING if ref.status == oracle.MAX_PIVOTS else ref.status), rc
    path = _path(L, t._h)
    t._touch()
    _same(t, ref, "requests %s" % requests)
    return path


def _id(case):
    return "%dx%d-r%d-c%d" % case


# =========================================================================== 1. per-pivot kernels (block 1)
PER_PIVOT_CASES = [(1100, 600, 300, 550), (1100, 600, 64, 64), (1100, 600, 1, 1)]   # partners workgroups / waves / lanes apart


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("compact", [1, 0], ids=["compact", "dense"])
@pytest.mark.parametrize("select_mode", [1, 2], ids=["one-workgroup-select", "split-select"])
@pytest.mark.parametrize("case", PER_PIVOT_CASES, ids=_id)
def test_per_pivot_kernels(knobs, case, select_mode, compact, kind):
    """k_select (one workgroup of 1024 threads) and k_select_gather / k_select_scale, one pivot per launch
    pair; compact: the columns change slots with every pivot, the tie goes to the lowest logical column."""
    L = knobs
    L.mi355x_tune_set_block(1)
    L.mi355x_tune_set_select_mode(select_mode)
    L.mi355x_tune_set_compact(compact)
    path, ref = _capped_run(L, case, kind)
    c = path.counts
    assert c[PER_PIVOT] >= ref.pivots and c[LA_PERSISTENT] == c[LA_TWO_LAUNCH] == c[RESIDENT] == 0, c
    assert (c[SELECT_SPLIT] > 0) == (select_mode == 2), c


# =========================================================================== 2. two-launch look-ahead
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("block", [16, 24])
@pytest.mark.parametrize("case", [(1100, 600, 300, 550), (2000, 900, 450, 1000)], ids=_id)
def test_two_launch_lookahead(knobs, case, block, kind):
    """k_la_gather / k_la_scale per step behind pending pivots (look-ahead mode 1), 16 and 24 per sweep.
    (Select mode 2: below 1024 rows / 4096 stored columns the two-launch form is not chosen by size.)"""
    L = knobs
    L.mi355x_tune_set_lookahead_mode(1)
    L.mi355x_tune_set_select_mode(2)
    L.mi355x_tune_set_block(block)
    for path in (_capped_run(L, case, kind)[0], _request_sequence(L, case, kind, block)):
        c = path.counts
        assert path.block == block
        assert c[LA_TWO_LAUNCH] > 0 and c[LA_PERSISTENT] == c[RESIDENT] == c[PER_PIVOT] == 0, c


# =========================================================================== 3. persistent look-ahead
# (case, workgroups, blocks).  Up to 16 workgroups' wave records fit one poll (64), 17 need more than 64 wave
# records, from 33 on a workgroup publishes ONE record (k_la_block<., WGR = true>); by rows and by column pairs.
PERSISTENT_CASES = [
    ((1100, 600, 300, 550), 3, (24, 16)),                  # partners in different workgroups (rows) / the last and the first (pairs)
    ((1100, 600, 64, 64), 3, (24,)),                       # ... in neighbouring waves (rows), 32 lanes apart (pairs)
    ((1100, 600, 1, 1), 3, (24,)),                         # ... in neighbouring lanes (rows), in ONE thread's pair (columns)
    ((64, 4200, 2100, 32), 17, (24, 16)),                  # by rows, > 64 wave records
    ((8300, 40, 20, 4150), 17, (24, 16)),                  # by column pairs, > 64 wave records
    ((64, 4200, 256, 32), 17, (24,)),                      # partners in ADJACENT workgroups, by rows
    ((8300, 40, 20, 512), 17, (24,)),                      # ... by column pairs
    ((64, 8300, 4150, 32), 33, (24,)),                     # one record per workgroup, by rows
    ((16500, 40, 20, 8250), 33, (24,)),                    # one record per workgroup, by column pairs
]
PERSISTENT = [(case, wg, block) for case, wg, blocks in PERSISTENT_CASES for block in blocks]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,wg,block", PERSISTENT, ids=["%s-wg%d-b%d" % (_id(c), w, b) for c, w, b in PERSISTENT])
def test_persistent_lookahead(knobs, case, wg, block, kind):
    """k_la_block (look-ahead mode 2): the wave winners meet through exchange records -- every wave's up to
    32 workgroups, one per workgroup above; none lost, so no step fell back to the two-launch form."""
    L = knobs
    assert _la_workgroups(case[0], case[1]) == wg
    L.mi355x_tune_set_lookahead_mode(2)
    L.mi355x_tune_set_block(block)
    for path in (_capped_run(L, case, kind)[0], _request_sequence(L, case, kind, block)):
        c = path.counts
        assert path.block == block
        assert c[LA_PERSISTENT] > 0 and c[LA_TWO_LAUNCH] == c[RESIDENT] == c[PER_PIVOT] == 0, c
        assert path.lost == 0 and path.workgroups == wg


# =========================================================================== 4. resident solve
RESIDENT_CASES = [((300, 257, 128, 128), 0), ((1024, 512, 256, 512), 0), ((2048, 200, 100, 1024), 0),
                  ((2048, 200, 100, 1024), 1), ((2048, 200, 100, 1), 0), ((2048, 200, 100, 1), 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,lds", RESIDENT_CASES, ids=["%s-lds%d" % (_id(c), s) for c, s in RESIDENT_CASES])
def test_resident_solve(knobs, case, lds, kind):
    """k_resident: the tableau in registers, 64-column strips over the workgroups, one exchange per pivot.
    Column partners sit in different strips (col_d 128 .. 1024) or side by side in one strip (col_d 1), row
    partners in different row slots or waves; lds 1: the last 24 columns of a strip in LDS (m <= 256)."""
    L = knobs
    L.mi355x_tune_set_resident(2)
    assert L.mi355x_tune_set_resident_lds(lds) == lds
    path, ref = _capped_run(L, case, kind, prepare=True)
    c = path.counts
    assert c[RESIDENT] > 0 and c[LA_PERSISTENT] == c[LA_TWO_LAUNCH] == c[PER_PIVOT] == 0, c
    path = _request_sequence(L, case, kind, 16)            # every request ONE launch that keeps the tableau on chip
    c = path.counts
    assert path.resident == 1
    assert c[RESIDENT] > 0 and c[LA_PERSISTENT] == c[LA_TWO_LAUNCH] == c[PER_PIVOT] == 0, c


# =========================================================================== 5. signed zeros
def _signed_zero_reference(negative_in_lower_row, hi):
    M0, b0 = tc.signed_zero_case(negative_in_lower_row, hi)
    M, b = M0.copy(), b0.copy()
    st, npiv, trace = oracle.solve(M, b, trace_cap=1 << 10)
    assert tuple(trace[0]) == (tc.SZ_COL, tc.SZ_LO)
    return M0, b0, tc.Reference(st, npiv, trace, M, b)


@pytest.mark.parametrize("hi", tc.SZ_HIGHER, ids=["same-wave", "other-wave"])
@pytest.mark.parametrize("negative_in_lower_row", [False, True], ids=["lower+0-higher-0", "lower-0-higher+0"])
@pytest.mark.parametrize("path", ["per-pivot-one-workgroup", "per-pivot-split", "persistent"])
def test_signed_zero_quotients_tie(knobs, path, negative_in_lower_row, hi):
    """Quotients +0.0 and -0.0 compare equal: the lower row wins whichever holds the minus sign (a hardware
    minimum orders -0.0 first), and the result's zeros keep their signs -- int64 bits.  Both rows in one wave:
    wave_argmin's v_min_f64 butterfly and its `==` ballot meet the two zeros; in two waves: the fold across the
    waves does."""
    L = knobs
    M0, b0, ref = _signed_zero_reference(negative_in_lower_row, hi)
    if path == "persistent":
        L.mi355x_tune_set_lookahead_mode(2)
        L.mi355x_tune_set_block(16)
    else:
        L.mi355x_tune_set_block(1)
        L.mi355x_tune_set_select_mode(1 if path == "per-pivot-one-workgroup" else 2)
    t = lp.Tableau(None, lp.Problem(type="max"), M0, b0, tc.SZ_N + tc.SZ_M, tc.SZ_M, {})
    k = ctypes.c_int64(0)
    rc = L.mi355x_tab_solve(t._h, 1, 1024.0, 0, ctypes.byref(k))
    c = _path(L, t._h).counts
    t._touch()
    assert (rc, k.value) == (ref.status, ref.pivots)
    _same(t, ref, path)
    if path == "persistent":
        assert c[LA_PERSISTENT] > 0 and c[LA_TWO_LAUNCH] == c[PER_PIVOT] == c[RESIDENT] == 0, c
    else:
        assert c[PER_PIVOT] > 0 and (c[SELECT_SPLIT] > 0) == (path == "per-pivot-split"), c
        assert c[LA_PERSISTENT] == c[LA_TWO_LAUNCH] == c[RESIDENT] == 0, c


@pytest.mark.parametrize("batch_block", [1, 16])
def test_signed_zero_quotients_tie_in_a_batch(knobs, batch_block):
    """The four signed-zero cases as the members of one batch, one workgroup per LP (k_batch_solve / k_batch_block)."""
    L = knobs
    cases = [_signed_zero_reference(neg, hi) for hi in tc.SZ_HIGHER for neg in (False, True)]
    assert batch_block == 1 or _batch_block_fits(tc.SZ_N, tc.SZ_M, batch_block)
    L.mi355x_tune_set_batch_mode(2)
    L.mi355x_tune_set_batch_block(batch_block)
    batch = lp.TableauBatch.from_arrays(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
    st, npv = batch.solve()
    assert _batch_counts(L, batch)[B_PER_LP] > 0
    for k, (_, _, ref) in enumerate(cases):
        G, gb = batch.download(k)
        assert (int(st[k]), int(npv[k])) == (ref.status, ref.pivots), k
        assert np.array_equal(G.view(np.int64), ref.M.view(np.int64)) and np.array_equal(gb, ref.basis), k


# =========================================================================== batches
def _batch_counts(L, batch):
    out = (ctypes.c_int64 * 4)()
    lp.capi.check(L.mi355x_batch_path_counts(batch._h, out), "batch_path_counts")
    return list(out)


def _batch_block_fits(n, m, kb):
    """launch_batch_solve takes k_batch_block<kb> only if its block state fits 150 KiB of LDS, and goes on to
    the next smaller block -- in the end to the unblocked k_batch_solve -- without a trace in the counters: the
    cases that name a block size say here that it is the one that runs."""
    rows, ld = m + 1, (n + 1 + 15) // 16 * 16              # the compact member: n non-basic columns + RHS, padded
    rp, ldv = (rows + 1) & ~1, ld >> 1
    return (kb * (ld + rp) + 3 * (ld + rp)) * 8 + (rp + ldv) * 4 <= 150 * 1024


def _check_batch(batch, st, npv, refs, what):
    for k, ref in enumerate(refs):
        G, gb = batch.download(k)
        assert (int(st[k]), int(npv[k])) == (ref.status, ref.pivots), (what, k, int(st[k]), int(npv[k]), ref.status, ref.pivots)
        assert np.array_equal(gb, ref.basis), (what, k)
        assert np.array_equal(G.view(np.int64), ref.M.view(np.int64)), (what, k)


# (batch mode, batch block, compact) -> the driver that must have run.  Left out on purpose: mode 2 with DENSE
# members at batch blocks 4 and 16 -- k_batch_block needs the compact column maps (launch_batch_solve asks for
# t.p2l), so dense members run k_batch_solve whatever the block: the same launch as (2, 1, dense).  In mode 3
# dense members have no split form and take mode 2's kernel.
BATCH_PATHS = [
    (1, 0, 1, B_LOCKSTEP), (1, 0, 0, B_LOCKSTEP),
    (2, 1, 1, B_PER_LP), (2, 4, 1, B_PER_LP), (2, 16, 1, B_PER_LP), (2, 1, 0, B_PER_LP),
    (3, 0, 1, B_SPLIT), (3, 0, 0, B_PER_LP),
]
BATCH_CASES = [(60, 30, 15, 30), (300, 40, 20, 150), (33, 200, 100, 16)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode,batch_block,compact,path", BATCH_PATHS,
                         ids=["mode%d-bb%d-%s" % (a, b, "compact" if c else "dense") for a, b, c, _ in BATCH_PATHS])
@pytest.mark.parametrize("case", BATCH_CASES, ids=_id)
def test_batches(knobs, case, mode, batch_block, compact, path, kind):
    """Six LPs per batch, five with duplicated rows and columns (their ties fall at different steps) and one
    without any: lockstep launch pairs (k_select / k_update over grid.z), one workgroup per LP (k_batch_solve;
    k_batch_block with 4 and 16 pending pivots: bb_reduce), the look-ahead per LP + one sweep over all LPs;
    to the LPs' ends (cap 0) and with a cap inside the first block (5).  The min members are the max
    members with the objective row negated."""
    L = knobs
    L.mi355x_tune_set_batch_mode(mode)
    L.mi355x_tune_set_batch_block(batch_block)
    L.mi355x_tune_set_compact(compact)
    if compact and (mode == 3 or batch_block > 1):         # the blocked kernel named is the one that runs
        assert _batch_block_fits(case[0], case[1], batch_block or 16)
    Ms, Bs = tc.batch(*case, kind)
    for cap in (0, 5):
        batch = lp.TableauBatch.from_arrays(Ms, Bs)
        st, npv = batch.solve(is_max=(kind == "max"), max_pivots=cap)
        c = _batch_counts(L, batch)
        assert c[path] > 0 and sum(c) == c[path], (cap, c)
        _check_batch(batch, st, npv, tc.batch_reference(*case, kind, cap), "cap %d" % cap)


CONFIG4 = (512, 256, 128, 256)


@pytest.mark.parametrize("kind", KINDS)
def test_config4_members_with_default_knobs(knobs, kind):
    """The member shape of config 4 with every knob at its default: the batch runs RESIDENT (k_resident, every
    LP on chip with its own group of workgroups, all LPs in one launch) -- the batch path the benchmark times."""
    L = knobs
    Ms, Bs = tc.batch(*CONFIG4, kind)
    for cap in (0, 5):
        batch = lp.TableauBatch.from_arrays(Ms, Bs)
        st, npv = batch.solve(is_max=(kind == "max"), max_pivots=cap)
        c = _batch_counts(L, batch)
        assert c[B_RESIDENT] > 0 and sum(c) == c[B_RESIDENT], (cap, c)
        _check_batch(batch, st, npv, tc.batch_reference(*CONFIG4, kind, cap), "cap %d" % cap)


def test_multi_device_batch_of_three_sub_batches(knobs):
    """mi355x_multibatch_*: the six members as three sub-batches of two (logical ones where there is one GPU),
    each on its own stream and worker thread; by GLOBAL member index."""
    case = BATCH_CASES[0]
    Ms, Bs = tc.batch(*case, "max")
    mb = lp.MultiDeviceBatch.from_arrays(Ms, Bs, 3)
    assert mb.info()["n_sub_batches"] == 3
    st, npv = mb.solve()
    _check_batch(mb, st, npv, tc.batch_reference(*case, "max", 0), "multibatch")


# =========================================================================== column partitions
# (exchange mode, shard_la_block): 0 the all-reduce form, 2 pushes into the peers' buffers -- the look-ahead of
# a block as ONE persistent launch per device (k_shard_la_block) or the step kernels --, 3 four launches per step
EXCHANGES = [(0, 0), (2, 0), (2, 1), (3, 0)]
COLPART = [(shards, ex, lab, block, rep)
           for shards in sorted(tc.COLPART) for ex, lab in EXCHANGES for block in (16, 24) for rep in ("compact", "dense")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shards,exchange,la_block_off,block,rep", COLPART,
                         ids=["s%d-x%d%s-b%d-%s" % (s, x, "-steps" if o else "", b, r) for s, x, o, b, r in COLPART])
def test_column_partitions(knobs, shards, exchange, la_block_off, block, rep, kind):
    """mi355x_colpart_*: every shard prices its own columns, the shards' winners meet in exchange A -- the
    partner of a low column lies in a LATER shard (compact: always; dense: for a good part of the pairs, the
    others meet inside one shard), the winner must be the lowest GLOBAL column."""
    _colpart_case(knobs, shards, exchange, la_block_off, block, rep, kind)


def _colpart_case(L, shards, exchange, la_block_off, block, rep, kind):
    cp = importlib.import_module("linear-programming_amd.colpart")
    case, dense = tc.COLPART[shards], rep == "dense"
    M0, b0 = tc.single(*case, kind, dense)
    ref = tc.single_reference(*case, kind, dense)
    L.mi355x_tune_set_block(block)
    L.mi355x_tune_set_colpart_exchange(exchange)
    L.mi355x_tune_set_shard_la_block(la_block_off)
    assert ref.pivots > block + 7
    tab = cp.NativeColumnPartition.from_arrays(M0, b0, shards)
    try:
        assert tab.info()["n_shards"] == shards and tab.block_size() == block and tab.is_compact() == (not dense)
        st, k = tab.solve(is_max=(kind == "max"), max_pivots=block + 7)                    # ends inside a block
        assert (st, k) == (lp.capi.MI_MAX_PIVOTS, block + 7)
        st, k2 = tab.solve(is_max=(kind == "max"), max_pivots=tc.CAP - k)
        assert (st, k + k2) == (ref.status, ref.pivots), (st, k + k2, ref.status, ref.pivots)
        tr = tab.trace(ref.pivots)
        bad = np.where((tr != ref.trace).any(axis=1))[0] if tr.shape == ref.trace.shape else [-1]
        assert not len(bad), "pivot trace differs from the oracle's, first at %s: got %s, oracle %s" % (
            bad[:3], tr[bad[:3]].tolist(), ref.trace[bad[:3]].tolist())
        G, gb, last_row, last_col = tab.download()
        assert np.array_equal(gb, ref.basis)
        assert np.array_equal(G.view(np.int64), ref.M.view(np.int64))
        assert np.array_equal(last_row.view(np.int64), ref.M[-1].view(np.int64))
        assert np.array_equal(last_col.view(np.int64), ref.M[:, -1].copy().view(np.int64))
        stats = tab.la_stats()
        if exchange == 2 and not la_block_off:
            assert stats["blocks"] > 0 and stats["losses"] == 0, stats
        else:
            assert stats["blocks"] == 0, stats
    finally:
        tab.close()
