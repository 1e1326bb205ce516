"""Full-size parity (BASELINE configs 3, 4, 5) and the in-launch hand-off of the persistent
look-ahead kernel under load -- the round-1 review's list:

  * config 3: the first 400 pivots bit-identical to the oracle (trace, RHS column, objective
    row, whole tableau), not 24;
  * config 5 at full size: 64 pivots (4 blocks), every selection re-derived in numpy from what
    the GPU holds (objective row -> entering column, entering column + RHS column -> pivot row),
    sampled elements of the rank-1 update recomputed, and the size-independent properties
    (RHS >= 0, objective monotone, basic columns exact unit vectors);
  * config 4: 128 LPs, EVERY LP against the oracle;
  * the hand-off: the same LP solved over and over by the persistent look-ahead (workgroups spread
    over the XCDs and on one XCD) while another stream keeps HBM busy -- every pivot of every
    repetition must be the oracle's; and the lost-exchange path (a workgroup that never
    publishes) must end in a correct solve, not in an error.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle
from tests.helpers import ROOT, lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _synthetic_handle(n, m, seed):
    h = ctypes.c_void_p()
    lp.capi.check(lp.capi.lib().mi355x_tab_create_synthetic(ctypes.byref(h), n, m, seed, 0, -1, 0),
                  "create_synthetic")
    return h


def _trace(h, k):
    ec = np.empty(max(k, 1), dtype=np.int64); cr = np.empty(max(k, 1), dtype=np.int64)
    n = ctypes.c_int64(0)
    lp.capi.check(lp.capi.lib().mi355x_tab_trace(h, _ptr(ec), _ptr(cr), k, ctypes.byref(n)), "trace")
    return np.stack([ec[:k], cr[:k]], axis=1), int(n.value)


# =========================================================================== config 3
def test_config3_400_pivots_bitwise():
    """8192 vars x 4096 constraints: 400 pivots = 25 blocks of the default path (persistent
    look-ahead over 17 workgroups + blocked sweeps), bit for bit against the OpenMP oracle."""
    n, m, K = 8192, 4096, 400
    seed = lp.synth.seed_for(3)
    t = lp.Tableau(None, lp.Problem(type="max"), None, None, n + m, m, {}, _handle=_synthetic_handle(n, m, seed))
    M, b = lp.synth.tableau(n, m, seed)
    st, npiv, trace = oracle.solve(M, b, max_pivots=K, trace_cap=K, omp=True)
    assert (st, npiv) == (oracle.MAX_PIVOTS, K)
    with pytest.raises(lp.SolverError):
        lp.n_solve_tableau(t, max_pivots=K)
    got = t.pivot_trace()
    assert got.shape == trace.shape
    bad = np.where((got != trace).any(axis=1))[0]
    assert not len(bad), "first differing pivots %s: got %s, oracle %s" % (bad[:4], got[bad[:4]], trace[bad[:4]])
    G = t.matrix
    assert np.array_equal(G[:, -1].view(np.int64), M[:, -1].view(np.int64))      # RHS column
    assert np.array_equal(G[m].view(np.int64), M[m].view(np.int64))              # objective row
    assert np.array_equal(G.view(np.int64), M.view(np.int64))                    # everything
    assert np.array_equal(t.basis_columns, b)
    assert lp.capi.lib().mi355x_tab_la_lost(t._h) == 0


# =========================================================================== config 4
def test_config4_128_lps_every_lp_vs_oracle():
    """The per-GPU share of BASELINE config 4 (128 LPs of 512 vars x 256 constraints), default
    batch driver: status, pivot count and final tableau of EVERY LP equal the oracle's."""
    n, m, nl = 512, 256, 128
    seeds = np.array([lp.synth.seed_for(4, k) for k in range(nl)], dtype=np.uint64)
    batch = lp.TableauBatch.synthetic(nl, n, m, seeds)
    st, npv = batch.solve()
    pivots = []
    for k in range(nl):
        M, b = lp.synth.tableau(n, m, int(seeds[k]))
        so, no, _ = oracle.solve(M, b)
        Mg, bg = batch.download(k)
        assert (int(st[k]), int(npv[k])) == (so, no) and so == oracle.OPTIMAL, k
        assert np.array_equal(Mg.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b), k
        pivots.append(no)
    assert len(set(pivots)) > 10                      # the LPs really are different problems


# =========================================================================== config 5
def _block(h, r0, nr, c0, nc):
    out = np.empty((nr, nc))
    lp.capi.check(lp.capi.lib().mi355x_tab_download_block(h, r0, nr, c0, nc, _ptr(out)), "download_block")
    return out


def test_config5_full_size_64_pivots_rederived():
    """65536 vars x 32768 constraints (32769 x 98305 f64 = 25.8 GB; compact 17.2 GB).  No CPU
    oracle can hold this in test time, so the reference's loop is re-derived step by step from
    what the GPU holds: with the tableau state S_k after k pivots (k = 0, 16, 32, 48: the block
    boundaries, plus every single pivot of the first block),
      find-entering-column(S_k) in numpy == the GPU's next entering column,
      find-pivoting-row(S_k, ec) in numpy == the GPU's next pivot row,
    sampled entries of S_{k+1} == n-pivot-row's formula on S_k (two roundings, no FMA), and the
    size-independent properties hold at every checkpoint.  The blocked solver (4 blocks of 16 with
    the two-launch look-ahead) must take exactly the pivots of the per-pivot kernels."""
    L = lp.capi.lib()
    n, m, K = 65536, 32768, 64
    vc = n + m
    seed = lp.synth.seed_for(5)
    eps = oracle.EPSILON

    def price(obj):                                   # src/simplex.lisp:362-372 (max problem)
        j = int(np.argmin(obj[:vc]))                  # first index of the minimum
        return j if obj[j] < 0.0 - 128 * eps else -1

    def ratio(col, rhs):                              # src/simplex.lisp:382-389
        ok = col[:m] > 0.0 + 512 * eps
        if not ok.any():
            return -1
        q = np.full(m, np.inf)
        q[ok] = rhs[:m][ok] / col[:m][ok]
        return int(np.argmin(q))                      # first index of the minimum

    # (1) the blocked default path: 64 pivots, trace + state at the end
    h = _synthetic_handle(n, m, seed)
    assert L.mi355x_tab_solve(h, 1, 1024.0, K, None) == lp.capi.MI_MAX_PIVOTS
    trace, cnt = _trace(h, K)
    assert cnt == K
    rhs_blocked = _block(h, 0, m + 1, vc, 1)[:, 0]
    obj_blocked = _block(h, m, 1, 0, vc + 1)[0]
    basis_blocked = np.empty(m, dtype=np.int64)
    lp.capi.check(L.mi355x_tab_download(h, None, _ptr(basis_blocked), None, None), "basis")
    L.mi355x_tab_destroy(h)

    # (2) step-wise on a second handle: per-pivot kernels through the step-wise entry points
    # (a different code path: k_price_only / k_ratio_only / k_prepare_pivot + k_update, dense)
    h = _synthetic_handle(n, m, seed)
    rng = np.random.default_rng(5)
    obj_prev = None
    for k in range(K):
        check = k < 16 or k % 16 == 0
        ec, cr = int(trace[k, 0]), int(trace[k, 1])
        if check:
            obj = _block(h, m, 1, 0, vc + 1)[0]
            rhs = _block(h, 0, m + 1, vc, 1)[:, 0]
            col = _block(h, 0, m + 1, ec, 1)[:, 0]
            assert price(obj) == ec, "pivot %d: numpy prices column %d, the GPU took %d" % (k, price(obj), ec)
            assert ratio(col, rhs) == cr, "pivot %d: numpy ratio test gives row %d, the GPU took %d" % (k, ratio(col, rhs), cr)
            assert rhs[:m].min() >= 0.0                               # primal feasible throughout
            if obj_prev is not None:
                assert obj[vc] >= obj_prev                            # objective never decreases
            obj_prev = obj[vc]
            # sample of the update: rows x columns incl. the pivot row / column and the objective row
            rows = np.unique(np.concatenate([rng.integers(0, m + 1, 6), [cr, m]]))
            cols = np.unique(np.concatenate([rng.integers(0, vc + 1, 6), [ec, vc]]))
            before = np.array([[_block(h, int(r), 1, int(c), 1)[0, 0] for c in cols] for r in rows])
            prow_before = np.array([_block(h, cr, 1, int(c), 1)[0, 0] for c in cols])
        got_ec, got_cr = ctypes.c_int64(-2), ctypes.c_int64(-2)
        lp.capi.check(L.mi355x_tab_price(h, 1, 1024.0, ctypes.byref(got_ec)), "price")
        lp.capi.check(L.mi355x_tab_ratio(h, ec, 1024.0, ctypes.byref(got_cr)), "ratio")
        assert (got_ec.value, got_cr.value) == (ec, cr), "pivot %d: step-wise kernels disagree with the blocked solve" % k
        lp.capi.check(L.mi355x_tab_pivot(h, ec, cr), "pivot")
        if check:
            piv = col[cr]
            prow = prow_before / piv                                  # true division
            for i, r in enumerate(rows):
                for j in range(len(cols)):
                    want = prow[j] if r == cr else before[i, j] - col[r] * prow[j]   # product, then difference
                    got = _block(h, int(r), 1, int(cols[j]), 1)[0, 0]
                    assert got == want or (np.isnan(got) and np.isnan(want)), (k, int(r), int(cols[j]), got, want)
    rhs_step = _block(h, 0, m + 1, vc, 1)[:, 0]
    obj_step = _block(h, m, 1, 0, vc + 1)[0]
    assert np.array_equal(rhs_step.view(np.int64), rhs_blocked.view(np.int64))
    assert np.array_equal(obj_step.view(np.int64), obj_blocked.view(np.int64))
    # basic columns are exact unit vectors with +0.0 in the objective row (sample of 24 + the
    # last entered ones), non-basic reduced costs live where the basis is not
    for i in list(rng.integers(0, m, 24)) + [int(c) for c in trace[-4:, 1]]:
        colv = _block(h, 0, m + 1, int(basis_blocked[i]), 1)[:, 0]
        unit = np.zeros(m + 1); unit[i] = 1.0
        assert np.array_equal(colv.view(np.int64), unit.view(np.int64)), i
    assert len(set(basis_blocked.tolist())) == m
    assert set(trace[:, 0].tolist()) <= set(basis_blocked.tolist()) | set(range(n))
    L.mi355x_tab_destroy(h)


@pytest.mark.slow
@pytest.mark.timeout(1500, method="thread")
def test_config5_full_size_64_pivots_vs_the_oracle():
    """The same 32769 x 98305 tableau through the CPU ORACLE (OpenMP row-parallel restatement of
    src/simplex.lisp:337-389, 453-461) on the box's host cores: the dense 25.8 GB tableau the GPU
    generated is downloaded (sampled rows, the whole RHS column and objective row checked against
    the numpy generator first), the oracle makes 64 pivots on it in host memory, the GPU makes
    its 64 pivots in HBM -- two WIDE blocks of 28 pivots per sweep, the default at this size since
    round 4, and the 8 pivots the cap leaves of the third (a block cut short: k_sweepw_rest) --
    and then pivot trace, basis and EVERY entry of the tableau must agree bit for bit."""
    import time
    n, m, K = 65536, 32768, 64
    seed = lp.synth.seed_for(5)
    t = lp.Tableau(None, lp.Problem(type="max"), None, None, n + m, m, {}, _handle=_synthetic_handle(n, m, seed))
    t0 = time.perf_counter()
    M = t.matrix                                       # the initial tableau as the GPU holds it
    b = t.basis_columns.copy()
    t_down = time.perf_counter() - t0
    assert M.shape == (m + 1, n + m + 1)
    # ... which is the generator's LP (linear-programming_amd/synth.py; its numpy form at this size
    # would take minutes): sampled rows entirely, RHS column and objective row entirely
    for i in (0, 1, 777, 16384, m - 1):
        row = np.zeros(n + m + 1)
        row[:n] = 0.05 + lp.synth.splitmix_u01(seed, i * n, n)
        row[n + i] = 1.0
        row[n + m] = float(n) * (0.25 + 0.5 * lp.synth.splitmix_u01(seed, n * m + i, 1)[0])
        assert np.array_equal(M[i].view(np.int64), row.view(np.int64)), i
    assert np.array_equal(M[:m, n + m], float(n) * (0.25 + 0.5 * lp.synth.splitmix_u01(seed, n * m, m)))
    obj = np.zeros(n + m + 1)
    obj[:n] = -(0.5 + lp.synth.splitmix_u01(seed, n * m + m, n))
    assert np.array_equal(M[m].view(np.int64), obj.view(np.int64))
    assert np.array_equal(b, np.arange(n, n + m))
    t0 = time.perf_counter()
    st, npiv, trace = oracle.solve(M, b, max_pivots=K, trace_cap=K, omp=True)
    t_orc = time.perf_counter() - t0
    assert (st, npiv) == (oracle.MAX_PIVOTS, K)
    t._touch()
    with pytest.raises(lp.SolverError):
        lp.n_solve_tableau(t, max_pivots=K)
    assert lp.capi.lib().mi355x_tab_block_size(t._h) == 28
    got = t.pivot_trace()
    assert got.shape == trace.shape
    bad = np.where((got != trace).any(axis=1))[0]
    assert not len(bad), "first differing pivots %s: got %s, oracle %s" % (bad[:4], got[bad[:4]], trace[bad[:4]])
    t0 = time.perf_counter()
    G = t.matrix
    assert G is not M
    assert np.array_equal(t.basis_columns, b)
    assert np.array_equal(G[:, -1].view(np.int64), M[:, -1].view(np.int64))      # RHS column
    assert np.array_equal(G[m].view(np.int64), M[m].view(np.int64))              # objective row
    for r0 in range(0, m + 1, 2048):                                             # everything
        assert np.array_equal(G[r0:r0 + 2048].view(np.int64), M[r0:r0 + 2048].view(np.int64)), r0
    t_cmp = time.perf_counter() - t0
    assert lp.capi.lib().mi355x_tab_la_lost(t._h) == 0
    del G, t
    # ---- the SAME tableau as BASELINE config 5 specifies it: column-partitioned into 8 shards,
    # the library's per-pivot loop with both exchanges per pivot (mi355x_colpart_*) -- 8 logical
    # shards on this one GPU, i.e. everything of the 8-GPU run but the wire -- against the same
    # oracle result, every entry; the default exchange and the collective-free P2P push
    from importlib import import_module
    cp = import_module("linear-programming_amd.colpart")
    L = lp.capi.lib()
    t_cp = []
    for mode in (0, 2):
        L.mi355x_tune_set_colpart_exchange(mode)
        try:
            part = cp.NativeColumnPartition.synthetic(n, m, seed, 8)
        finally:
            L.mi355x_tune_set_colpart_exchange(0)
        assert part.info()["n_shards"] == 8
        t0 = time.perf_counter()
        rc, npv = part.solve(max_pivots=K)
        t_cp.append(time.perf_counter() - t0)
        assert (rc, npv) == (lp.capi.MI_MAX_PIVOTS, K)
        Gp, bp, _, _ = part.download()
        part.close()
        assert np.array_equal(bp, b), mode
        for r0 in range(0, m + 1, 2048):
            assert np.array_equal(Gp[r0:r0 + 2048].view(np.int64), M[r0:r0 + 2048].view(np.int64)), (mode, r0)
        del Gp
    print("config 5 vs oracle: download %.1f s, oracle %.1f s for %d pivots (%d threads), download + compare %.1f s; "
          "8 logical shards: %.3f s (device-local exchanges), %.3f s (P2P push)"
          % (t_down, t_orc, K, oracle.omp_threads(), t_cmp, t_cp[0], t_cp[1]))


# =========================================================================== the hand-off
def _background_load(torch, stop_after_s=60.0):
    """A stream that keeps HBM busy (uneven load next to the look-ahead kernel): big device
    copies enqueued ahead; returns (stream, buffers) to keep alive."""
    s = torch.cuda.Stream()
    a = torch.empty(1 << 28, dtype=torch.float64, device="cuda")      # 2 GiB
    b = torch.empty_like(a)
    return s, a, b


@pytest.mark.parametrize("one_xcd", [1, 0], ids=["one-xcd", "spread"])
@pytest.mark.parametrize("n,m", [(1500, 700), (2600, 2300)])
def test_persistent_lookahead_handoff_under_load(n, m, one_xcd):
    """The same LP, 60 solves of up to 320 pivots each by the persistent look-ahead (3 / 10
    workgroups), while a second stream streams 4 GiB copies through HBM: every pivot of every
    repetition must be the oracle's pivot (a stale hand-off shows up as a different pivot)."""
    import torch
    L = lp.capi.lib()
    seed = lp.synth.seed_for(2, n + m)
    M0, b0 = lp.synth.tableau(n, m, seed)
    M, b = M0.copy(), b0.copy()
    cap = 320
    st_o, npiv, trace = oracle.solve(M, b, max_pivots=cap, trace_cap=cap, omp=True)
    stream, src, dst = _background_load(torch)
    try:
        L.mi355x_tune_set_lookahead_mode(2)
        L.mi355x_tune_set_la_one_xcd(one_xcd)
        t = lp.Tableau(None, lp.Problem(type="max"), M0, b0, n + m, m, {})
        for rep in range(60):
            with torch.cuda.stream(stream):
                for _ in range(4):
                    dst.copy_(src, non_blocking=True)
            lp.capi.check(L.mi355x_tab_upload(t._h, _ptr(M0), _ptr(b0)), "upload")
            k = ctypes.c_int64(0)
            rc = L.mi355x_tab_solve(t._h, 1, 1024.0, cap, ctypes.byref(k))
            assert (rc, k.value) == (st_o, npiv), rep
            got, _ = _trace(t._h, npiv)
            bad = np.where((got != trace).any(axis=1))[0]
            assert not len(bad), "repetition %d, first differing pivots %s" % (rep, bad[:4])
        t._touch()
        assert np.array_equal(t.matrix.view(np.int64), M.view(np.int64))
        assert L.mi355x_tab_la_lost(t._h) == 0
    finally:
        L.mi355x_tune_set_lookahead_mode(0)
        L.mi355x_tune_set_la_one_xcd(1)
        torch.cuda.synchronize()


@pytest.mark.parametrize("fault_step", [1, 4, 16, -1, -4, -9, -16])
def test_lost_exchange_falls_back_to_two_launch_lookahead(fault_step, hooks_lib):
    """A workgroup of the persistent look-ahead that stops publishing (what a workgroup that is
    not resident looks like to the others): the others give up after the poll bound, the pivots
    selected before are applied, the host switches the handle to the two-launch look-ahead and the
    solve ends with the oracle's pivots and bits -- no error, no hang.
    fault_step < 0: ONE workgroup gives up alone, right after publishing its ratio record of step
    -fault_step - 1 -- every workgroup times out on its own, so the leader still sees all records
    and commits a pivot whose col / prow entries that workgroup never stored (round-2 advisor
    finding).  The sweep must apply only what every workgroup completed (BlockCtl::done) and the
    recovery must take the leader's bookkeeping of that one pivot back (k_la_rollback)."""
    L = hooks_lib
    n, m = 1500, 700
    seed = lp.synth.seed_for(2, 77)
    M0, b0 = lp.synth.tableau(n, m, seed)
    M, b = M0.copy(), b0.copy()
    st_o, npiv, trace = oracle.solve(M, b, max_pivots=200, trace_cap=200)
    try:
        L.mi355x_tune_set_la_max_spins(20000)
        L.mi355x_tune_set_la_fault(fault_step)
        t = lp.Tableau(None, lp.Problem(type="max"), M0, b0, n + m, m, {})
        k = ctypes.c_int64(0)
        rc = L.mi355x_tab_solve(t._h, 1, 1024.0, 200, ctypes.byref(k))
        t._touch()
    finally:
        L.mi355x_tune_set_la_max_spins(0)
        L.mi355x_tune_set_la_fault(0)
    assert (rc, k.value) == (st_o, npiv)
    assert L.mi355x_tab_la_lost(t._h) == 1
    assert np.array_equal(t.pivot_trace(), trace)
    assert np.array_equal(t.matrix.view(np.int64), M.view(np.int64))
    assert np.array_equal(t.basis_columns, b)
    # the handle stays usable (and stays on the two-launch look-ahead)
    rc = L.mi355x_tab_solve(t._h, 1, 1024.0, 0, ctypes.byref(k))
    t._touch()
    M2, b2 = M0.copy(), b0.copy()
    so2, no2, _ = oracle.solve(M2, b2)
    assert rc == so2 and np.array_equal(t.matrix.view(np.int64), M2.view(np.int64))


@pytest.mark.parametrize("fault_step", [3, -3, -16])
def test_lost_exchange_through_solve_async_and_sync(fault_step, hooks_lib):
    """The same through the asynchronous entry points: mi355x_tab_sync reports MI_RUNNING with
    FEWER pivots than requested (documented), the count is what the tableau really holds, and
    enqueueing the difference reaches the oracle's state bit for bit -- also with the persistent
    look-ahead forced (mode 2), which must not be re-launched for ever on such a handle."""
    L = hooks_lib
    n, m = 1500, 700
    seed = lp.synth.seed_for(2, 78)
    M0, b0 = lp.synth.tableau(n, m, seed)
    want = 48
    M, b = M0.copy(), b0.copy()
    st_o, npiv, trace = oracle.solve(M, b, max_pivots=want, trace_cap=want)
    assert npiv == want
    try:
        L.mi355x_tune_set_la_max_spins(20000)
        L.mi355x_tune_set_la_fault(fault_step)
        L.mi355x_tune_set_lookahead_mode(2)
        t = lp.Tableau(None, lp.Problem(type="max"), M0, b0, n + m, m, {})
        k = ctypes.c_int64(0)
        lp.capi.check(L.mi355x_tab_solve_async(t._h, 1, 1024.0, want, 1), "solve_async")
        rc = L.mi355x_tab_sync(t._h, ctypes.byref(k))
        assert rc == lp.capi.MI_RUNNING and 0 <= k.value < want and L.mi355x_tab_la_lost(t._h) == 1
        applied = abs(fault_step) - 1                # pivots every workgroup had completed
        assert k.value == applied
        lp.capi.check(L.mi355x_tab_solve_async(t._h, 1, 1024.0, want - k.value, 0), "solve_async (rest)")
        rc = L.mi355x_tab_sync(t._h, ctypes.byref(k))
        t._touch()
    finally:
        L.mi355x_tune_set_la_max_spins(0)
        L.mi355x_tune_set_la_fault(0)
        L.mi355x_tune_set_lookahead_mode(0)
    assert (rc, k.value) == (lp.capi.MI_RUNNING, want)
    assert np.array_equal(t.pivot_trace()[:want], trace)
    assert np.array_equal(t.matrix.view(np.int64), M.view(np.int64))
    assert np.array_equal(t.basis_columns, b)


# =========================================================================== multi-device C ABI
@pytest.mark.parametrize("n_devices", [1, 2, 3, 8])
@pytest.mark.parametrize("n,m,seed", [(96, 64, 1), (700, 333, 2)])
def test_colpart_c_abi_logical_shards_bitwise(n, m, seed, n_devices):
    """mi355x_colpart_*: the whole column-partitioned solve behind the C ABI (per-pivot loop and
    both exchanges in C++).  This box has one GPU, so n_devices > 1 means logical shards on it with
    device-local exchanges of the collectives' semantics: pivots and every bit as the oracle's."""
    import importlib
    cp = importlib.import_module("linear-programming_amd.colpart")
    M0, b0 = lp.synth.tableau(n, m, lp.synth.seed_for(5, seed))
    M, b = M0.copy(), b0.copy()
    st_o, npiv, trace = oracle.solve(M, b, trace_cap=1 << 14)
    tab = cp.NativeColumnPartition.from_arrays(M0, b0, n_devices)
    info = tab.info()
    assert info["n_shards"] == n_devices
    st, k = tab.solve()
    assert (st, k) == (st_o, npiv)
    assert np.array_equal(tab.trace(npiv), trace)
    G, bg, last_row, last_col = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    assert np.array_equal(last_row.view(np.int64), M[m].view(np.int64))
    assert np.array_equal(last_col.view(np.int64), M[:, -1].view(np.int64))
    tab.close()


def test_colpart_c_abi_cap_resume_synthetic_and_dense_fallback():
    import importlib
    cp = importlib.import_module("linear-programming_amd.colpart")
    n, m = 300, 120
    seed = lp.synth.seed_for(5, 7)
    M, b = lp.synth.tableau(n, m, seed)
    tab = cp.NativeColumnPartition.synthetic(n, m, seed, 4)
    st, k = tab.solve(max_pivots=37)                             # stops inside a block
    assert (st, k) == (lp.capi.MI_MAX_PIVOTS, 37)
    oracle.solve(M, b, max_pivots=37)
    G, bg, _, _ = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    st, k2 = tab.solve()                                         # resume to optimality
    so, no, _ = oracle.solve(M, b)
    assert (st, k2) == (so, no)
    G, bg, _, _ = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    tab.close()
    # a basis that is not a set of unit columns: dense shards (every logical column distributed)
    M0, b0 = lp.synth.tableau(40, 25, 3)
    M0[:25, 40:65] *= 2.0                                        # slack "identity" scaled: basis columns != e_i
    M, b = M0.copy(), b0.copy()
    so, no, trace = oracle.solve(M, b, trace_cap=4096)
    tab = cp.NativeColumnPartition.from_arrays(M0, b0, 3)
    st, k = tab.solve()
    assert (st, k) == (so, no) and np.array_equal(tab.trace(no), trace)
    G, bg, _, _ = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    tab.close()


@pytest.mark.parametrize("exchange", [0, 1, 2, 12, 13, 22],
                         ids=["allreduce", "rooted-broadcast", "p2p-push", "p2p-two-launch-step", "p2p-four-launch-step",
                              "p2p-persistent-block"])
@pytest.mark.parametrize("entry", ["comm-init-all", "comm-init-rank"])
def test_colpart_c_abi_over_rccl_single_rank(monkeypatch, entry, exchange):
    """The RCCL code path itself on the one GPU this box has: a single shard forced through its
    one-rank communicator -- ncclAllGather + ncclAllReduce (or, exchange 1, ncclBroadcast from the
    owner with the root read back from the all-gather; or, exchange 2, no collective at all: the
    P2P push / poll kernels on the shard's own fine-grained buffer) on the shard's stream,
    communicator teardown.  Both ways in: ncclCommInitAll (one process, what the Lisp host's `:devices` reaches)
    and EXACTLY what `bench.py --gpus N` does on every rank -- mi355x_rccl_unique_id ->
    mi355x_colpart_create_synthetic_rank(world, rank, device, id) -> ncclCommInitRank -- at
    world = 1.  (Two ranks need two devices: RCCL refuses two ranks on one GPU.)"""
    import importlib
    cp = importlib.import_module("linear-programming_amd.colpart")
    monkeypatch.setenv("MI355X_COLPART_FORCE_RCCL", "1")
    n, m = 500, 260
    seed = lp.synth.seed_for(5, 11)
    M, b = lp.synth.tableau(n, m, seed)
    so, no, trace = oracle.solve(M, b, trace_cap=1 << 14)
    L = lp.capi.lib()
    # 12 / 13: exchange 2 / 3 with the multi-workgroup look-ahead step of large shards forced at this
    # size -- 12 is then the two-launch step (k_shard_p2p_step: the shard has its stream to itself),
    # 13 the same step as four launches
    # 22 (round 6): exchange 2 with the look-ahead of a whole block as ONE persistent launch (k_shard_la_block);
    # the other P2P cases keep that form off, so that the step kernels they name are what runs
    persistent = exchange == 22
    split = 2 if 10 <= exchange < 20 else 0
    exchange = exchange % 10
    try:
        L.mi355x_tune_set_colpart_exchange(exchange)
        L.mi355x_tune_set_shard_la_split(split)
        L.mi355x_tune_set_shard_la_block(0 if persistent else 1)
        if entry == "comm-init-rank":
            uid = cp.NativeColumnPartition.rccl_unique_id()
            assert len(uid) == 128 and any(uid)
            tab = cp.NativeColumnPartition.synthetic_rank(n, m, seed, 1, 0, 0, uid)
        else:
            tab = cp.NativeColumnPartition.synthetic(n, m, seed, 1)
    finally:
        L.mi355x_tune_set_colpart_exchange(0)
        L.mi355x_tune_set_shard_la_block(0)
    assert tab.info() == {"n_shards": 1, "n_devices_used": 1, "uses_rccl": True}
    tab.exchange_timing(4, 64)
    try:
        st, k = tab.solve()
    finally:
        L.mi355x_tune_set_shard_la_split(0)
    assert (st, k) == (so, no) and np.array_equal(tab.trace(no), trace)
    stats = tab.la_stats()
    assert (stats["blocks"] > 0) == persistent and stats["losses"] == 0, stats
    ns, ag_us, ar_us = tab.exchange_timing_read()
    if exchange >= 2:
        assert ns == 0                       # no collective to bracket: the exchanges are inside the step kernels
    else:
        assert 0 < ns <= 64 and 0.0 < ag_us < 1e5 and 0.0 < ar_us < 1e5      # both collectives were bracketed
    G, bg, _, _ = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    tab.close()


@pytest.mark.parametrize("persistent", [False, True], ids=["step-kernels", "persistent-block"])
@pytest.mark.parametrize("n_devices", [1, 2, 3, 8])
@pytest.mark.parametrize("n,m,seed", [(96, 64, 1), (700, 333, 2)])
def test_colpart_p2p_exchange_logical_shards_bitwise(n, m, seed, n_devices, persistent):
    """Exchange mode 2 -- every shard writes its pricing pair and (the owner) the entering column
    straight into the other shards' fine-grained buffers as self-validating granules, the consumers
    poll their own buffer: no collective, no host in the loop.  On this one GPU the shards are
    logical (all producers of an exchange are enqueued before its consumers on the one stream), so
    the data path, the buffer layout, the parities and the tags are what is exercised here; the
    cross-device visibility of the stores needs a multi-GPU node.  Pivots and bits as the oracle's,
    incl. a capped solve that resumes (the tags go on counting) and the two-phase hand-over.
    persistent-block (round 6, the default of this mode): the look-ahead of a whole block of ALL the logical
    shards as ONE launch of k_shard_la_block -- the shards' workgroups are co-resident by construction and
    wait for each other's pairs / column granules inside the kernel, as the shards of a multi-GPU run do."""
    import importlib
    cp = importlib.import_module("linear-programming_amd.colpart")
    L = lp.capi.lib()
    M0, b0 = lp.synth.tableau(n, m, lp.synth.seed_for(5, seed))
    M, b = M0.copy(), b0.copy()
    st_o, npiv, trace = oracle.solve(M, b, trace_cap=1 << 14)
    L.mi355x_tune_set_shard_la_block(0 if persistent else 1)
    try:
        L.mi355x_tune_set_colpart_exchange(2)
        tab = cp.NativeColumnPartition.from_arrays(M0, b0, n_devices)
    finally:
        L.mi355x_tune_set_colpart_exchange(0)
    st, k = tab.solve(max_pivots=23)
    assert (st, k) == (lp.capi.MI_MAX_PIVOTS, 23)
    st, k = tab.solve()
    assert (st, k) == (st_o, npiv - 23)
    assert np.array_equal(tab.trace(npiv), trace)
    stats = tab.la_stats()
    assert (stats["blocks"] > 0) == persistent and stats["losses"] == 0, stats
    G, bg, last_row, last_col = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    tab.close()
    # two-phase on the partition, exchanges in mode 2 (drive-out pivots push their column the same way)
    from tests.helpers import random_mixed_problem
    problem = random_mixed_problem(lp, 30, 10, 8, 4, seed)
    tabs = lp.build_tableau(problem, problem)
    art, main = tabs
    A, ab = art.matrix.copy(), art.basis_columns.copy()
    Mm, mb = main.matrix.copy(), main.basis_columns.copy()
    so, npv = oracle.solve_two_phase(A, ab, Mm, mb, main_is_max=main.is_max)
    try:
        L.mi355x_tune_set_colpart_exchange(2)
        tab = cp.NativeColumnPartition.from_arrays(art.matrix.copy(), art.basis_columns.copy(), n_devices)
        rc, got, mt = tab.solve_two_phase(main.matrix[-1].copy(), main.is_max, 1024)
    finally:
        L.mi355x_tune_set_colpart_exchange(0)
        L.mi355x_tune_set_shard_la_block(0)
    assert rc == so
    GA, ga, _, _ = tab.download()
    assert np.array_equal(GA.view(np.int64), A.view(np.int64)) and np.array_equal(ga, ab)
    if mt is not None:
        GM, gm, _, _ = mt.download()
        assert got == (int(npv[0]), int(npv[1]))
        assert np.array_equal(GM.view(np.int64), Mm.view(np.int64)) and np.array_equal(gm, mb)
        mt.close()
    tab.close()
    L.mi355x_tune_set_shard_la_block(0)


def test_bench_colpart_one_rank_through_the_multi_gpu_entry():
    """`bench.py --workload colpart --gpus 1 --full` forced through the branch N > 1 takes (unique id ->
    create_synthetic_rank -> ncclCommInitRank -> collectives on a one-rank communicator), incl. the
    second leg with the rooted-broadcast exchange and the steady-state figure."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, MI355X_COLPART_FORCE_RCCL="1", BENCH_COLPART_RANK_ENTRY="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "colpart", "--gpus", "1",
                          "--steps", "20", "--warmup", "5", "--colpart-vars", "4096", "--full"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["rccl_ranks"] == 1 and "ncclCommInitRank" in rec["config"]["driver"]
    assert rec["value"] > 0 and rec["steady_state_pivots_per_s"] > 0
    assert rec["exchange"]["samples"] > 0
    modes = rec["exchange_modes"]
    assert modes["int64_sum_allreduce"]["value"] > 0 and modes["rooted_broadcast"]["value"] > 0
    assert modes["p2p_push"]["value"] > 0
    # every mode must end in the default mode's state bit for bit; the headline is the fastest of them
    assert modes["rooted_broadcast"]["identical_to_default_mode"] and modes["p2p_push"]["identical_to_default_mode"]
    # (round 6) the P2P leg runs the look-ahead of a block as one persistent launch; the step kernels beside it
    assert modes["p2p_push"]["persistent_block_launch"]["live"] and not modes["p2p_push_step_kernels"]["persistent_block_launch"]["live"]
    assert modes["p2p_push_step_kernels"]["value"] > 0 and modes["p2p_push_step_kernels"]["identical_to_default_mode"]
    # the headline is the library's DEFAULT exchange; the fastest bit-identical mode is reported next to it
    assert rec["value_mode"] == "int64_sum_allreduce" and rec["value"] == modes["int64_sum_allreduce"]["value"]
    assert rec["best_mode"]["mode"] in modes and rec["best_mode"]["value"] >= rec["value"]


def test_plain_c_client_on_the_gpu(tmp_path):
    """tests/c_abi_check.c with a device present: the native solver and the column-partitioned
    entry points (2 logical shards) from a plain C program, the way a non-Python host binds them."""
    import os
    import subprocess
    from tests.helpers import ROOT
    exe = str(tmp_path / "c_abi_check")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_check.c"), "-o", exe,
                           "-L", os.path.dirname(lp.capi.LIB_PATH), "-lmi355x_simplex",
                           "-Wl,-rpath," + os.path.dirname(lp.capi.LIB_PATH)])
    out = subprocess.check_output([exe], text=True)
    assert "solved on the GPU: w = 28.5, x = 0.5" in out and "c abi ok" in out


@pytest.mark.parametrize("n_shards", [1, 3])
@pytest.mark.parametrize("dense", [False, True], ids=["compact-shards", "dense-shards"])
def test_colpart_split_lookahead_step_bitwise(n_shards, dense):
    """The local look-ahead step of a shard spread over many workgroups (k_shard_la_ratio +
    k_shard_la_scale<J>: what large shards -- config 5 on few GPUs -- run), forced on at a size
    the oracle can follow: pivots and bits as the oracle's, compact and dense shards."""
    import importlib
    cp = importlib.import_module("linear-programming_amd.colpart")
    L = lp.capi.lib()
    n, m = 900, 420
    M0, b0 = lp.synth.tableau(n, m, lp.synth.seed_for(5, 21))
    if dense:
        M0[:m, n:n + m] *= 2.0                                   # basis columns != e_i: every column is distributed
    M, b = M0.copy(), b0.copy()
    so, no, trace = oracle.solve(M, b, max_pivots=150, trace_cap=150)
    try:
        L.mi355x_tune_set_shard_la_split(2)
        tab = cp.NativeColumnPartition.from_arrays(M0, b0, n_shards)
        st, k = tab.solve(max_pivots=150)
    finally:
        L.mi355x_tune_set_shard_la_split(0)
    assert (st, k) == (so, no) and np.array_equal(tab.trace(no), trace)
    G, bg, _, _ = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    tab.close()


def _bench_two_ranks(extra_env, extra_args=()):
    import json
    import socket
    import subprocess
    import sys
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, BENCH_SHARE_DEVICE="1", BENCH_DIST_BACKEND="gloo", **extra_env)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
         "--gpus", "2", "--steps", "20", "--warmup", "5", "--colpart-vars", "2048", *extra_args],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_headline_is_the_column_partition():
    """`bench.py --gpus 2` as the driver launches it (two ranks; here both on the one GPU with the
    scalar reductions over gloo, where the shards' exchanges are staged through the host), with `--full`:
    ONE JSON line, the strong-scaling column-partition record with the independent LPs attached."""
    rec = _bench_two_ranks({}, ["--full"])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "strong" and rec["steps"] == 20
    assert rec["value"] > 0 and "column-partitioned" in rec["config"]["workload"]
    # the ranks share the one GPU: the library's own loop runs in exchange mode 2 (P2P push) without a
    # communicator, and the record carries its own one-GPU baseline, speed-up and steady-state figure
    assert "exchange mode 2" in rec["config"]["driver"] and rec["rccl_ranks"] == 0
    assert rec["one_gpu_same_workload"]["value"] > 0 and rec["speedup_vs_one_gpu"] > 0
    assert rec["steady_state_pivots_per_s"] > 0 and rec["one_gpu_same_workload"]["steady_state_pivots_per_s"] > 0
    weak = rec["independent_lps_weak_scaling"]
    assert weak["scaling"] == "weak" and weak["value"] > 0 and weak["roofline"]["frac"] > 0


def test_bench_two_ranks_watchdog_still_prints_a_line():
    """The column-partition leg under a watchdog that fires at once: the weak-scaling record is
    printed with the reason (a run that hangs in a collective must not end without a line)."""
    rec = _bench_two_ranks({"BENCH_COLPART_TIMEOUT": "0.001"})
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and "did not finish" in rec["colpart_error"]


@pytest.mark.parametrize("exchange", [0, 1, 2], ids=["allreduce", "rooted-broadcast", "p2p-push"])
@pytest.mark.parametrize("n_devices", [2, 4, 8])
def test_colpart_over_rccl_on_real_devices(n_devices, exchange):
    """The column partition with one shard per PHYSICAL GPU (ncclCommInitAll, one host thread and one
    RCCL rank per device, all-gather + all-reduce over xGMI per pivot).  Needs that many GPUs in
    this process: skipped on the one-GPU test box, where the same code runs over a one-rank
    communicator (test_colpart_c_abi_over_rccl_single_rank) and as logical shards."""
    import importlib
    if lp.capi.device_count() < n_devices:
        pytest.skip("needs %d GPUs, %d visible" % (n_devices, lp.capi.device_count()))
    cp = importlib.import_module("linear-programming_amd.colpart")
    n, m = 1500, 700
    seed = lp.synth.seed_for(5, 21)
    M, b = lp.synth.tableau(n, m, seed)
    so, no, trace = oracle.solve(M, b, trace_cap=1 << 14)
    try:
        lp.capi.lib().mi355x_tune_set_colpart_exchange(exchange)
        tab = cp.NativeColumnPartition.synthetic(n, m, seed, n_devices)
    finally:
        lp.capi.lib().mi355x_tune_set_colpart_exchange(0)
    assert tab.info() == {"n_shards": n_devices, "n_devices_used": n_devices, "uses_rccl": True}
    tab.exchange_timing(8, 64)
    st, k = tab.solve()
    assert (st, k) == (so, no) and np.array_equal(tab.trace(no), trace)
    stats = tab.la_stats()
    assert (stats["blocks"] > 0) == persistent and stats["losses"] == 0, stats
    ns, ag_us, ar_us = tab.exchange_timing_read()
    assert ns > 0 and ag_us > 0.0 and ar_us > 0.0
    G, bg, _, _ = tab.download()
    assert np.array_equal(G.view(np.int64), M.view(np.int64)) and np.array_equal(bg, b)
    tab.close()
