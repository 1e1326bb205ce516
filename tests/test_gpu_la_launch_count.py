"""The persistent look-ahead launches a thread per constraint row and per pair of non-RHS columns
(csrc/kernels_la_block.inc, la_launch_workgroups): the objective row and the RHS column have no owner.
col_J[m] is the pricing winner's key, prow_J[vc] is the winning row's RHS entry over the pivot; both are
stored for the sweeps by designated threads (tests/test_la_ownerless_identities.py is the argument).

Here: the smallest shapes at which the launched count differs from max(rows, ld / 2) / 256 -- by the rows,
by the pairs, by both, with the RHS sharing a pair with a column (odd vc), at exactly 64 and exactly 128
records -- and one where it does not; both kernel forms; a lost exchange on the narrower launch; a
non-finite objective-row entry of the entering column.  Everything bitwise against the oracle."""
import ctypes

import numpy as np
import pytest

import oracle
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
LA_PERSISTENT, LA_TWO_LAUNCH = 1, 2


def _present_count(n, m):
    ld = (n + 1 + 15) // 16 * 16
    return (max(m + 1, ld // 2) + 255) // 256


def _launched(n, m):
    return (max(m, (n + 1) // 2) + 255) // 256             # vc = n: ceil(vc / 2) pairs hold a non-RHS column


def _counts(L, h):
    out = (ctypes.c_int64 * 8)()
    lp.capi.check(L.mi355x_tab_path_counts(h, out), "path_counts")
    return list(out)


@pytest.fixture
def knobs():
    L = lp.capi.lib()
    yield L
    L.mi355x_tune_set_block(0)


SHAPES = [
    (1000, 4096, 17, 16),       # rows; exactly 64 records, 33 MB stored
    (4096, 1000, 9, 8),         # pairs
    (4096, 2048, 9, 8),         # both
    (4095, 2048, 9, 8),         # odd vc: the RHS shares a pair with a column
    (4097, 2049, 9, 9),         # nothing changes
    (600, 8192, 33, 32),        # the per-wave form at 128 records instead of a record per workgroup
]


@pytest.mark.parametrize("n,m,before,now", SHAPES, ids=["rows-16", "pairs-8", "both-8", "odd-vc-8", "same-9", "rows-32"])
@pytest.mark.parametrize("block", [24, 16])
def test_launched_count_matches_the_oracle(knobs, n, m, before, now, block):
    L = knobs
    assert (_present_count(n, m), _launched(n, m)) == (before, now)
    if block == 16 and (n, m) not in ((1000, 4096), (4095, 2048)):
        pytest.skip("the 16-step form on two shapes only (suite time)")
    seed = lp.synth.seed_for(3, 9100 + before + block)
    L.mi355x_tune_set_block(block if block == 16 else 0)
    h = ctypes.c_void_p()
    lp.capi.check(L.mi355x_tab_create_synthetic(ctypes.byref(h), n, m, seed, 0, -1, 0), "create_synthetic")
    t = lp.Tableau(None, lp.Problem(type="max"), None, None, n + m, m, {}, _handle=h)
    M = t.matrix
    b = t.basis_columns.copy()
    requests = [5, block, 2 * block + 3, 1]               # a short block, a full one, two full ones + a short one, a single pivot
    K = sum(requests)
    st, npiv, trace = oracle.solve(M, b, max_pivots=K, trace_cap=K, omp=True)
    assert (st, npiv) == (oracle.MAX_PIVOTS, K)
    t._touch()
    k = ctypes.c_int64(0)
    done = 0
    for i, q in enumerate(requests):
        lp.capi.check(L.mi355x_tab_solve_async(h, 1, 1024.0, q, 1 if i == 0 else 0), "solve_async")
        rc = L.mi355x_tab_sync(h, ctypes.byref(k))
        done += q
        assert (rc, k.value) == (lp.capi.MI_RUNNING, done)
    c = _counts(L, h)
    assert L.mi355x_tab_block_size(h) == block
    assert c[LA_PERSISTENT] > 0 and c[LA_TWO_LAUNCH] == 0 and L.mi355x_tab_la_lost(h) == 0, c
    assert L.mi355x_tab_la_workgroups(h) == now
    t._touch()
    tr = t.pivot_trace()
    bad = np.where((tr[:K] != trace[:K]).any(axis=1))[0]
    assert not len(bad), "first differing pivots %s: got %s, oracle %s" % (bad[:4], tr[bad[:4]], trace[bad[:4]])
    assert np.array_equal(t.basis_columns, b)
    G = t.matrix
    for r0 in range(0, m + 1, 2048):
        assert np.array_equal(G[r0:r0 + 2048].view(np.int64), M[r0:r0 + 2048].view(np.int64)), r0


def test_lost_exchange_on_the_narrower_launch(hooks_lib):
    """As tests/test_gpu_la_wide.py test_lost_exchange_behind_blocks_of_24, on (1000, 4096): 16 workgroups where
    max(rows, ld / 2) asks for 17.  The last LAUNCHED workgroup gives up right behind its ratio record of step
    6; the sweep and the rollback count the done[] entries of the 16 workgroups that ran; the handle carries on
    on the two-launch look-ahead and ends with the oracle's pivots and bits."""
    L = hooks_lib
    n, m = 1000, 4096
    assert (_present_count(n, m), _launched(n, m)) == (17, 16)
    seed = lp.synth.seed_for(3, 9177)
    M0, b0 = lp.synth.tableau(n, m, seed)
    M, b = M0.copy(), b0.copy()
    K = 60
    st_o, npiv, trace = oracle.solve(M, b, max_pivots=K, trace_cap=K, omp=True)
    assert npiv == K
    try:
        L.mi355x_tune_set_la_max_spins(20000)
        L.mi355x_tune_set_la_fault(-7)
        t = lp.Tableau(None, lp.Problem(type="max"), M0, b0, n + m, m, {})
        k = ctypes.c_int64(0)
        rc = L.mi355x_tab_solve(t._h, 1, 1024.0, K, ctypes.byref(k))
        t._touch()
    finally:
        L.mi355x_tune_set_la_max_spins(0)
        L.mi355x_tune_set_la_fault(0)
    assert (rc, k.value) == (st_o, npiv)
    assert L.mi355x_tab_la_lost(t._h) == 1 and L.mi355x_tab_la_workgroups(t._h) == 16
    c = _counts(L, t._h)
    assert c[LA_PERSISTENT] > 0 and c[LA_TWO_LAUNCH] > 0 and c[4] > 0, c          # (c[4]: wide sweeps)
    assert np.array_equal(t.pivot_trace()[:npiv], trace[:npiv])
    assert np.array_equal(t.matrix.view(np.int64), M.view(np.int64))
    assert np.array_equal(t.basis_columns, b)


def _nonfinite_objective_case():
    """Column 5 enters first (finite, -1.5e308); the pivot row's entry of column 7 is negative, so column 7's
    objective entry (-1e308) overflows to -inf under that pivot and column 7 enters second: its objective-row
    entry, col_1[m], is not finite."""
    rng = np.random.default_rng(11)
    m, n = 6, 12
    A = rng.uniform(0.5, 2.0, (m, n))
    A[:, 7] = -rng.uniform(1.0, 2.0, m)
    A[2, 7] = 1.0                                          # (column 7 is not unbounded)
    c = rng.uniform(0.5, 1.0, n)
    c[5], c[7] = -1.5e308, -1.0e308
    M = np.zeros((m + 1, n + m + 1))
    M[:m, :n] = A
    M[np.arange(m), n + np.arange(m)] = 1.0
    M[:m, -1] = rng.uniform(1.0, 2.0, m)
    M[m, :n] = c
    return M, np.arange(n, n + m, dtype=np.int64)


def test_nonfinite_objective_entry_of_the_entering_column():
    """The entry nobody chains any more: the non-finite test on col_J[m] is made on the pricing winner's key,
    by every wave alike, and sends the solve to the dense tableau in the same step (kNeedDense) -- the oracle's
    status, pivots, NaN pattern and bits, as tests/test_gpu_nan_rules.py asks of every path."""
    L = lp.capi.lib()
    M0, b0 = _nonfinite_objective_case()
    M, b = M0.copy(), b0.copy()
    cap = 20
    with np.errstate(all="ignore"):
        st_o, npiv, trace = oracle.solve(M, b, is_max=True, max_pivots=cap, trace_cap=cap)
    assert npiv >= 2 and trace[0][0] == 5 and trace[1][0] == 7
    cr0 = int(trace[0][1])
    with np.errstate(all="ignore"):
        assert M0[-1, 7] - M0[-1, 5] * (M0[cr0, 7] / M0[cr0, 5]) == -np.inf      # col_1[m], as the oracle forms it
    assert not np.isfinite(M).all()
    try:
        L.mi355x_tune_set_lookahead_mode(2)               # the persistent look-ahead whatever the size (default here: resident)
        t = lp.Tableau(None, lp.Problem(type="max"), M0, b0, M0.shape[1] - 1, M0.shape[0] - 1, {})
        k = ctypes.c_int64(0)
        rc = L.mi355x_tab_solve(t._h, 1, 1024.0, cap, ctypes.byref(k))
    finally:
        L.mi355x_tune_set_lookahead_mode(0)
    c = _counts(L, t._h)
    t._touch()
    got = t.pivot_trace()
    assert (rc, k.value) == (st_o, npiv), (rc, k.value, st_o, npiv, got.tolist(), trace.tolist())
    assert c[LA_PERSISTENT] > 0, c
    assert np.array_equal(got, trace)
    G = t.matrix
    nan_o, nan_g = np.isnan(M), np.isnan(G)
    assert np.array_equal(nan_o, nan_g)
    assert np.array_equal(G[~nan_g].view(np.int64), M[~nan_o].view(np.int64))
    assert np.array_equal(t.basis_columns, b)
