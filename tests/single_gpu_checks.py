"""The checks tests/test_gpu_single_edges.py and tests/test_gpu_single_thresholds.py share: a case of the float32
model (tests/single_cases.py) through a single-float path of the library, against the model's answer -- status, pivot
count(s), whole trace(s), basis and EVERY entry of the final tableau(x) bit for bit (sc.same_bits: any NaN equals any
NaN), no tolerance anywhere -- and the form that ran, read back from info().  `factor` is the tolerance factor the
model's answer was computed with; it reaches the library the way a caller passes it."""
import numpy as np

from tests import single_cases as sc
from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi
F32 = np.float32
AUTO, PAIR, LDS = 0, 1, 2
same_bits = sc.same_bits


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def tableau(M0, b0, is_max, factor=1024):
    return lp.SingleTableau(None, lp.Problem(type="max" if is_max else "min"), np.array(M0, dtype=F32), np.array(b0),
                            M0.shape[1] - 1, M0.shape[0] - 1, {}, fp_tolerance_factor=factor)


def check_single(case, form, chunk=None, factor=1024):
    """One tableau through lp.single.solve_status in the given form, against the model's answer."""
    M0, b0, is_max, cap, (wst, wtrace, M, b) = case
    lp.single.set_form(form)
    t = tableau(M0, b0, is_max, factor)
    st, n = lp.single.solve_status(t, max_pivots=cap, chunk=chunk)
    assert t.info()["form"] == form
    assert st == wst and n == len(wtrace), (st, n, wst, len(wtrace))
    assert _pairs(t.pivot_trace().tolist()) == wtrace
    assert np.array_equal(t.basis_columns, b)
    assert same_bits(t.matrix, M)


def check_batch(cases, threads, launch_cap, factor=1024):
    """The cases (one shape, one sense, one cap) as the members of one batch."""
    is_max, cap = cases[0][2], cases[0][3]
    assert all(c[2] == is_max and c[3] == cap and c[0].shape == cases[0][0].shape for c in cases)
    lp.single.set_batch_threads(threads)
    lp.single.set_batch_launch_cap(launch_cap)
    sb = lp.SingleBatch.from_arrays(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
    try:
        info = sb.info()
        assert info["workgroup_threads"] == threads and info["n_lps"] == len(cases)
        st, npv = sb.solve(is_max, factor, cap)
        assert sb.last_return == capi.MI_OK
        for q, c in enumerate(cases):
            wst, wtrace, M, b = c[4]
            assert int(st[q]) == wst and int(npv[q]) == len(wtrace), (q, int(st[q]), int(npv[q]), wst, len(wtrace))
            assert _pairs(sb.trace(q).tolist()) == wtrace, q
            G, gb = sb.download(q)
            assert np.array_equal(gb, b), q
            assert same_bits(G, M), q
    finally:
        sb.close()


def check_two_phase_single(pair, want, form, chunk, factor=1024):
    A0, ab0, M0, mb0 = pair
    lp.single.set_form(form)
    art, main = tableau(A0, ab0, False, factor), tableau(M0, mb0, True, factor)
    st, npv = lp.single.solve_status([art, main], max_pivots=2000, chunk=chunk)
    assert art.info()["form"] == form and main.info()["form"] == form
    assert st == want["status"] and npv == (want["n1"], want["n2"]), (st, npv)
    assert _pairs(art.pivot_trace().tolist()) == want["art_trace"]
    assert _pairs(main.pivot_trace().tolist()) == want["main_trace"]
    assert same_bits(art.matrix, want["A"]) and np.array_equal(art.basis_columns, want["abasis"])
    assert same_bits(main.matrix, want["M"]) and np.array_equal(main.basis_columns, want["mbasis"])


def check_two_phase_batch(cases, threads, per_call, factor=1024):
    pairs, wants = [c[0] for c in cases], [c[1] for c in cases]
    lp.single.set_batch_threads(threads)
    ab = lp.SingleBatch.from_arrays(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    mb = lp.SingleBatch.from_arrays(np.stack([p[2] for p in pairs]), np.stack([p[3] for p in pairs]))
    try:
        assert ab.info()["workgroup_threads"] == threads and mb.info()["workgroup_threads"] == threads
        total = np.zeros((len(pairs), 2), dtype=np.int64)
        for _ in range(2000):
            st, npv = ab.solve_two_phase(mb, True, factor, per_call)
            assert ab.last_return == capi.MI_OK
            total += npv
            if not (st == capi.MI_MAX_PIVOTS).any():
                break
        else:
            raise AssertionError("the pair did not finish")
        for q, w in enumerate(wants):
            assert int(st[q]) == w["status"], (q, int(st[q]), w["status"])
            assert total[q].tolist() == [len(w["art_trace"]), w["n2"]], (q, total[q].tolist())
            assert _pairs(ab.trace(q).tolist()) == w["art_trace"], q
            assert _pairs(mb.trace(q).tolist()) == w["main_trace"], q
            A, abasis = ab.download(q)
            M, mbasis = mb.download(q)
            assert same_bits(A, w["A"]) and np.array_equal(abasis, w["abasis"]), q
            assert same_bits(M, w["M"]) and np.array_equal(mbasis, w["mbasis"]), q
    finally:
        ab.close()
        mb.close()
