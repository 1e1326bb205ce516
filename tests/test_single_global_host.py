"""Host-side checks of the global form of the single-float batch (mi355x_sbatch_create_global, `beyond_lds`): the new
symbols, the order of the argument checks, the keyword's argument error, the member-count rule and the routing of
groups -- everything that needs no GPU.  On the parent commit every test here fails: the symbols, the keyword and
global_batch_min_members do not exist."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests.helpers import lp_amd
from tests.test_capi_symbols import HEADER, TUNE_HEADER, declared_functions

lp = lp_amd()
capi = lp.capi
F32 = np.float32


def test_new_symbols_are_declared_exported_and_bound():
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("mi355x_sbatch_create_global", "mi355x_sbatch_form"):
        assert name in declared_functions(HEADER) and name in capi.SIGNATURES and hasattr(L, name), name
    name = "mi355x_tune_set_sbatch_global_threads"
    assert name in declared_functions(TUNE_HEADER) and name in capi._EXTRA and hasattr(L, name)
    assert capi.SIGNATURES["mi355x_sbatch_create_global"] == capi.SIGNATURES["mi355x_sbatch_create"]
    assert capi.lib().mi355x_abi_version() == 1


def test_bad_arguments_come_before_the_device_check():
    """MI_BAD_ARG before MI_NO_DEVICE, as for mi355x_sbatch_create: the argument checks need no device."""
    L = capi.lib()
    M = np.zeros((2, 3, 4), dtype=F32)
    b = np.zeros((2, 2), dtype=np.int64)
    h = ctypes.c_void_p()
    mp, bp = M.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 2, 3, 4, mp, bp, 0), (ctypes.byref(h), 2, 3, 4, None, bp, 0), (ctypes.byref(h), 2, 3, 4, mp, None, 0),
                 (ctypes.byref(h), 0, 3, 4, mp, bp, 0), (ctypes.byref(h), 2, 0, 4, mp, bp, 0),
                 (ctypes.byref(h), 2, 3, 0, mp, bp, 0), (ctypes.byref(h), 2, 65535 * 16 + 1, 4, mp, bp, 0),
                 (ctypes.byref(h), 2, 3, (1 << 30) + 1, mp, bp, 0)):
        assert L.mi355x_sbatch_create_global(*args) == capi.MI_BAD_ARG, args[1:4]
        assert L.mi355x_sbatch_create(*args) == capi.MI_BAD_ARG, args[1:4]
        assert not h.value
    assert L.mi355x_sbatch_form(None, None) == capi.MI_BAD_ARG
    assert L.mi355x_tune_set_sbatch_global_threads(512) == capi.MI_BAD_ARG
    for ok in (256, 1024, 0):
        assert L.mi355x_tune_set_sbatch_global_threads(ok) == capi.MI_OK
    if capi.device_count() == 0:
        assert L.mi355x_sbatch_create_global(ctypes.byref(h), 2, 3, 4, mp, bp, 0) == capi.MI_NO_DEVICE and not h.value
        assert L.mi355x_sbatch_create_global(ctypes.byref(h), 2, 3, 4, mp, bp, -1) == capi.MI_NO_DEVICE


def test_from_arrays_declines_an_unknown_form():
    with pytest.raises(ValueError, match="form"):
        lp.SingleBatch.from_arrays(np.zeros((1, 2, 3), dtype=F32), np.zeros((1, 1), dtype=np.int64), form="hbm")


def _max2(c, rhs):
    return lp.Problem(type="max", vars=["x", "y"], objective_var="z", objective_func=[("x", c[0]), ("y", c[1])],
                      constraints=[("<=", [("x", 1), ("y", 2)], rhs[0]), ("<=", [("x", 3), ("y", 1)], rhs[1])])


def test_beyond_lds_needs_single_precision():
    ps = [_max2((1, F32(0.5)), (4, F32(6.5)))]
    for kw in ({}, {"precision": "double"}, {"exact": True}):
        with pytest.raises(ValueError, match="beyond_lds"):
            lp.solve_problems(ps, beyond_lds=True, **kw)
    with pytest.raises(ValueError, match="beyond_lds"):
        lp.mi355x_solve_problems(ps, beyond_lds=True)


def test_min_members_grow_with_the_stored_bytes():
    f = lp.single.global_batch_min_members
    shapes = [(99, 399), (131, 1161), (257, 769), (513, 1537), (1101, 1107), (2049, 4097), (8193, 8193), (19000, 19000)]
    stored = [r * ((c + 31) // 32 * 32) * 4 for r, c in shapes]
    assert stored == sorted(stored)
    counts = [f(r, c) for r, c in shapes]
    assert counts == sorted(counts) and counts[0] >= 2, counts
    assert f(257, 769) == f(257, 800)                        # the stored row, padding included, decides
    try:
        lp.single.GLOBAL_BATCH_MIN_MEMBERS = 5
        assert [f(r, c) for r, c in shapes] == [5] * len(shapes)
    finally:
        lp.single.GLOBAL_BATCH_MIN_MEMBERS = None
    assert [f(r, c) for r, c in shapes] == counts


class _FakeBatch:
    """A batch that declines what the LDS form declines (stored tableau + pivot row + column snapshot beyond 156 KiB)
    and otherwise reports every member optimal without a pivot."""
    made = []

    def __init__(self, M, b, form):
        self.M, self.b, self.form = M, b, form
        self.n_lps, self.rows, self.cols = M.shape

    @staticmethod
    def from_arrays(matrices, basis, device=0, form="lds"):
        M = np.asarray(matrices)
        n, rows, cols = M.shape
        ldl, rp = (cols + 3) // 4 * 4, (rows + 3) // 4 * 4
        if form == "lds" and 4 * (rows * ldl + ldl + rp) > 156 * 1024:
            raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create")
        _FakeBatch.made.append((form, n, rows, cols))
        return _FakeBatch(M, np.asarray(basis), form)

    def solve(self, is_max, fp_tolerance=1024, max_pivots=0):
        return np.zeros(self.n_lps, dtype=np.int32), np.zeros(self.n_lps, dtype=np.int64)

    def download(self, q):
        return self.M[q].copy(), self.b[q].copy()

    def close(self):
        pass


def _problem_of(M0, n, m):
    names = ["x%d" % j for j in range(n)]
    return lp.Problem(type="max", vars=names, objective_var="z",
                      objective_func=[(names[j], F32(-M0[m, j])) for j in range(n)],
                      constraints=[("<=", [(names[j], M0[i, j]) for j in range(n)], M0[i, n + m]) for i in range(m)])


def test_grouping_leaves_lds_sized_groups_on_the_lds_route(monkeypatch):
    """The routing of solve_problems_single with the device calls replaced: a group the LDS form takes is made as an
    LDS batch whether or not the keyword is given; a group beyond the budget goes to the global form only with the
    keyword and with enough members, else one by one."""
    small =[_problem_of(sc.synthetic(40, 24, seed=s)[0], 40, 24) for s in (1, 2)]
    big = [_problem_of(sc.synthetic(300, 98, seed=s)[0], 300, 98) for s in (1, 2, 3)]
    ps = [big[0], small[0], big[1], small[1], big[2]]
    alone = []
    monkeypatch.setattr(lp.single.SingleBatch, "from_arrays", _FakeBatch.from_arrays)
    monkeypatch.setattr(lp.single, "solve_single", lambda p, **kw: alone.append(p) or "alone")
    monkeypatch.setattr(lp.single, "GLOBAL_BATCH_MIN_MEMBERS", 3)

    def run(**kw):
        del _FakeBatch.made[:], alone[:]
        got = lp.single.solve_problems_single(ps, **kw)
        return list(_FakeBatch.made), len(alone), got

    made, n_alone, got = run()
    assert made == [("lds", 2, 25, 65)] and n_alone == 3 and [g == "alone" for g in got] == [True, False, True, False, True]
    made, n_alone, got = run(beyond_lds=True)
    assert sorted(made) == [("global", 3, 99, 399), ("lds", 2, 25, 65)] and n_alone == 0
    assert all(isinstance(g, lp.SingleTableau) for g in got)
    monkeypatch.setattr(lp.single, "GLOBAL_BATCH_MIN_MEMBERS", 4)
    made, n_alone, got = run(beyond_lds=True)
    assert made == [("lds", 2, 25, 65)] and n_alone == 3
