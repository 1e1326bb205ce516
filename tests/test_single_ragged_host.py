"""Host-side checks of the ragged single-float batch (mi355x_sbatch_create_ragged, `mixed_shapes`): that the mixed
lists of tests/single_ragged_cases.py exercise what they claim, the new symbols, the argument errors that need no
device, and the routing of members -- everything that needs no GPU.  On the parent commit the tests of the symbols,
the keyword, from_ragged and the routing fail: none of them exists."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_ragged_cases as rc
from tests.helpers import lp_amd
from tests.test_capi_symbols import HEADER, TUNE_HEADER, declared_functions

lp = lp_amd()
capi = lp.capi
F32 = np.float32


# ------------------------------------------------------------------ the inputs exercise what they claim
def test_the_four_bands_have_the_stated_lds_bytes():
    for (m, n), want in rc.BANDS:
        assert lp.single.single_lds_bytes(m + 1, n + m + 1) == want, (m, n)
    assert all(want <= lp.single.LDS_BUDGET for _, want in rc.BANDS)
    assert lp.single.single_lds_bytes(98, 398) <= lp.single.LDS_BUDGET < lp.single.single_lds_bytes(99, 399)


def test_mixed_members_differ_from_their_neighbours_and_finish_at_different_times():
    ins, wants = rc.mixed()
    shapes = [M.shape for M, _, _ in ins]
    assert sorted(set(shapes)) == sorted((m + 1, n + m + 1) for (m, n), _ in rc.BANDS)
    assert all(shapes[k] != shapes[k + 1] and ins[k][2] != ins[k + 1][2] for k in range(len(ins) - 1))
    assert {(s, is_max) for s, (_, _, is_max) in zip(shapes, ins)} == {(s, x) for s in shapes for x in (True, False)}
    counts = [len(w[1]) for w in wants]
    assert all(w[0] == sc.OPTIMAL for w in wants) and len(set(counts)) >= 5, counts
    assert 5 <= min(counts) and 20 * max(counts) < rc.CAP, counts


def test_small_cycle_has_every_column_residue_and_different_basis_lengths():
    ins, wants = rc.small_cycle()
    assert len(ins) == 1100
    assert {M.shape[1] % 4 for M, _, _ in ins[:4]} == {0, 1, 2, 3}
    assert [len(b) for _, b, _ in ins[:4]] == [5, 6, 3, 1]
    assert {x for _, _, x in ins} == {True, False}
    assert {(M.shape, x) for M, _, x in ins} == {(M.shape, x) for M, _, _ in ins[:4] for x in (True, False)}
    counts = {len(w[1]) for w in wants}
    assert all(w[0] == sc.OPTIMAL for w in wants) and len(counts) > 5 and max(counts) <= 20, counts


def test_outcome_members_have_the_outcomes():
    ins, wants = rc.outcome_members()
    got = [(w[0], len(w[1])) for w in wants]
    assert got[1] == (sc.UNBOUNDED, 0) and got[4] == (sc.OPTIMAL, 0) and np.isnan(ins[4][0][-1, 0])
    assert [got[k] for k in (2, 5, 7)] == [(sc.MAX_PIVOTS, rc.OUTCOME_CAP)] * 3
    assert all(got[k][0] == sc.OPTIMAL and 1 <= got[k][1] < rc.OUTCOME_CAP for k in (0, 3, 6)), got


def test_pairs_have_every_outcome_and_different_shapes():
    members, wants = rc.pairs()
    assert [w["status"] for w in wants] == [sc.OPTIMAL, sc.OPTIMAL, sc.INFEASIBLE, sc.OPTIMAL, sc.OPTIMAL, sc.UNBOUNDED,
                                            sc.ART_NONZERO]
    solved_art = sc.solve(members[0][0], members[0][1], False)
    assert len(wants[0]["art_trace"]) - len(solved_art[1]) == 1         # a drive-out pivot: an artificial still basic
    assert [p[0].shape[0] for p in members] == [3, 4, 3, 3, 5, 3, 3]
    assert all(p[0].shape[0] == p[2].shape[0] and p[0].shape[1] > p[2].shape[1] for p in members)
    assert [p[4] for p in members].count(False) == 1 and wants[1]["n2"] >= 1 and wants[4]["n1"] >= 1


# ------------------------------------------------------------------ symbols and argument errors
def test_new_symbols_are_declared_exported_and_bound():
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("mi355x_sbatch_create_ragged", "mi355x_sbatch_member_shape"):
        assert name in declared_functions(HEADER) and name in capi.SIGNATURES and hasattr(L, name), name
    name = "mi355x_tune_set_sbatch_ragged_classes"
    assert name in declared_functions(TUNE_HEADER) and name in capi._EXTRA and hasattr(L, name)
    assert capi.lib().mi355x_abi_version() == 1


def test_bad_arguments_come_before_the_device_check():
    L = capi.lib()
    M = np.zeros(2 * 3 * 4, dtype=F32)
    b = np.zeros(4, dtype=np.int64)
    rows, cols = np.array([3, 3], dtype=np.int64), np.array([4, 4], dtype=np.int64)
    sense = np.array([1, 0], dtype=np.int32)
    h = ctypes.c_void_p()

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def create(out=ctypes.byref(h), n=2, r=rows, c=cols, s=sense, m=M, bb=b, device=0):
        return L.mi355x_sbatch_create_ragged(out, n, p(r) if r is not None else None, p(c) if c is not None else None,
                                             p(s) if s is not None else None, p(m) if m is not None else None,
                                             p(bb) if bb is not None else None, device)
    bad = [dict(out=None), dict(r=None), dict(c=None), dict(m=None), dict(bb=None), dict(n=0), dict(n=(1 << 30) + 1)]
    for r, c in (((3, 0), (4, 4)), ((3, 3), (4, 1)), ((3, 65535 * 16 + 1), (4, 4)), ((3, 3), (4, (1 << 30) + 1))):
        bad.append(dict(r=np.array(r, dtype=np.int64), c=np.array(c, dtype=np.int64)))
    for kw in bad:
        assert create(**kw) == capi.MI_BAD_ARG, kw
        assert not h.value
    assert L.mi355x_sbatch_member_shape(None, 0, None, None, None, None, None) == capi.MI_BAD_ARG
    for bad_count in (2, 3, 5, -1):
        assert L.mi355x_tune_set_sbatch_ragged_classes(bad_count) == capi.MI_BAD_ARG
    for ok in (1, 4, 0):
        assert L.mi355x_tune_set_sbatch_ragged_classes(ok) == capi.MI_OK
    if capi.device_count() == 0:
        assert create() == capi.MI_NO_DEVICE and not h.value
        assert create(s=None) == capi.MI_NO_DEVICE                       # (no senses: every member min)


def test_from_ragged_checks_its_arrays_before_any_device():
    Ms = [np.zeros((3, 4), dtype=F32), np.zeros((2, 5), dtype=F32)]
    bs = [np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.int64)]
    f = lp.SingleBatch.from_ragged
    with pytest.raises(ValueError, match="at least one member"):
        f([], [], [])
    with pytest.raises(ValueError, match="1 bases for 2 matrices"):
        f(Ms, bs[:1], [True, False])
    with pytest.raises(ValueError, match="3 senses for 2 matrices"):
        f(Ms, bs, [True, False, True])
    with pytest.raises(TypeError, match=r"float32 matrices, not float64 \(member 1\)"):
        f([Ms[0], Ms[1].astype(np.float64)], bs, [True, False])
    with pytest.raises(ValueError, match="member 1 must be"):
        f([Ms[0], np.zeros((2, 1), dtype=F32)], bs, [True, False])
    with pytest.raises(ValueError, match="member 0 must be"):
        f([np.zeros((2, 3, 4), dtype=F32), Ms[1]], bs, [True, False])
    with pytest.raises(ValueError, match="member 1: basis shape"):
        f(Ms, [bs[0], np.zeros(2, dtype=np.int64)], None)


def _max2(c, rhs):
    return lp.Problem(type="max", vars=["x", "y"], objective_var="z", objective_func=[("x", c[0]), ("y", c[1])],
                      constraints=[("<=", [("x", 1), ("y", 2)], rhs[0]), ("<=", [("x", 3), ("y", 1)], rhs[1])])


def test_mixed_shapes_needs_single_precision():
    ps = [_max2((1, F32(0.5)), (4, F32(6.5)))]
    for kw in ({}, {"precision": "double"}, {"exact": True}):
        with pytest.raises(ValueError, match="mixed_shapes=True needs precision=\"single\""):
            lp.solve_problems(ps, mixed_shapes=True, **kw)
    with pytest.raises(ValueError, match="mixed_shapes"):
        lp.mi355x_solve_problems(ps, mixed_shapes=True)


# ------------------------------------------------------------------ routing, with the device calls replaced
class _FakeBatch:
    """Reports every member optimal without a pivot and hands its input back."""
    made = []

    def __init__(self, Ms, bs, kind):
        self.Ms, self.bs, self.n_lps, self.ragged = Ms, bs, len(Ms), kind == "ragged"
        self.rows, self.cols = max((M.shape for M in Ms), key=lambda s: s[0] * s[1])

    @staticmethod
    def from_ragged(matrices, bases, is_max, device=0):
        _FakeBatch.made.append(("ragged", [np.asarray(M).shape for M in matrices], None if is_max is None else list(is_max)))
        return _FakeBatch([np.asarray(M) for M in matrices], [np.asarray(b) for b in bases], "ragged")

    @staticmethod
    def from_arrays(matrices, basis, device=0, form="lds"):
        M = np.asarray(matrices)
        if form == "lds" and lp.single.single_lds_bytes(*M.shape[1:]) > lp.single.LDS_BUDGET:
            raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create")
        _FakeBatch.made.append((form, [M.shape[1:]] * len(M), None))
        return _FakeBatch(list(M), list(np.asarray(basis)), form)

    def solve(self, is_max, fp_tolerance=1024, max_pivots=0):
        assert self.ragged == (is_max == -1)
        return np.zeros(self.n_lps, dtype=np.int32), np.zeros(self.n_lps, dtype=np.int64)

    def solve_two_phase(self, main, is_max, fp_tolerance=1024, max_pivots=0):
        assert self.ragged and main.ragged and is_max == -1
        return np.zeros(self.n_lps, dtype=np.int32), np.zeros((self.n_lps, 2), dtype=np.int64)

    def download(self, q):
        return self.Ms[q].copy(), self.bs[q].copy()

    def close(self):
        pass


def _problem_of(M0, n, m, kind="max"):
    names = ["x%d" % j for j in range(n)]
    return lp.Problem(type=kind, vars=names, objective_var="z",
                      objective_func=[(names[j], F32(-M0[m, j])) for j in range(n)],
                      constraints=[("<=", [(names[j], M0[i, j]) for j in range(n)], M0[i, n + m]) for i in range(m)])


def _two_phase_problem(k):
    return lp.Problem(type="max", vars=["x", "y"], objective_var="z", objective_func=[("x", 1), ("y", F32(0.5))],
                      constraints=[("<=", [("x", 1), ("y", 1)], F32(3.5))] * k + [(">=", [("x", 1)], F32(0.5))])


def test_mixed_shapes_routes_all_fitting_members_into_one_batch_and_one_pair(monkeypatch):
    ps = [_problem_of(sc.synthetic(7, 5, seed=1)[0], 7, 5), _two_phase_problem(1),
          _problem_of(sc.synthetic(300, 98, seed=1)[0], 300, 98), _problem_of(sc.synthetic(9, 6, seed=2)[0], 9, 6, "min"),
          _two_phase_problem(2), _problem_of(sc.synthetic(7, 5, seed=3)[0], 7, 5),
          lp.Problem(type="max", vars=["x", "y"], objective_var="z", objective_func=[("x", 1), ("y", 1)],
                     constraints=[("<=", [("x", 1), ("y", 2)], 4)], integer_vars=["x"])]
    alone = []
    monkeypatch.setattr(lp.single.SingleBatch, "from_ragged", _FakeBatch.from_ragged)
    monkeypatch.setattr(lp.single.SingleBatch, "from_arrays", _FakeBatch.from_arrays)
    monkeypatch.setattr(lp.single, "solve_single", lambda p, **kw: alone.append(p) or "alone")

    def run(**kw):
        del _FakeBatch.made[:], alone[:]
        got = lp.single.solve_problems_single(ps, **kw)
        return list(_FakeBatch.made), [k for p in alone for k in range(len(ps)) if ps[k] is p], got

    made, went_alone, got = run(mixed_shapes=True)
    assert made == [("ragged", [(6, 13), (7, 16), (6, 13)], [True, False, True]),
                    ("ragged", [(3, 5), (4, 6)], [True, True]), ("ragged", [(3, 6), (4, 7)], None)]
    assert went_alone == [6, 2] and [g == "alone" for g in got] == [False, False, True, False, False, False, True]
    assert all(isinstance(got[k], lp.SingleTableau) for k in (0, 1, 3, 4, 5))
    assert [got[k].matrix.shape for k in (0, 1, 3, 4, 5)] == [(6, 13), (3, 5), (7, 16), (4, 6), (6, 13)]
    # without the keyword: the one group of two is a batch of one shape, everything else goes alone
    made, went_alone, got = run()
    assert made == [("lds", [(6, 13)] * 2, None)] and len(went_alone) == 5
    # a lone fitting member gains nothing from a batch of one
    del _FakeBatch.made[:], alone[:]
    lp.single.solve_problems_single(ps[:3], mixed_shapes=True)
    assert _FakeBatch.made == [] and len(alone) == 3
    # groups the rule keeps as batches of one shape stay out of the ragged batch
    monkeypatch.setattr(lp.single, "RAGGED_UNIFORM_MIN_MEMBERS", 2)
    made, went_alone, got = run(mixed_shapes=True)
    assert ("lds", [(6, 13)] * 2, None) in made and ("ragged", [(3, 5), (4, 6)], [True, True]) in made
    assert sorted(went_alone) == [2, 3, 6]
