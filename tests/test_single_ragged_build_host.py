"""Host-side checks of the ragged single-float batches built on the device (mi355x_sbatch_create_lps_ragged,
_create_nodes_ragged, _readback_ragged; `mixed_shapes` on the from-rows and branch-and-bound routes): that the lists
of tests/single_ragged_build_cases.py are what they claim, the new symbols and their signatures, the argument errors
that need no device, and the routing with the create calls replaced.  Nothing here needs a GPU.  On the parent commit
the tests of the symbols, the keywords and the routing fail: none of them exists."""
import ctypes

import numpy as np
import pytest

from tests import single_bb_cases as B
from tests import single_cases as sc
from tests import single_lps_cases as C
from tests import single_ragged_build_cases as R
from tests.helpers import lp_amd
from tests.test_capi_symbols import HEADER, declared_functions

lp = lp_amd()
capi = lp.capi
F32 = np.float32


# ------------------------------------------------------------------ the lists are what they claim
def test_the_lists_have_distinct_shapes_both_senses_and_fit():
    for name in ("sweep_single", "sweep_two_phase"):
        ds = getattr(R, name)()
        shapes = [R.shape_of(d) for d in ds]
        assert len(ds) == 15 and len(set(shapes)) == 15 and set(shapes) == {(m, n) for m in R.SWEEP_M for n in R.SWEEP_NCV}
        assert [d["type"] for d in ds[:4]] in (["min", "max"] * 2, ["max", "min"] * 2)
    for name in ("sweep_single", "ld_steps_main", "tall_members", "outcome_single"):
        assert all(sc.build(d)["art"] is None for d in getattr(R, name)()), name
    for name in ("sweep_two_phase", "ld_steps_art", "outcome_pair"):
        ds = getattr(R, name)()
        assert all(sc.build(d)["art"] is not None for d in ds), name
        assert len({R.counts_of(d)[1] for d in ds}) >= 2, name             # n_art differs inside the pair
    for name in ("sweep_single", "sweep_two_phase", "ld_steps_main", "ld_steps_art", "tall_members", "outcome_pair",
                 "outcome_single"):
        for d in getattr(R, name)():
            b = sc.build(d)
            assert C.fits(*(b["art"] or b["main"])[0].shape), name
    assert [R.main_cols(d) for d in R.ld_steps_main()] == [31, 32, 33, 64, 65]
    # the artificial columns cross a 32-float step where the main columns do not
    assert [(R.main_cols(d), R.art_cols(d)) for d in R.ld_steps_art()] == [(30, 31), (30, 32), (30, 33), (30, 34)]
    ms = [R.shape_of(d)[0] for d in R.tall_members()]
    assert set(R.TALL_M) < set(ms) and 1 in ms and min(ms) < 64 < 65 <= max(ms) and any(m > 128 for m in ms)
    assert C.fits(197, 198) and not C.fits(198, 199)
    assert {d["type"] for d in R.tall_members()} == {"max", "min"}


def test_the_solved_lists_have_the_outcomes():
    got = [R.solution("outcome_pair", q)["status"] for q in range(len(R.outcome_pair()))]
    assert got[:4] == [sc.INFEASIBLE, sc.OPTIMAL, sc.UNBOUNDED, sc.ART_NONZERO] and got[4:] == [sc.OPTIMAL] * 7
    w = R.solution("outcome_pair", 4)
    assert len(w["art_trace"]) - len(sc.solve(w["build"]["art"][0], w["build"]["art"][1], False)[1]) == 1      # a drive-out pivot
    single = [R.solution("outcome_single", q) for q in range(len(R.outcome_single()))]
    assert [s["status"] for s in single].count(sc.UNBOUNDED) == 1 and max(s["n"][0] for s in single) > 3
    assert any(sum(R.solution("sweep_two_phase", q)["n"]) >= 3 for q in range(15))
    assert all(sum(R.solution(name, q)["n"]) < R.CAP // 4 for name in R.SOLVED_LISTS for q in range(len(getattr(R, name)())))


def test_the_node_lists_mix_depths_and_artificial_counts():
    for art_base, want_art in ((False, False), (False, True), (True, False)):
        base, entries = R.node_base(art_base), R.node_entries(want_art)
        assert sorted({len(e) for e in entries}) == list(R.DEPTHS) and R.free_variable_rows(entries)
        built = [B.build_node(base, e) for e in entries]
        assert all((b[2] is not None) == (art_base or want_art) for b in built)
        if want_art:
            assert len({b[2].shape[1] - b[0].shape[1] for b in built}) >= 2
        assert all(C.fits(*(b[2] if b[2] is not None else b[0]).shape) for b in built)


def test_the_searches_have_rounds_of_mixed_depths_at_width_four():
    for seed, shape in R.SEARCH_MIXED_TWO:
        R.search_problem(seed, shape)
        sets = R.round_depth_sets(seed, shape, 4)
        assert any(len(set(two)) >= 2 for _, two in sets), (seed, shape, sets)
        assert any(len(one) + len(two) >= 3 for one, two in sets)
        # the single-phase nodes of a round: one path of the tree, never two of them in a round
        assert all(len(one) <= 1 for one, _ in sets), (seed, shape, sets)


# ------------------------------------------------------------------ symbols and argument errors
NEW = {"mi355x_sbatch_create_lps_ragged": 10, "mi355x_sbatch_create_nodes_ragged": 8, "mi355x_sbatch_readback_ragged": 4,
       "mi355x_sbb_base_set_sense": 2}


def test_new_symbols_are_declared_exported_and_bound():
    L = ctypes.CDLL(capi.LIB_PATH)
    for name, n_args in NEW.items():
        assert name in declared_functions(HEADER) and name in capi.SIGNATURES and hasattr(L, name), name
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args, name
    assert capi.SIGNATURES["mi355x_sbatch_create_lps_ragged"][1][-1] is ctypes.c_int
    assert capi.SIGNATURES["mi355x_sbatch_create_nodes_ragged"][1][3] is ctypes.c_int64
    assert capi.lib().mi355x_abi_version() == 1


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_come_before_the_device_check():
    L = capi.lib()
    m, ncv = np.array([2, 1], dtype=np.int64), np.array([2, 3], dtype=np.int64)
    is_max = np.array([1, 0], dtype=np.int32)
    lps = np.ones(3 * 3 + 2 * 4, dtype=F32)
    sense = np.zeros(3, dtype=np.int32)
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()

    def create(out=True, n=2, m=m, ncv=ncv, is_max=is_max, lps=lps, sense=sense):
        return L.mi355x_sbatch_create_lps_ragged(ctypes.byref(hm) if out else None, ctypes.byref(ha), n, _p(m), _p(ncv),
                                                 _p(is_max), _p(lps), _p(sense), None, 0)
    bad = [dict(out=False), dict(m=None), dict(ncv=None), dict(is_max=None), dict(lps=None), dict(sense=None), dict(n=0),
           dict(m=np.array([2, 0], dtype=np.int64)), dict(ncv=np.array([0, 3], dtype=np.int64)),
           dict(sense=np.array([0, 3, 0], dtype=np.int32)),
           dict(sense=np.array([0, 0, 1], dtype=np.int32)), dict(sense=np.array([2, 0, 0], dtype=np.int32))]   # mixtures
    for kw in bad:
        assert create(**kw) == capi.MI_BAD_ARG, kw
        assert not hm.value and not ha.value
    create(sense=np.array([0, 0, 1], dtype=np.int32))
    assert b"member 1" in L.mi355x_last_error()
    assert L.mi355x_sbatch_create_nodes_ragged(ctypes.byref(hm), ctypes.byref(ha), None, 1, None, None, None, None) == capi.MI_BAD_ARG
    assert L.mi355x_sbatch_readback_ragged(None, None, None, None) == capi.MI_BAD_ARG
    assert L.mi355x_sbb_base_set_sense(None, 1) == capi.MI_BAD_ARG
    if capi.device_count() == 0:
        assert create() == capi.MI_NO_DEVICE and not hm.value
    # the declines that need no device either: the guard and the budget, the member named
    sums = np.zeros(7, dtype=np.float64)
    sums[5] = 2.0 ** 24 + 2
    assert L.mi355x_sbatch_create_lps_ragged(ctypes.byref(hm), ctypes.byref(ha), 2, _p(m), _p(ncv), _p(is_max), _p(lps),
                                             _p(sense), _p(sums), 0) == capi.MI_UNSUPPORTED
    assert b"member 1" in L.mi355x_last_error()


def test_from_lps_ragged_checks_its_arrays_before_any_device():
    f = lp.SingleBatch.from_lps_ragged
    Ls, ss = [np.ones((3, 3), dtype=F32), np.ones((2, 4), dtype=F32)], [np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32)]
    with pytest.raises(ValueError, match="at least one member"):
        f([], [], [])
    with pytest.raises(ValueError, match="1 sense arrays for 2 members"):
        f(Ls, ss[:1], [True, False])
    with pytest.raises(ValueError, match="3 senses for 2 members"):
        f(Ls, ss, [True, False, True])
    with pytest.raises(TypeError, match=r"float32 rows, not float64 \(member 1\)"):
        f([Ls[0], Ls[1].astype(np.float64)], ss, [True, False])
    with pytest.raises(ValueError, match="member 1: sense shape"):
        f(Ls, [ss[0], np.zeros(3, dtype=np.int32)], [True, False])
    with pytest.raises(ValueError, match="member 0: col_int_sum shape"):
        f(Ls, ss, [True, False], [np.zeros(2), np.zeros(4)])


def test_the_keyword_is_an_argument_error_anywhere_else():
    p = C.to_problem(lp, C.lone_member())
    for kw in ({}, {"precision": "single"}, {"branch_and_bound": True}, {"precision": "single", "branch_and_bound": True}):
        with pytest.raises(ValueError, match="mixed_shapes=True needs precision=\"single\", branch_and_bound=True"):
            lp.mi355x_simplex_solver(p, mixed_shapes=True, **kw)         # (no integer variables: not that route)
    ip = C.to_problem(lp, C.lone_member(), integer_vars=["x0"])
    with pytest.raises(ValueError, match="mixed_shapes=True needs"):
        lp.mi355x_simplex_solver(ip, precision="single", branch_and_bound=True, exact=True, mixed_shapes=True)


# ------------------------------------------------------------------ routing, with the create calls replaced
class _Fake:
    made = []

    def __init__(self, shapes, ragged):
        self.shapes, self.n_lps, self.ragged = shapes, len(shapes), ragged
        self.rows, self.cols = max(shapes, key=lambda s: s[0] * s[1])

    def solve(self, is_max, fp_tolerance=1024, max_pivots=0):
        assert self.ragged == (is_max == -1)
        return np.zeros(self.n_lps, dtype=np.int32), np.zeros(self.n_lps, dtype=np.int64)

    def solve_two_phase(self, main, is_max, fp_tolerance=1024, max_pivots=0):
        assert self.ragged == main.ragged == (is_max == -1)
        return np.zeros(self.n_lps, dtype=np.int32), np.zeros((self.n_lps, 2), dtype=np.int64)

    def download(self, q):
        r, c = self.shapes[q]
        return np.zeros((r, c), dtype=F32), np.arange(r - 1, dtype=np.int64)

    def close(self):
        pass


def _shapes(L, s):
    n_eq, n_art = (int(x) for x in lp.lists.row_counts(L[:-1, -1] < 0, s))
    m, ncv = L.shape[0] - 1, L.shape[1] - 1
    return (m + 1, ncv + m - n_eq + 1), n_art


def _fake_ragged(lps_list, sense_list, is_max, col_int_sum_list=None, device=0):
    shapes = [_shapes(np.asarray(L), np.asarray(s)) for L, s in zip(lps_list, sense_list)]
    _Fake.made.append(("ragged", [s for s, _ in shapes], [bool(x) for x in is_max]))
    main = _Fake([s for s, _ in shapes], True)
    return main, (_Fake([(s[0], s[1] + a) for s, a in shapes], True) if shapes[0][1] else None)


def _fake_lps(lps, sense, col_int_sum=None, device=0, form="lds"):
    shape, n_art = _shapes(np.asarray(lps)[0], np.asarray(sense)[0])
    if form == "lds" and not C.fits(shape[0], shape[1] + n_art):
        raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create_lps")
    _Fake.made.append((form, [shape] * len(lps), None))
    main = _Fake([shape] * len(lps), False)
    return main, (_Fake([(shape[0], shape[1] + n_art)] * len(lps), False) if n_art else None)


def test_mixed_shapes_routes_the_fitting_members_into_one_batch_and_one_pair(monkeypatch):
    one, two = R.sweep_single(), R.sweep_two_phase()
    ds = [one[0], two[0], one[1], C._synthetic_problem(300, 98, 1, False), two[1], one[0], C.float_zero_member(), one[2]]
    ps = [C.to_problem(lp, d) for d in ds] + [C.to_problem(lp, C.lone_member(), integer_vars=["x0"])]
    alone = []
    monkeypatch.setattr(lp.single.SingleBatch, "from_lps_ragged", staticmethod(_fake_ragged))
    monkeypatch.setattr(lp.single.SingleBatch, "from_lps", staticmethod(_fake_lps))
    monkeypatch.setattr(lp.single_lps, "solve_single", lambda p, **kw: alone.append(p) or "alone")

    def run(ps=ps, **kw):
        del _Fake.made[:], alone[:]
        got = lp.single_lps.solve_problems_single_from_rows(ps, **kw)
        return list(_Fake.made), sorted(k for p in alone for k in range(len(ps)) if ps[k] is p), got
    made, went_alone, got = run(mixed_shapes=True)
    s1 = [sc.build(ds[k])["main"][0].shape for k in (0, 2, 5, 7)]
    s2 = [sc.build(ds[k])["main"][0].shape for k in (1, 4)]
    assert made == [("ragged", s1, [ds[k]["type"] == "max" for k in (0, 2, 5, 7)]),
                    ("ragged", s2, [ds[k]["type"] == "max" for k in (1, 4)])]
    assert went_alone == [3, 6, 8]
    assert [got[k].matrix.shape for k in (0, 2, 5, 7)] == s1 and all(got[k] == "alone" for k in (3, 6, 8))
    # without the keyword: the one group of two is a batch of one shape, every other member goes alone
    made, went_alone, _ = run()
    assert made == [("lds", [s1[0]] * 2, None)] and len(went_alone) == 7
    # fewer than two: no ragged create
    made, went_alone, _ = run(ps=ps[:2], mixed_shapes=True)
    assert made == [] and went_alone == [0, 1]
    # groups the rule keeps as batches of one shape stay out of the ragged batch
    monkeypatch.setattr(lp.single, "RAGGED_UNIFORM_MIN_MEMBERS", 2)
    made, went_alone, _ = run(mixed_shapes=True)
    assert ("lds", [s1[0]] * 2, None) in made and ("ragged", [s1[1], s1[3]], [ds[2]["type"] == "max", ds[7]["type"] == "max"]) in made


def test_a_declined_ragged_create_sends_its_members_one_by_one(monkeypatch):
    one = R.sweep_single()
    ps = [C.to_problem(lp, d) for d in one[:3]]
    alone = []

    def declined(*a, **kw):
        raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create_lps_ragged")
    monkeypatch.setattr(lp.single.SingleBatch, "from_lps_ragged", staticmethod(declined))
    monkeypatch.setattr(lp.single_lps, "solve_single", lambda p, **kw: alone.append(p) or "alone")
    assert lp.single_lps.solve_problems_single_from_rows(ps, mixed_shapes=True) == ["alone"] * 3 and len(alone) == 3


def test_device_rounds_take_the_keyword_and_count():
    p = B.to_problem(lp, B.case("le_1")[0])
    assert lp.single_bb.DeviceRounds(p).mixed_shapes is False
    r = lp.single_bb.DeviceRounds(p, mixed_shapes=True)
    assert r.mixed_shapes and r.ragged_batched == 0 and lp.single_bb.RAGGED_NODES_MIN == 2
    s = lp.single_bb.SingleBranchAndBound(p, width=4, mixed_shapes=True)
    assert s.rounds.mixed_shapes
