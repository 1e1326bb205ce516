"""Host-side checks of the device-built single-float batches in the GLOBAL form (mi355x_sbatch_create_lps_global,
mi355x_sbatch_create_nodes_global; `form=` on SingleBatch.from_lps / Base.create_nodes / solve_lps_single,
`beyond_lds` on solve_problems_single_from_rows, the single-float branch-and-bound and mi355x_simplex_solver): the
symbols, the order of the argument checks, the argument errors, the routing of groups with the device calls replaced
by spies, and the array yardstick (single_lps_cases.assemble_rows) pinned against the model at multi-trip shapes --
everything that needs no GPU.  On the parent commit every test here fails: the symbols and keywords do not exist."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_global_build_cases as G
from tests import single_lps_cases as C
from tests.helpers import lp_amd
from tests.test_capi_symbols import HEADER, declared_functions

lp = lp_amd()
capi, sbb = lp.capi, lp.single_bb
F32 = np.float32
NEW = ("mi355x_sbatch_create_lps_global", "mi355x_sbatch_create_nodes_global")


def test_new_symbols_are_declared_exported_and_bound():
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared_functions(HEADER) and name in capi.SIGNATURES and hasattr(L, name), name
    assert capi.SIGNATURES[NEW[0]] == capi.SIGNATURES["mi355x_sbatch_create_lps"]
    assert capi.SIGNATURES[NEW[1]] == capi.SIGNATURES["mi355x_sbatch_create_nodes"]
    assert capi.lib().mi355x_abi_version() == 1


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_come_before_the_device_check():
    """MI_BAD_ARG before MI_NO_DEVICE, in the order of the LDS twins: the argument checks need no device, and no
    handle is left behind."""
    L = capi.lib()
    lps, sense = np.ones((2, 3, 4), dtype=F32), np.zeros((2, 2), dtype=np.int32)
    bad_sense = sense.copy()
    bad_sense[1, 0] = 3
    uneven = sense.copy()
    uneven[1, 1] = 1                                         # member 1 has an artificial row, member 0 none
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    out = (ctypes.byref(hm), ctypes.byref(ha))
    for name in ("mi355x_sbatch_create_lps_global", "mi355x_sbatch_create_lps"):
        f = getattr(L, name)
        for args in ((None, out[1], 2, 2, 3, _p(lps), _p(sense), None, 0), (out[0], None, 2, 2, 3, _p(lps), _p(sense), None, 0),
                     out + (2, 2, 3, None, _p(sense), None, 0), out + (2, 2, 3, _p(lps), None, None, 0),
                     out + (0, 2, 3, _p(lps), _p(sense), None, 0), out + (2, 0, 3, _p(lps), _p(sense), None, 0),
                     out + (2, 2, 0, _p(lps), _p(sense), None, 0), out + (2, 2, 3, _p(lps), _p(bad_sense), None, 0),
                     out + (2, 2, 3, _p(lps), _p(uneven), None, 0)):
            assert f(*args) == capi.MI_BAD_ARG, (name, args[2:5])
            assert not hm.value and not ha.value
    var, bound, s1 = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
    for name in ("mi355x_sbatch_create_nodes_global", "mi355x_sbatch_create_nodes"):
        f = getattr(L, name)
        for args in ((None, out[1], None, 2, 1, _p(var), _p(s1), _p(bound)), out + (None, 2, 1, _p(var), _p(s1), _p(bound))):
            assert f(*args) == capi.MI_BAD_ARG, name
            assert not hm.value and not ha.value
    if capi.device_count() == 0:
        for device in (0, -1):
            rc = L.mi355x_sbatch_create_lps_global(*out, 2, 2, 3, _p(lps), _p(sense), None, device)
            assert rc == capi.MI_NO_DEVICE and not hm.value and not ha.value
        # the integer-sum guard needs no device either: MI_UNSUPPORTED, naming the member
        sums = np.zeros((2, 4), dtype=np.float64)
        sums[1, 2] = 2.0 ** 24 + 2
        assert L.mi355x_sbatch_create_lps_global(*out, 2, 2, 3, _p(lps), _p(sense), _p(sums), 0) == capi.MI_UNSUPPORTED
        assert b"member 1" in L.mi355x_last_error() and not hm.value and not ha.value


def test_unknown_forms_are_argument_errors():
    lps, sense = np.ones((2, 3, 4), dtype=F32), np.zeros((2, 2), dtype=np.int32)
    with pytest.raises(ValueError, match="form"):
        lp.SingleBatch.from_lps(lps, sense, form="hbm")
    with pytest.raises(ValueError, match="form"):
        lp.solve_lps_single(lps, sense, form="hbm")
    base = object.__new__(sbb.Base)                          # (no device: the check comes before anything is touched)
    base.g = base.handle = None
    with pytest.raises(ValueError, match="form"):
        base.create_nodes([(("x", 0, 1),)], form="hbm")


def _ilp(integer=True):
    return lp.Problem(type="max", vars=["x", "y"], objective_var="z", objective_func=[("x", 1), ("y", F32(0.5))],
                      constraints=[("<=", [("x", 1), ("y", 2)], 4), ("<=", [("x", 3), ("y", 1)], F32(6.5))],
                      integer_vars=["x"] if integer else [])


@pytest.mark.parametrize("kw,integer", [({}, True), ({"precision": "double"}, True), ({"branch_and_bound": True}, True),
                                        ({"precision": "single"}, False), ({"precision": "single"}, True),
                                        ({"precision": "single", "branch_and_bound": True}, False),
                                        ({"exact": True, "branch_and_bound": True}, True),
                                        ({"precision": "single", "branch_and_bound": True, "devices": 2}, True)])
def test_beyond_lds_on_the_solver_needs_the_single_float_branch_and_bound(kw, integer):
    with pytest.raises(ValueError, match="beyond_lds"):
        lp.mi355x_simplex_solver(_ilp(integer), beyond_lds=True, **kw)
    with pytest.raises(ValueError, match="beyond_lds"):
        lp.solve_problem(_ilp(integer), beyond_lds=True, **kw)


def test_single_float_from_rows_stays_an_argument_error_on_the_public_list_call():
    with pytest.raises(ValueError):
        lp.mi355x_solve_problems([_ilp(False)], precision="single", from_rows=True)


# ------------------------------------------------------------------ routing, the device calls replaced by spies
def _lds_declines(rows, cols):
    ldl, rp = (cols + 3) // 4 * 4, (rows + 3) // 4 * 4
    return 4 * (rows * ldl + ldl + rp) > 156 * 1024


class _FakeBatch:
    """A batch that reports every member optimal without a pivot (status: every member that, for the node routes)."""

    def __init__(self, n, rows, cols, status=0):
        self.n_lps, self.rows, self.cols, self.status = n, rows, cols, status

    def _st(self):
        return np.full(self.n_lps, self.status, dtype=np.int32)

    def solve(self, is_max, fp_tolerance=1024, max_pivots=0):
        return self._st(), np.zeros(self.n_lps, dtype=np.int64)

    def solve_two_phase(self, main, main_is_max, fp_tolerance=1024, max_pivots=0):
        return self._st(), np.zeros((self.n_lps, 2), dtype=np.int64)

    def download(self, q):
        return np.zeros((self.rows, self.cols), dtype=F32), np.arange(self.rows - 1, dtype=np.int64)

    def close(self):
        pass


def _synthetic_problems(n, m, seeds, two_phase=False):
    return [C.to_problem(lp, C._synthetic_problem(n, m, s, two_phase)) for s in seeds]


def test_list_route_takes_the_lds_form_first_and_the_global_form_only_when_asked(monkeypatch):
    """solve_problems_single_from_rows: LDS first; the global form only on MI_UNSUPPORTED, with the keyword and with
    enough members (of the ARTIFICIAL shape for a two-phase group); else one by one."""
    small = _synthetic_problems(40, 24, (1, 2))
    big = _synthetic_problems(300, 98, (1, 2, 3))
    big2 = _synthetic_problems(300, 84, (1, 2), two_phase=True)
    ps = [big[0], small[0], big2[0], big[1], small[1], big[2], big2[1]]
    assert lp.group_lowered_rows_single(ps)[0] == {}
    made, alone, asked = [], [], []

    def from_lps(cls, lps, sense, col_int_sum=None, device=0, form="lds"):
        n, m, ncv = lps.shape[0], lps.shape[1] - 1, lps.shape[2] - 1
        n_eq, n_art = (int(x[0]) for x in lp.lists.row_counts(lps[:1, :-1, -1] < 0, sense[:1]))
        rows, cols = m + 1, ncv + (m - n_eq) + 1
        made.append((form, n, rows, cols + n_art))
        if form == "lds" and _lds_declines(rows, cols + n_art):
            raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create_lps")
        return _FakeBatch(n, rows, cols), (_FakeBatch(n, rows, cols + n_art) if n_art else None)

    def min_members(rows, cols):
        asked.append((rows, cols))
        return hook[0]
    monkeypatch.setattr(lp.SingleBatch, "from_lps", classmethod(from_lps))
    monkeypatch.setattr(lp.single_lps, "solve_single", lambda p, **kw: alone.append(p) or "alone")
    monkeypatch.setattr(lp.single, "global_batch_min_members", min_members)
    hook = [2]

    def run(**kw):
        del made[:], alone[:], asked[:]
        return lp.solve_problems_single_from_rows(ps, **kw)

    got = run()
    assert sorted(made) == [("lds", 2, 25, 65), ("lds", 2, 85, 469), ("lds", 3, 99, 399)] and asked == []
    assert [g == "alone" for g in got] == [True, False, True, True, False, True, True] and len(alone) == 5
    got = run(beyond_lds=True)
    assert sorted(made) == [("global", 2, 85, 469), ("global", 3, 99, 399), ("lds", 2, 25, 65), ("lds", 2, 85, 469),
                            ("lds", 3, 99, 399)]
    assert made.index(("lds", 3, 99, 399)) < made.index(("global", 3, 99, 399))
    assert sorted(asked) == [(85, 469), (99, 399)] and alone == []
    assert all(isinstance(g, lp.SingleTableau) for g in got)
    hook[0] = 3                                              # the pair of two is too small now
    got = run(beyond_lds=True)
    assert sorted(f for f, *_ in made) == ["global", "lds", "lds", "lds"] and len(alone) == 2
    assert [g == "alone" for g in got] == [False, False, True, False, False, False, True]
    hook[0] = 4
    run(beyond_lds=True)
    assert sorted(f for f, *_ in made) == ["lds"] * 3 and len(alone) == 5


def test_the_member_count_hook_reaches_the_list_route(monkeypatch):
    assert lp.single_lps.single.global_batch_min_members is lp.single.global_batch_min_members
    monkeypatch.setattr(lp.single, "GLOBAL_BATCH_MIN_MEMBERS", 7)
    assert lp.single.global_batch_min_members(99, 399) == 7


@pytest.mark.parametrize("guard_fails", [False, True])
def test_node_groups_take_the_lds_form_first_and_the_global_form_only_when_asked(monkeypatch, guard_fails):
    """DeviceRounds: the LDS batches first; the global form only when they decline, with the keyword and with enough
    nodes in the group -- create_nodes(form="global") for the device-built groups, from_arrays(form="global") for
    the host-built ones; else node by node."""
    d = G.big_bb_problem(two_phase=False)
    p = B_to_problem(d)
    calls, alone = [], []

    class FakeBase:
        def __init__(self, g, device=0):
            self.g = g

        def create_nodes(self, entries, form="lds"):
            rows, cols = self.g.matrix.shape[0] + len(entries[0]), self.g.matrix.shape[1] + len(entries[0])
            calls.append(("create_nodes", form, len(entries), rows, cols))
            if form == "lds":
                raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create_nodes")
            return _FakeBatch(len(entries), rows, cols, capi.MI_INFEASIBLE), None

        def close(self):
            pass

    def from_arrays(matrices, basis, device=0, form="lds"):
        n, rows, cols = np.asarray(matrices).shape
        calls.append(("from_arrays", form, n, rows, cols))
        if form == "lds" and _lds_declines(rows, cols):
            raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create")
        return _FakeBatch(n, rows, cols, capi.MI_INFEASIBLE)
    monkeypatch.setattr(sbb, "Base", FakeBase)
    monkeypatch.setattr(lp.SingleBatch, "from_arrays", staticmethod(from_arrays))
    monkeypatch.setattr(sbb, "readback", lambda sb: (None, None, None))
    monkeypatch.setattr(sbb.DeviceRounds, "_alone", lambda self, tabs: alone.append(tabs) or (capi.MI_INFEASIBLE, None, None))
    if guard_fails:
        monkeypatch.setattr(sbb.GeneralFormSingle, "device_ok", lambda self, entry: False)
    monkeypatch.setattr(lp.single, "GLOBAL_BATCH_MIN_MEMBERS", 3)
    entries = [(("x", 0, 2),), (("y", 0, 3),), (("z", 0, 1),), (("x", 0, 1), ("y", 0, 2)), (("x", 0, 0), ("y", 0, 1))]
    route = "from_arrays" if guard_fails else "create_nodes"

    def run(**kw):
        del calls[:], alone[:]
        r = sbb.DeviceRounds(p, **kw)
        out = r(entries)
        assert [o[0] for o in out] == [capi.MI_INFEASIBLE] * 5
        return r
    r = run()
    assert [c[:3] for c in calls] == [(route, "lds", 3), (route, "lds", 2)] and len(alone) == 5
    assert (r.one_by_one, r.global_batched, r.host_built) == (5, 0, 0)
    r = run(beyond_lds=True)
    assert [c[:3] for c in calls] == [(route, "lds", 3), (route, "global", 3), (route, "lds", 2)] and len(alone) == 2
    assert calls[1][3:] == (202, 206)
    assert (r.one_by_one, r.global_batched, r.host_built) == (2, 3, 3 if guard_fails else 0)
    monkeypatch.setattr(lp.single, "GLOBAL_BATCH_MIN_MEMBERS", 2)
    r = run(beyond_lds=True)
    assert [c[:3] for c in calls] == [(route, "lds", 3), (route, "global", 3), (route, "lds", 2), (route, "global", 2)]
    assert (r.one_by_one, r.global_batched, alone) == (0, 5, [])
    monkeypatch.setattr(lp.single, "GLOBAL_BATCH_MIN_MEMBERS", 4)
    r = run(beyond_lds=True)
    assert [c[:3] for c in calls] == [(route, "lds", 3), (route, "lds", 2)] and (r.one_by_one, r.global_batched) == (5, 0)


def B_to_problem(d):
    from tests import single_bb_cases as B
    return B.to_problem(lp, d)


def test_stats_count_the_nodes_of_global_form_batches():
    s = sbb.SingleBranchAndBound(B_to_problem(G.big_bb_problem()), width=4, beyond_lds=True)
    assert s.rounds.beyond_lds is True and s.rounds.global_batched == 0
    assert sbb.SingleBranchAndBound(B_to_problem(G.big_bb_problem()), width=4).rounds.beyond_lds is False


# ------------------------------------------------------------------ the array yardstick at multi-trip shapes
@pytest.mark.parametrize("m", [257, 513])
def test_assemble_rows_equals_the_models_build_at_multi_trip_shapes(m):
    """single_lps_cases.assemble_rows against sc.build, bit for bit, on one generated member of m rows (ncv = 3, all
    six kinds of rows: both senses and `=`, flipped and not) -- more rows than one trip of a 256-thread workgroup."""
    kinds = G.row_kinds(m, True)[0]
    assert {G.KIND_OF[k] for k in kinds} == {G.SLACK, G.EQ, G.ART} and set(kinds) == set(G.KIND_OF)
    d = G.kinds_problem(m, seed=m)
    low = lp.single_lps.lower_problem_rows_single(C.to_problem(lp, d))
    assert low is not None and not low.float_zero and low.L.shape == (m + 1, 4)
    assert [(op, bool(r < 0)) for (op, _, r) in d["constraints"]] == kinds
    got = C.assemble_rows(low.L, low.sense, low.col_int_sum)
    want = sc.build(d)
    n_eq, n_art = C.counts(kinds)
    assert want["main"][0].shape == (m + 1, 3 + (m - n_eq) + 1) and want["art"][0].shape == (m + 1, 3 + (m - n_eq) + 1 + n_art)
    assert sc.same_bits(got[0], want["main"][0]) and np.array_equal(got[1], want["main"][1])
    assert sc.same_bits(got[2], want["art"][0]) and np.array_equal(got[3], want["art"][1])


@pytest.mark.parametrize("m", [255, 256, 257, 513, 1100])
def test_generated_rows_put_every_kind_on_both_sides_of_the_chunk_boundaries(m):
    """The arrays of the GPU file's row-pass cases: in the two-phase group slack rows, `=` rows and artificial rows
    each end a thread's chunk and each begin the next one somewhere, the first and the last row are artificial in
    member 0, and both members have the same counts."""
    members = G.row_kinds(m, True)
    last, first = G.kinds_at_boundaries(members, m)
    assert last == first == {G.SLACK, G.EQ, G.ART}
    assert G.KIND_OF[members[0][0]] == G.ART and G.KIND_OF[members[0][-1]] == G.EQ
    assert len(G.chunk_boundaries(m)) == (m - 1) // G.chunk_of(m) >= 128 and G.chunk_of(m) == {255: 1, 256: 1, 257: 2, 513: 3, 1100: 5}[m]
    L, sense = G.rows_arrays(m, True)
    want = G.expected_rows(m, True)
    assert L.shape == (2, m + 1, 4) and all(w[2] is not None for w in want)
    assert np.signbit(L[0, :m, -1][L[0, :m, -1] == 0]).any()                  # a -0.0 right-hand side: not flipped
    single = G.row_kinds(m, False)
    assert {G.KIND_OF[k] for k in single[0]} == {G.SLACK} and len(set(single[0])) == 2
    assert all(w[2] is None for w in G.expected_rows(m, False))
