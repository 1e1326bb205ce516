"""Double-precision batches built on the device (mi355x_batch_create_lps / mi355x_multibatch_create_lps: k_blp_rows,
k_assemble, k_art_objective) against the batches the host builds from build_tableau -- start states bit for
bit, then statuses, pivot counts and final entries through the unchanged solve entries -- and against the numpy
statement of the kernels (tests/lps_cases.assemble) at the shapes where their loops take more than one trip; the
one-copy read-back (k_batch_readback); then the public functions on top: solve_problems(from_rows=True) and
solve_lps."""
import ctypes

import numpy as np
import pytest

from tests import lps_cases as lc
from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi
bl = lp.batch_lps
pytestmark = pytest.mark.gpu
CAP = 2000                                    # every solve carries a finite cap


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(lc.bits(a), lc.bits(b))


def _check_members(main, art, expected):
    """Every member of a device-built pair against expected[q] = (M, basis, A or None, abasis or None)."""
    assert main.n_lps == len(expected) and (art is None) == (expected[0][2] is None)
    for q, (M, basis, A, abasis) in enumerate(expected):
        assert (main.rows, main.cols) == M.shape
        G, gb = main.download(q)
        assert _same_bits(G, M), q
        assert np.array_equal(gb, basis), q
        if A is not None:
            assert (art.rows, art.cols) == A.shape
            G, gb = art.download(q)
            assert _same_bits(G, A), q
            assert np.array_equal(gb, abasis), q


def _stored(batch, q):
    """Member q of a TableauBatch as stored: rows x ld, the padding columns included."""
    ld = ctypes.c_int64(0)
    L = capi.lib()
    assert L.mi355x_batch_debug_stored(batch._h, q, None, ctypes.byref(ld)) == capi.MI_OK
    out = np.full((batch.rows, ld.value), np.nan)
    assert L.mi355x_batch_debug_stored(batch._h, q, out.ctypes.data_as(ctypes.c_void_p), None) == capi.MI_OK
    return out


# ------------------------------------------------------------------ start states
def test_start_states_equal_build_tableau_on_the_generators_groups():
    groups = {}
    for seed in range(120):
        p, _ = lc.problem(lp, seed)
        low = lp.lower_problem_rows(p)
        n_eq, n_art, _ = (int(x) for x in bl.row_counts(low.L, low.sense))
        groups.setdefault(low.L.shape + (n_eq, n_art), []).append((p, low))
    assert sum(len(g) > 1 for g in groups.values()) >= 10
    assert any(key[3] > 0 for key in groups) and any(key[3] == 0 for key in groups)
    for members in groups.values():
        main, art = lp.MultiDeviceBatch.from_lps(np.stack([l.L for _, l in members]),
                                                 np.stack([l.sense for _, l in members]), n_devices=1)
        _check_members(main, art, [lc.host_tableaux(lp, p)[:4] for p, _ in members])


PATTERNS = {
    "le": lambda i: (0, False),
    "mixed": lambda i: ((0, False), (1, False), (2, False), (1, True), (0, True), (2, True))[i % 6],
    "all_art": lambda i: ((1, False), (2, False), (0, True), (2, True))[i % 4],
    "none_art": lambda i: ((0, False), (1, True))[i % 2],
}


@pytest.mark.parametrize("n, m, ncv, pattern, n_devices", [
    (3, 3, 12, "le", 1),            # cols = 16: no padding in the main tableau
    (3, 3, 5, "le", 1),             # cols = 9: padding
    (2, 3, 13, "mixed", 1),         # cols = 16, artificial 18 (ld 32)
    (2, 6, 9, "mixed", 1),          # cols = 14, artificial 18
    (2, 2, 4100, "all_art", 1),     # a stored row longer than one pass of the column grid (16 x 256)
    (2, 1030, 2, "mixed", 1),       # more rows than the row grid (1024) and than a workgroup's threads
    (5, 4, 3, "mixed", 2),          # 3 + 2 members over two logical devices: the member offsets
    (3, 5, 3, "all_art", 1),
    (3, 5, 3, "none_art", 1),
])
def test_assembly_at_the_shapes_where_a_loop_takes_another_trip(n, m, ncv, pattern, n_devices):
    L, sense = lc.random_rows(n, m, ncv, 7 * m + ncv, PATTERNS[pattern])
    expected = [lc.assemble(L[q], sense[q]) for q in range(n)]
    if pattern == "all_art":
        assert all((e[1] == e[0].shape[1]).all() for e in expected)
    if pattern in ("le", "none_art"):
        assert expected[0][2] is None
    main, art = lp.MultiDeviceBatch.from_lps(L, sense, n_devices=n_devices)
    assert main.info()["n_sub_batches"] == n_devices
    _check_members(main, art, expected)
    # the same through the single-batch entry, and every stored column: the padding [cols, ld) holds +0.0
    main, art = lp.TableauBatch.from_lps(L, sense)
    _check_members(main, art, expected)
    for batch, k in ((main, 0), (art, 2)):
        if batch is None:
            continue
        for q in range(n):
            S = _stored(batch, q)
            assert S.shape[1] % 16 == 0 and S.shape[1] >= batch.cols
            assert _same_bits(S[:, :batch.cols], expected[q][k]), q
            assert not lc.bits(S[:, batch.cols:]).any(), q
    if (m, ncv, pattern) == (3, 12, "le"):
        assert _stored(main, 0).shape[1] == main.cols == 16
    if (m, ncv, pattern) == (3, 13, "mixed"):
        assert _stored(main, 0).shape[1] == main.cols == 16 and _stored(art, 0).shape[1] == 32


def test_assembly_where_the_launcher_caps_its_grid():
    """16390 members of 16 rows: one column block times 16 row blocks times the members is 262 240 workgroups, past
    the launcher's 2^18, so it halves the row blocks to 8 and every workgroup's row loop takes two trips of stride
    8.  Six distinct members of one group, tiled: the stored tableaux (padding included) of the first six, of six
    around the middle and of the last six, and the read-back planes and bases of every member of both batches."""
    n, m, ncv = 16390, 15, 2
    L6, sense6 = lc.random_rows(6, m, ncv, 7 * m + ncv, PATTERNS["mixed"])
    expected = [lc.assemble(L6[q], sense6[q]) for q in range(6)]
    assert len({lc.bits(e[2]).tobytes() for e in expected}) == 6
    reps = -(-n // 6)
    main, art = lp.TableauBatch.from_lps(np.tile(L6, (reps, 1, 1))[:n], np.tile(sense6, (reps, 1))[:n])
    assert main.n_lps == art.n_lps == n and (art.rows, art.cols) == expected[0][2].shape
    assert min(main.rows, 1024) * n > 1 << 18 and -(-_stored(art, 0).shape[1] // 256) == 1
    for batch, k in ((main, 0), (art, 2)):
        for q in list(range(6)) + list(range(n // 2 - 3, n // 2 + 3)) + list(range(n - 6, n)):
            S = _stored(batch, q)
            assert _same_bits(S[:, :batch.cols], expected[q % 6][k]), q
            assert not lc.bits(S[:, batch.cols:]).any(), q
        tiled = lambda plane: np.tile(np.stack(plane), (reps,) + (1,) * plane[0].ndim)[:n]
        rows, cols, bases = batch.readback()
        assert _same_bits(rows, tiled([e[k][-1] for e in expected]))
        assert _same_bits(cols, tiled([e[k][:, -1] for e in expected]))
        assert np.array_equal(bases, tiled([e[k + 1] for e in expected]))


# ------------------------------------------------------------------ solves through the existing entries
def _host_pair(L, sense, is_max, n_devices):
    """(main, artificial or None) MultiDeviceBatch built on the host: build_tableau per member, from_arrays."""
    tabs = [lp.build_tableau(lc.problem_of_rows(lp, L[q], sense[q], is_max)) for q in range(len(L))]
    if isinstance(tabs[0], list):
        return (lp.MultiDeviceBatch.from_arrays(np.stack([t[1]._matrix for t in tabs]), np.stack([t[1]._basis for t in tabs]), n_devices),
                lp.MultiDeviceBatch.from_arrays(np.stack([t[0]._matrix for t in tabs]), np.stack([t[0]._basis for t in tabs]), n_devices))
    return lp.MultiDeviceBatch.from_arrays(np.stack([t._matrix for t in tabs]), np.stack([t._basis for t in tabs]), n_devices), None


def _solved_both_ways(L, sense, is_max, n_devices=2):
    out = []
    for main, art in (lp.MultiDeviceBatch.from_lps(L, sense, n_devices=n_devices), _host_pair(L, sense, is_max, n_devices)):
        st, npv = bl.solve_batches(main, art, is_max, max_pivots=CAP)
        out.append((main, art, st, npv))
    return out


def _same_outcome(dev, host):
    (dm, da, dst, dnp), (hm, ha, hst, hnp) = dev, host
    assert dst.tolist() == hst.tolist() and dnp.tolist() == hnp.tolist()
    for a, b in ((dm, hm), (da, ha)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        for q in range(a.n_lps):
            (G, gb), (H, hb) = a.download(q), b.download(q)
            assert _same_bits(G, H), q
            assert np.array_equal(gb, hb), q


@pytest.fixture(scope="module")
def single_phase():
    L, sense = lc.single_phase_members(6, 7, 5, 11)
    return (L, sense) + tuple(_solved_both_ways(L, sense, True))


@pytest.fixture(scope="module")
def two_phase():
    L, sense = lc.two_phase_members(7, 4, 12)
    return (L, sense) + tuple(_solved_both_ways(L, sense, False))


def test_single_phase_group_solves_as_the_host_built_one(single_phase):
    _, _, dev, host = single_phase
    assert dev[1] is None
    _same_outcome(dev, host)
    st = dev[2].tolist()
    assert st[1] == capi.MI_UNBOUNDED and st.count(capi.MI_OPTIMAL) == len(st) - 1
    assert dev[3].min() >= 1


def test_two_phase_group_solves_as_the_host_built_one(two_phase):
    _, _, dev, host = two_phase
    assert dev[1] is not None and dev[3].shape == (7, 2)
    _same_outcome(dev, host)
    st = dev[2].tolist()
    assert st[1] == capi.MI_INFEASIBLE and st[2] == capi.MI_UNBOUNDED and st.count(capi.MI_OPTIMAL) == len(st) - 2
    assert dev[3][:, 0].min() >= 1                    # phase 1 pivots in every member


# ------------------------------------------------------------------ read-back
def test_readback_equals_the_per_member_download(two_phase, single_phase):
    for case in (two_phase, single_phase):
        for batch in (case[2][0], case[2][1], case[3][0]):        # device-built main and artificial, host-built main
            if batch is None:
                continue
            assert batch.info()["n_sub_batches"] == 2
            rows, cols, bases = batch.readback()
            assert rows.shape == (batch.n_lps, batch.cols) and cols.shape == (batch.n_lps, batch.rows)
            for q in range(batch.n_lps):
                G, gb = batch.download(q)
                assert _same_bits(rows[q], G[-1]) and _same_bits(cols[q], G[:, -1]) and np.array_equal(bases[q], gb), q
    # the single-batch entry, before any solve; outputs may be NULL
    L, sense = two_phase[:2]
    main, art = lp.TableauBatch.from_lps(L, sense)
    for batch in (main, art):
        rows, cols, bases = batch.readback()
        for q in range(batch.n_lps):
            G, gb = batch.download(q)
            assert _same_bits(rows[q], G[-1]) and _same_bits(cols[q], G[:, -1]) and np.array_equal(bases[q], gb), q
    only = np.empty((main.n_lps, main.rows))
    assert capi.lib().mi355x_batch_readback(main._h, None, only.ctypes.data_as(ctypes.c_void_p), None) == capi.MI_OK
    assert _same_bits(only, main.readback()[1])


# ------------------------------------------------------------------ the public list route
def _same_result(a, b):
    assert type(a) is type(b)
    if isinstance(a, Exception):
        assert a.args == b.args
        return
    assert isinstance(a, lp.Tableau)
    assert _same_bits(a.matrix, b.matrix) and np.array_equal(a.basis_columns, b.basis_columns)
    assert a.n_pivots == b.n_pivots and type(a.n_pivots) is type(b.n_pivots)
    assert a.var_mapping == b.var_mapping and a.problem is b.problem and a.instance_problem is b.instance_problem
    assert (a.var_count, a.constraint_count, a.fp_tolerance_factor) == (b.var_count, b.constraint_count, b.fp_tolerance_factor)


@pytest.fixture(scope="module")
def mixed_list(single_phase, two_phase):
    ps = [lc.problem_of_rows(lp, single_phase[0][q], single_phase[1][q], True) for q in range(4)]
    ps += [lc.problem_of_rows(lp, two_phase[0][q], two_phase[1][q], False) for q in range(5)]
    L, sense = lc.single_phase_members(1, 3, 4, 5)
    ps.append(lc.problem_of_rows(lp, L[0], sense[0], True))                                       # alone in its group
    ps.append(lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1), ("y", 2)],
                         integer_vars=["x"], constraints=[("<=", [("x", 1), ("y", 1)], 4)]))      # declined: integer
    ps.append(lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1), ("y", -2)],
                         var_bounds=[("x", (0, 3)), ("y", (1, 5))]))                              # no constraints
    ps.append(lp.Problem(type="max", vars=["x", "y"], objective_var="w", objective_func=[("x", 1), ("y", 1)],
                         constraints=[("<=", [("x", 1), ("y", 2)], 4), (">=", [("x", -1), ("y", 1)], -1)]))   # "basis"
    # two members with bounds of every kind and a constant, one group
    for ub in (6, 7.5):
        ps.append(lp.Problem(type="max", vars=["a", "b", "c", "d"], objective_var="w",
                             objective_func=[("a", 1), ("b", 2), ("c", 1), ("d", 0.5)],
                             var_bounds=[("a", (1, ub)), ("b", (None, 3)), ("c", (None, None))],
                             constraints=[("<=", [("a", 1), ("b", 1), ("c", 1), ("d", 1)], 10),
                                          (">=", [("a", 1), ("c", -1)], 0.5), ("=", [("b", 1), ("d", 2)], 4)]))
    host, groups = lp.group_lowered_rows(ps)
    assert sorted(host.values()) == ["alone", "basis", "integer variables", "no constraints"]
    assert sorted(len(g) for g in groups.values()) == [2, 4, 5]
    return ps


def test_solve_problems_from_rows_equals_the_default_route(mixed_list):
    want = lp.solve_problems(mixed_list, errorp=False, max_pivots=CAP)
    got = lp.solve_problems(mixed_list, errorp=False, max_pivots=CAP, from_rows=True)
    assert len(got) == len(want) == len(mixed_list)
    for a, b in zip(got, want):
        _same_result(a, b)
    kinds = {type(r) for r in want}
    assert {lp.Tableau, lp.UnboundedProblemError, lp.InfeasibleProblemError, lp.UnsupportedConstraintError} <= kinds
    assert isinstance(want[-1], lp.Tableau) and isinstance(want[-2], lp.Tableau)
    assert [lp.solution_variable(got[-1], v) for v in "wabcd"] == [lp.solution_variable(want[-1], v) for v in "wabcd"]
    # errorp: the first member without a solution is raised, after every member was attempted
    first = next(r for r in want if isinstance(r, Exception))
    for kw in ({}, {"from_rows": True}):
        with pytest.raises(type(first)):
            lp.solve_problems(mixed_list, max_pivots=CAP, **kw)


def test_solve_problems_from_rows_under_a_pivot_cap(mixed_list):
    """max_pivots = 1: members end in the pivot cap's SolverError on both routes alike."""
    want = lp.solve_problems(mixed_list, errorp=False, max_pivots=1)
    got = lp.solve_problems(mixed_list, errorp=False, max_pivots=1, from_rows=True)
    for a, b in zip(got, want):
        _same_result(a, b)
    assert any(type(r) is lp.SolverError and r.args == ("pivot cap reached",) for r in want)


# ------------------------------------------------------------------ the array front end
def test_solve_lps_gives_the_batches_results(single_phase, two_phase):
    for (L, sense, dev, _), is_max in ((single_phase, True), (two_phase, False)):
        st, npv, rows, cols, bases = lp.solve_lps(L, sense, is_max=is_max, devices=2, max_pivots=CAP)
        assert st.tolist() == dev[2].tolist() and npv.tolist() == dev[3].tolist()
        for q in range(len(L)):
            G, gb = dev[0].download(q)
            assert _same_bits(rows[q], G[-1]) and _same_bits(cols[q], G[:, -1]) and np.array_equal(bases[q], gb), q
