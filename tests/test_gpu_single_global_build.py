"""Single-float batches built on the device in the GLOBAL form (kernels_single_assemble_global.inc behind
mi355x_sbatch_create_lps_global and mi355x_sbatch_create_nodes_global; `form="global"` and `beyond_lds=True` in
single.py, single_lps.py and single_bb.py) against the float32 model of tests/single_cases.py, against
single_lps_cases.assemble_rows for arrays and against single_bb_cases.build_node / search for nodes: what a member
starts from -- every entry, sign of zero included, both bases, all-zero padding bits as stored -- and what it ends
with -- status, pivot counts per phase, traces, final basis and every final entry.  Bits are compared with
sc.same_bits; there is no tolerance anywhere, and the new route's own output is never a yardstick.

Every test that builds from Problem dicts asserts group_lowered_rows_single(...)[0] == {}: no member leaves the
device route unnoticed.  The branch-and-bound tests assert the stats() counts.

The folds of the write pass's launcher (sga_launch), each crossed by the smallest shape that crosses it and met by one
just below:
    columns   at most 8 column blocks of 256 quads: a leading dimension beyond 8192 floats makes a workgroup stride
              (artificial tableau of 8192 | 8193 columns at m = 5)
    rows      at most 1024 row blocks: a member of more than 1024 rows makes a workgroup stride (m = 1023 | 1024)
    total     at most 2^16 workgroups: beyond them the row blocks are halved until they fit, a workgroup taking
              several rows (1024 | 1025 members of 64 rows)
The row passes fold at 256 rows (a thread owns ceil(m / 256) consecutive rows): m = 255, 256, 257, 513, 1100.

On the parent commit every test here fails: the symbols and keywords do not exist."""
import ctypes

import numpy as np
import pytest

from tests import single_bb_cases as B
from tests import single_cases as sc
from tests import single_global_build_cases as G
from tests import single_lps_cases as C
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi, sbb = lp.capi, lp.single_bb
F32 = np.float32
THREADS = [256, 1024]
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)
    lp.single.set_batch_global_threads(0)
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = None


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def lowered(ds):
    """The group's arrays (L, sense, col_int_sum), after the condition: no member strays to the host route."""
    ps = [C.to_problem(lp, d) for d in ds]
    host, groups = lp.group_lowered_rows_single(ps)
    assert host == {} and len(groups) == 1
    (_, members), = groups.items()
    assert [k for k, _ in members] == list(range(len(ds)))
    lows = [low for _, low in members]
    return (np.stack([low.L for low in lows]), np.stack([low.sense for low in lows]),
            np.stack([low.col_int_sum for low in lows]))


def check_info(sb, n, threads=0):
    info = sb.info()
    assert info["form"] == 3 and info["n_lps"] == n and info["ld"] % 32 == 0 and info["ld"] >= info["cols"]
    assert (info["rows"], info["cols"]) == (sb.rows, sb.cols) and info["members_per_cu"] >= 1
    assert info["lds_bytes_per_member"] == 4 * ((sb.cols + 3) // 4 * 4 + (sb.rows + 3) // 4 * 4)
    auto = 256 if sb.rows * info["ld"] * 4 < 256 * 1024 else 1024          # the global form's own rule
    assert info["workgroup_threads"] == (threads or auto)


def create(arrays, threads=0):
    lp.single.set_batch_global_threads(threads)
    main, art = lp.SingleBatch.from_lps(*arrays, form="global")
    for sb in (main, art):
        if sb is not None:
            check_info(sb, arrays[0].shape[0], threads)
    return main, art


def close(*batches):
    for sb in batches:
        if sb is not None:
            sb.close()


def stored(sb, q):
    """Member q as stored: rows x ld, the padding columns included."""
    ld = ctypes.c_int64(0)
    L = capi.lib()
    assert L.mi355x_sbatch_debug_stored(sb._handle, q, None, ctypes.byref(ld)) == capi.MI_OK
    out = np.full((sb.rows, ld.value), np.nan, dtype=F32)
    assert L.mi355x_sbatch_debug_stored(sb._handle, q, out.ctypes.data_as(ctypes.c_void_p), None) == capi.MI_OK
    return out


def check_member(main, art, q, want, download=True):
    """Member q before any solve against (main, main basis, art or None, art basis or None): every entry, both bases,
    the padding all-zero bits."""
    assert (art is None) == (want[2] is None), q
    for sb, M, basis in ((main, want[0], want[1]), (art, want[2], want[3])):
        if sb is None:
            continue
        S = stored(sb, q)
        assert S.shape[0] == M.shape[0] and sb.cols == M.shape[1], q
        assert same_bits(S[:, :sb.cols], M), q
        assert not S[:, sb.cols:].view(np.uint32).any(), q
        if download:
            G_, gb = sb.download(q)
            assert same_bits(G_, M) and np.array_equal(gb, basis), q
            assert sb.trace(q).shape[0] == 0


def model_build(d):
    b = sc.build(d)
    return b["main"][0], b["main"][1], (b["art"][0] if b["art"] else None), (b["art"][1] if b["art"] else None)


def check_assembly(ds):
    main, art = create(lowered(ds))
    try:
        for q, d in enumerate(ds):
            check_member(main, art, q, model_build(d))
        return main.cols, (None if art is None else art.cols)
    finally:
        close(main, art)


# ------------------------------------------------------------------ 1. the existing groups through the new entry
def test_assembly_sweep_m_1_to_7_ncv_1_to_5_all_senses():
    two_phase = 0
    for (m, ncv), ds in C.sweep_groups().items():
        n_eq, n_art = C.counts(C.sweep_rows(m, ncv))
        mc, ac = check_assembly(ds)
        assert mc == ncv + (m - n_eq) + 1 and ac == (mc + n_art if n_art else None), (m, ncv)
        two_phase += n_art > 0
    assert 0 < two_phase < 35


@pytest.mark.parametrize("group", ["moving", "zero_rhs", "bounds", "outcome", "driveout", "single_phase"])
def test_assembly_rows_that_move_zero_right_hand_sides_and_bounds(group):
    ds = getattr(C, group + "_group")()
    check_assembly(ds)
    if group == "zero_rhs":
        # the negated rows hold +0.0 for integer zeros, for what is not mentioned and in the other rows' slack columns;
        # the -0.0 right-hand side stays (the row is not negated) -- on the device as in the model
        main, art = create(lowered(ds))
        try:
            for M in (sc.build(ds[0])["main"][0], main.download(0)[0]):
                assert (M[2, [1, 2]] == 0).all() and not np.signbit(M[2, [1, 2]]).any() and M[2, -1] == 3
                assert np.signbit(M[0, -1]) and M[0, -1] == 0
        finally:
            close(main, art)


def test_assembly_of_extreme_rows():
    """The artificial objective row is the float sum in INCREASING row order (3e38 + 3e38 - 3e38 = inf, any other order
    3e38; 1 + 2**-24 + 2**-24 = 1, the other way round 1 + 2**-23), a row with a subnormal negative right-hand side is
    negated exactly (no flush) and its sense flipped, a right-hand side -0.0 is not: as the LDS test states them."""
    ds = C.extreme_rows_group()
    assert check_assembly(ds) == (9, 12)
    main, art = create(lowered(ds))
    try:
        got = [(art.download(q)[0][-1, 0], art.download(q)[0][-1, 1]) for q in range(3)]
        assert got == [(F32(np.inf), F32(1)), (C.BIG, F32(1)), (C.BIG, F32(1 + 2.0 ** -23))]
        for q in range(3):
            M = main.download(q)[0]
            assert M[3, -1].view(np.uint32) == C.SUB.view(np.uint32)
            assert M[3, 3].view(np.uint32) == F32(3e-39).view(np.uint32)
            assert M[4, -1] == 0 and np.signbit(M[4, -1])
    finally:
        close(main, art)


@pytest.mark.parametrize("kw,cols", [(dict(main_cols=32), (32, None)), (dict(main_cols=33), (33, None)),
                                     (dict(art_cols=64), (54, 64)), (dict(art_cols=65), (55, 65))])
def test_assembly_at_the_steps_of_the_leading_dimension(kw, cols):
    assert check_assembly(C.ld_step_group(**kw)) == cols


# ------------------------------------------------------------------ 2. the row pass across its trips
def check_arrays(L, sense, wants, members=None):
    main, art = create((L, sense, None))
    try:
        for q in (range(L.shape[0]) if members is None else members):
            check_member(main, art, q, wants[q])
        return main, art
    except BaseException:
        close(main, art)
        raise


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("m", [255, 256, 257, 513, 1100])
def test_row_pass_across_trips(m, two_phase):
    """ncv = 3, two members, against assemble_rows: slack rows, `=` rows and artificial rows on both sides of the
    chunk boundaries (tests/test_single_global_build_host.py states it), first and last row artificial in member 0."""
    L, sense = G.rows_arrays(m, two_phase)
    wants = G.expected_rows(m, two_phase)
    assert (wants[0][2] is not None) == two_phase
    if two_phase:
        assert wants[0][3][0] >= wants[0][0].shape[1] - 1 and wants[0][3][-1] == wants[0][0].shape[1] - 1
    close(*check_arrays(L, sense, wants))


# ------------------------------------------------------------------ 3. the write pass across its folds
@pytest.mark.parametrize("ncv,art_cols", [(8184, 8192), (8185, 8193)])
def test_write_pass_wide(ncv, art_cols):
    """m = 5: the artificial tableau's leading dimension at (8192) and beyond (8224) one grid row of quads."""
    L, sense = G.wide_arrays(ncv)
    wants = [C.assemble_rows(L[q], sense[q]) for q in range(2)]
    assert wants[0][2].shape == (6, art_cols) and wants[0][0].shape == (6, ncv + 5)
    main, art = check_arrays(L, sense, wants)
    assert art.info()["ld"] == (8192 if art_cols == 8192 else 8224)
    close(main, art)


@pytest.mark.parametrize("m", [1023, 1024])
def test_write_pass_tall(m):
    """1024 rows fill the grid's row blocks, 1025 make a workgroup take a second row."""
    L, sense = G.rows_arrays(m, True)
    close(*check_arrays(L, sense, G.expected_rows(m, True)))


@pytest.mark.parametrize("n", [1024, 1025])
def test_write_pass_many_members(n):
    """64 rows x n members: 2^16 workgroups at n = 1024, one workgroup per two rows at 1025.  The model is built once
    and compared with every member."""
    d = G.many_member()
    assert lp.group_lowered_rows_single([C.to_problem(lp, d)] * 2)[0] == {}
    low = lp.single_lps.lower_problem_rows_single(C.to_problem(lp, d))
    want = model_build(d)
    assert want[0].shape == (64, 41) and want[2].shape == (64, 85)
    L, sense = np.repeat(low.L[None], n, axis=0), np.repeat(low.sense[None], n, axis=0)
    main, art = create((L, sense, np.repeat(low.col_int_sum[None], n, axis=0)))
    try:
        for q in range(n):
            check_member(main, art, q, want, download=q in (0, 1, n // 2, n - 2, n - 1))
        rhs, obj, basis = sbb.readback(main)                 # every member's basis, in one copy
        assert (basis == want[1][None]).all() and same_bits(obj, np.repeat(want[0][-1:], n, axis=0))
        rhs, obj, basis = sbb.readback(art)
        assert (basis == want[3][None]).all() and same_bits(obj, np.repeat(want[2][-1:], n, axis=0))
    finally:
        close(main, art)


# ------------------------------------------------------------------ 4. / 5. solves
def solve_group(ds, wants, threads, per_call=0):
    arrays = lowered(ds)
    main, art = create(arrays, threads)
    n = len(ds)
    is_max = ds[0]["type"] == "max"
    try:
        for q, w in enumerate(wants):
            b = w["build"]
            check_member(main, art, q, (b["main"][0], b["main"][1], b["art"][0] if b["art"] else None,
                                        b["art"][1] if b["art"] else None))
        total = None
        for _ in range(2000):
            st, npv = main.solve(is_max, 1024, per_call) if art is None else art.solve_two_phase(main, is_max, 1024, per_call)
            assert (main if art is None else art).last_return == capi.MI_OK
            total = npv if total is None else total + npv
            if not (st == capi.MI_MAX_PIVOTS).any():
                break
        else:
            raise AssertionError("the group did not finish")
        for q, w in enumerate(wants):
            assert int(st[q]) == w["status"], (q, int(st[q]), w["status"])
            assert tuple(np.atleast_1d(total[q]).tolist()) == w["n"], (q, total[q], w["n"])
            assert _pairs(main.trace(q).tolist()) == _pairs(w["main_trace"]), q
            G_, gb = main.download(q)
            assert same_bits(G_, w["M"]) and np.array_equal(gb, w["mbasis"]), q
            if art is not None:
                assert _pairs(art.trace(q).tolist()) == _pairs(w["art_trace"]), q
                A, ab = art.download(q)
                assert same_bits(A, w["A"]) and np.array_equal(ab, w["abasis"]), q
        assert total.shape == ((n,) if art is None else (n, 2))
    finally:
        close(main, art)
    return arrays


@pytest.mark.parametrize("two_phase", [False, True])
def test_the_first_shapes_the_lds_form_declines(two_phase):
    """98 x 300 single-phase and 84 x 300 two-phase with sc.synthetic's numbers: built, then solved, against the model;
    the LDS entry still answers MI_UNSUPPORTED for both."""
    ds = G.beyond_group(two_phase)
    wants = C.model_solution(G.beyond_group, two_phase)
    shapes = (wants[0]["build"]["main"][0].shape, wants[0]["build"]["art"][0].shape if two_phase else None)
    assert shapes == (((85, 385), (85, 469)) if two_phase else ((99, 399), None))
    assert not C.fits(*(shapes[1] if two_phase else shapes[0]))
    assert all(sum(w["n"]) > 40 for w in wants)
    arrays = solve_group(ds, wants, 0)
    with pytest.raises(capi.Mi355xError) as e:
        lp.SingleBatch.from_lps(*arrays)
    assert e.value.code == capi.MI_UNSUPPORTED


SOLVED = {"outcome": (C.outcome_group, ()), "driveout": (C.driveout_group, ()),
          "medium_max": (C.medium_group, ("max",)), "medium_min": (C.medium_group, ("min",))}


@pytest.mark.parametrize("per_call", [0, 3])
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("name", sorted(SOLVED))
def test_solves_from_device_built_members(name, threads, per_call):
    fn, args = SOLVED[name]
    wants = C.model_solution(fn, *args)
    if name == "outcome":
        assert [w["status"] for w in wants] == C.OUTCOMES
    if name == "driveout":
        assert all(w["status"] == sc.OPTIMAL and w["n"][0] == 1 for w in wants)
    if name.startswith("medium"):
        assert all(w["status"] == sc.OPTIMAL and min(w["n"]) > 0 for w in wants)
    solve_group(fn(*args), wants, threads, per_call)


def test_solves_two_members_of_256x512():
    wants = C.model_solution(G.config4_group)
    assert [(w["status"], w["n"]) for w in wants] == [(sc.OPTIMAL, (167,)), (sc.OPTIMAL, (104,))]
    assert wants[0]["build"]["main"][0].shape == (257, 769)
    solve_group(G.config4_group(), wants, 0)


def test_solves_a_two_phase_pair_of_102x405_and_102x402():
    wants = C.model_solution(G.two_phase_102_group)
    b = wants[0]["build"]
    assert (b["art"][0].shape, b["main"][0].shape) == ((102, 405), (102, 402))
    assert all(w["status"] == sc.OPTIMAL and w["n"][0] == 3 and w["n"][1] > 40 for w in wants)
    solve_group(G.two_phase_102_group(), wants, 0)


@pytest.mark.parametrize("name", ["outcome", "medium_min"])
def test_solve_lps_single_in_the_global_form(name, monkeypatch):
    fn, args = SOLVED[name]
    ds, wants = fn(*args), C.model_solution(fn, *args)
    L, sense, _ = lowered(ds)
    made = []
    real = lp.SingleBatch.from_lps.__func__

    def from_lps(cls, *a, **kw):
        made.append(kw.get("form", "lds"))
        return real(cls, *a, **kw)
    monkeypatch.setattr(lp.SingleBatch, "from_lps", classmethod(from_lps))
    st, npv, rhs, obj_rows, bases = lp.solve_lps_single(L, sense, is_max=ds[0]["type"] == "max", form="global")
    assert made == ["global"]
    assert rhs.dtype == np.float32 and obj_rows.dtype == np.float32 and bases.dtype == np.int64
    for q, w in enumerate(wants):
        assert int(st[q]) == w["status"] and tuple(np.atleast_1d(npv[q]).tolist()) == w["n"], q
        assert same_bits(rhs[q], w["M"][:, -1]) and same_bits(obj_rows[q], w["M"][-1]), q
        assert np.array_equal(bases[q], w["mbasis"]), q


# ------------------------------------------------------------------ 6. declines
def _raw_create(L, s, sums, m, ncv):
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    p = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in (L, s, sums)]
    rc = capi.lib().mi355x_sbatch_create_lps_global(ctypes.byref(hm), ctypes.byref(ha), L.shape[0], m, ncv, p[0], p[1], p[2], 0)
    return rc, hm, ha


def test_declines_leave_no_handle():
    low = lp.single_lps.lower_problem_rows_single(C.to_problem(lp, C.integer_sum_member()))
    L, s, sums = np.stack([low.L] * 2), np.stack([low.sense] * 2), np.stack([low.col_int_sum] * 2)
    with pytest.raises(capi.Mi355xError) as e:
        lp.SingleBatch.from_lps(L, s, sums, form="global")
    assert e.value.code == capi.MI_UNSUPPORTED
    rc, hm, ha = _raw_create(L, s, sums, 3, 2)
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value
    assert b"member 0" in capi.lib().mi355x_last_error()
    def snapshot(rows, cols):                                # pivot row + column snapshot, each rounded up to a quad
        return 4 * ((cols + 3) // 4 * 4 + (rows + 3) // 4 * 4)
    assert snapshot(6, 40000 + 5 + 1) > 156 * 1024
    rc, hm, ha = _raw_create(np.ones((2, 6, 40001), dtype=F32), np.zeros((2, 5), dtype=np.int32), None, 5, 40000)
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value
    # ... and when only the artificial shape is beyond it (five `>=` rows)
    assert snapshot(6, 39920 + 5 + 1) <= 156 * 1024 < snapshot(6, 39920 + 5 + 1 + 5)
    rc, hm, ha = _raw_create(np.ones((2, 6, 39921), dtype=F32), np.ones((2, 5), dtype=np.int32), None, 5, 39920)
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value
    # members that differ in their counts
    L, sense = (a.copy() for a in G.rows_arrays(255, True))
    sense[1, np.flatnonzero(sense[1] == 0)[0]] = 2
    rc, hm, ha = _raw_create(L, sense, None, 255, 3)
    assert rc == capi.MI_BAD_ARG and not hm.value and not ha.value
    assert b"member 1" in capi.lib().mi355x_last_error()


# ------------------------------------------------------------------ 7. the list route
def _same_result(r, w):
    """A slot of the list routes against another route's slot: type and bits."""
    assert type(r) is type(w), (r, w)
    if isinstance(w, Exception):
        assert r.args == w.args
        return
    assert isinstance(r, lp.SingleTableau) and same_bits(r.matrix, w.matrix)
    assert np.array_equal(r.basis_columns, w.basis_columns) and r.n_pivots == w.n_pivots
    assert r.var_mapping == w.var_mapping and r.is_max == w.is_max
    assert (r.var_count, r.constraint_count) == (w.var_count, w.constraint_count)
    assert r.problem is w.problem and r.instance_problem is w.instance_problem
    for v in r.problem.vars[:8]:
        a, b = lp.tableau_variable(r, v), lp.tableau_variable(w, v)
        assert type(a) is np.float32 and type(b) is np.float32 and a.view(np.uint32) == b.view(np.uint32)
    assert lp.tableau_objective_value(r).view(np.uint32) == lp.tableau_objective_value(w).view(np.uint32)


def _list():
    """One 98 x 300 group (members 1, 4, 8), one small group for the LDS form (0, 5, 9) and the host-route members."""
    sp = C.single_phase_group()
    big = G.beyond_group(False) + [C._synthetic_problem(300, 98, 5, False)]
    ds = [sp[0], big[0], C.float_zero_member(), C.integer_sum_member(), big[1], sp[1], C.lone_member(), C.declined_member(),
          big[2], sp[2]]
    return [C.to_problem(lp, d) for d in ds], big


def test_list_route_beyond_the_budget(monkeypatch):
    ps, big = _list()
    host, groups = lp.group_lowered_rows_single(ps)
    declined = host.pop(7)
    assert isinstance(declined, lp.UnsupportedConstraintError)
    assert host == {2: "float zero", 3: "integer sum", 6: "alone"}
    assert sorted(sorted(k for k, _ in v) for v in groups.values()) == [[0, 5, 9], [1, 4, 8]]
    assert lp.group_lowered_rows_single([ps[k] for k in (1, 4, 8)])[0] == {}
    calls, alone = [], []
    real_from_lps, real_solve_single = lp.SingleBatch.from_lps.__func__, lp.single_lps.solve_single

    def from_lps(cls, lps, *a, **kw):
        calls.append((kw.get("form", "lds"), lps.shape[0], lps.shape[1] - 1))
        return real_from_lps(cls, lps, *a, **kw)

    def solve_single(p, **kw):
        alone.append(next(k for k, q in enumerate(ps) if q is p))
        return real_solve_single(p, **kw)
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 2
    want = lp.single.solve_problems_single(ps, errorp=False, beyond_lds=True)
    want_capped = lp.single.solve_problems_single(ps, errorp=False, beyond_lds=True, max_pivots=4)
    monkeypatch.setattr(lp.SingleBatch, "from_lps", classmethod(from_lps))
    monkeypatch.setattr(lp.single_lps, "solve_single", solve_single)

    got = lp.solve_problems_single_from_rows(ps, errorp=False, beyond_lds=True)
    assert sorted(calls) == [("global", 3, 98), ("lds", 3, 3), ("lds", 3, 98)]       # ONE global create for the group
    assert sorted(alone) == [2, 3, 6]                                                # ... and none of its members alone
    for r, w in zip(got, want):
        _same_result(r, w)
    for k, d in zip((1, 4, 8), big):                         # the model's answer
        b = sc.build(d)
        st, tr, M, basis = sc.solve(b["main"][0], b["main"][1], True)
        assert st == sc.OPTIMAL and same_bits(got[k].matrix, M) and np.array_equal(got[k].basis_columns, basis)
        assert got[k].n_pivots == len(tr) > 40
    for r, w in zip(lp.solve_problems_single_from_rows(ps, errorp=False, beyond_lds=True, chunk=3), want):
        _same_result(r, w)
    for r, w in zip(lp.solve_problems_single_from_rows(ps, errorp=False, beyond_lds=True, max_pivots=4), want_capped):
        _same_result(r, w)
    assert isinstance(want_capped[1], lp.SolverError)

    del calls[:], alone[:]                                   # without the keyword: one by one, as before
    got = lp.solve_problems_single_from_rows(ps, errorp=False)
    assert sorted(calls) == [("lds", 3, 3), ("lds", 3, 98)] and sorted(alone) == [1, 2, 3, 4, 6, 8]
    for r, w in zip(got, want):
        _same_result(r, w)

    del calls[:], alone[:]                                   # ... and with too few members
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 4
    lp.solve_problems_single_from_rows(ps, errorp=False, beyond_lds=True)
    assert sorted(calls) == [("lds", 3, 3), ("lds", 3, 98)] and sorted(alone) == [1, 2, 3, 4, 6, 8]


# ------------------------------------------------------------------ 8. nodes
# (main columns of a node, depth, members, artificial bound row in front, `>=` rows, `=` rows, artificial node rows)
ASSEMBLY = [(31, 1, 1, False, 0, 0, 0),        # one below the padding boundary, no artificial row
            (32, 2, 3, False, 0, 0, 1),        # at the boundary; the node's own artificial row alone
            (33, 4, 65, True, 1, 0, 1),        # one above; the node's artificial row between base artificial rows
            (32, 1, 65, False, 2, 0, 1),       # the node's artificial row first
            (33, 2, 3, True, 0, 0, 2),         # the node's artificial rows last
            (30, 3, 3, False, 1, 1, 1),        # the boundary inside the artificial columns
            (31, 4, 3, False, 0, 0, 0)]


def check_nodes(base, entries, threads=0):
    """create_nodes(form="global") of the entries against build_node: every entry, both bases, the padding."""
    g = sbb.GeneralFormSingle(B.to_problem(lp, base))
    assert all(g.device_ok(e) for e in entries)
    lp.single.set_batch_global_threads(threads)
    b = sbb.Base(g)
    try:
        main, art = b.create_nodes(entries, form="global")
    finally:
        b.close()
    try:
        for sb in (main, art):
            if sb is not None:
                check_info(sb, len(entries), threads)
        for q, e in enumerate(entries):
            check_member(main, art, q, B.build_node(base, e))
    except BaseException:
        close(main, art)
        raise
    return main, art


@pytest.mark.parametrize("node_cols,d,n,art_bound,n_ge,n_eq,want", ASSEMBLY)
def test_node_assembly_equals_the_models_build_bit_for_bit(node_cols, d, n, art_bound, n_ge, n_eq, want):
    base = B.assembly_base(node_cols, d, art_bound, n_ge, n_eq, seed=node_cols + d)
    entries = B.assembly_nodes(100 * d + n, d, n, want)
    kinds = {sbb.GeneralFormSingle(B.to_problem(lp, base)).kind[int(v[1:])] for e in entries for v, _, _ in e}
    assert n < 65 or kinds == {0, 1, 2}                      # positive, negative and signed variables branch
    n_art = int(art_bound) + n_ge + n_eq + want
    main, art = check_nodes(base, entries)
    try:
        assert (main.n_lps, main.cols) == (n, node_cols) and (art is None) == (n_art == 0)
        if art:
            assert art.cols == node_cols + n_art and art.rows == main.rows
        is_max = base["type"] == "max"                       # every member starts MI_RUNNING: one call ends each
        st = (art.solve_two_phase(main, is_max, 1024, B.PIVOT_CAP) if art else main.solve(is_max, 1024, B.PIVOT_CAP))[0]
        for q in range(min(n, 3)):
            assert int(st[q]) == B.solve_node(base, entries[q])[0], q
    finally:
        close(main, art)


def test_a_group_that_fails_the_guard_is_declined():
    g = sbb.GeneralFormSingle(B.to_problem(lp, B.guard_case()))
    b = sbb.Base(g)
    try:
        with pytest.raises(capi.Mi355xError) as e:
            b.create_nodes([(("y", 0, 3),)], form="global")
        assert e.value.code == capi.MI_UNSUPPORTED
    finally:
        b.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_tall_case_is_built_the_node_row_pass_has_no_lds_limit(depth):
    """The global form's node row pass keeps two counts per thread in static LDS and the rows' words in device memory:
    nothing of it grows with m or d, so tall_case (203 x 205 and more) is built.  The LDS entry declines it."""
    base = B.tall_case()
    entries = [(("x", 0, 2),), (("y", 0, 1),)] if depth == 1 else [(("x", 1, 1), ("y", 0, 2)), (("y", 1, 1), ("x", 0, 3))]
    want = B.build_node(base, entries[0])
    assert want[0].shape == (202 + depth, 204 + depth)
    close(*check_nodes(base, entries))
    b = sbb.Base(sbb.GeneralFormSingle(B.to_problem(lp, base)))
    try:
        with pytest.raises(capi.Mi355xError) as e:
            b.create_nodes(entries)
        assert e.value.code == capi.MI_UNSUPPORTED
    finally:
        b.close()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("depth", [1, 2])
def test_nodes_of_a_base_beyond_the_budget(depth, two_phase, threads):
    """200 rows over three integer variables (z free): node tableaux 201 + d x 205 + d."""
    base = G.big_bb_problem(two_phase)
    entries = G.big_bb_nodes(depth)
    want = B.build_node(base, entries[0])
    assert want[0].shape == (201 + depth, 205 + depth) and (want[2] is not None) == (two_phase or depth == 2)
    main, art = check_nodes(base, entries, threads)
    try:
        is_max = base["type"] == "max"
        st = (art.solve_two_phase(main, is_max, 1024, B.PIVOT_CAP) if art else main.solve(is_max, 1024, B.PIVOT_CAP))[0]
        for q, e in enumerate(entries):
            wst, M, basis, _ = B.solve_node(base, e)
            assert int(st[q]) == wst, q
            if wst == sc.OPTIMAL:
                G_, gb = main.download(q)
                assert same_bits(G_, M) and np.array_equal(gb, basis), q
    finally:
        close(main, art)


def _same_incumbent(d, t, want):
    assert isinstance(t, lp.SingleTableau)
    assert same_bits(t.matrix, want.M) and np.array_equal(t.basis_columns, want.basis)
    for v in d["vars"]:
        got = lp.tableau_variable(t, v)
        assert isinstance(got, F32) and same_bits(np.array([got]), np.array([want.values[v]])), v
    assert same_bits(np.array([lp.tableau_objective_value(t)]), np.array([want.objective]))


@pytest.mark.parametrize("two_phase", [False, True])
def test_search_beyond_the_budget_equals_the_model(two_phase, monkeypatch):
    d, want = G.big_bb_search(two_phase)
    seen = []
    real = sbb.DeviceRounds._batches

    def spy(self, entries, form="lds"):
        made = real(self, entries, form)
        seen.append((form, len(entries), made is not None, None if made is None else made[0].info()["form"]))
        return made
    monkeypatch.setattr(sbb.DeviceRounds, "_batches", spy)
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 2
    s = sbb.SingleBranchAndBound(B.to_problem(lp, d), width=4, max_pivots=B.PIVOT_CAP, beyond_lds=True)
    t = s.run()
    assert B.same_trace(s.trace(), want.trace)
    _same_incumbent(d, t, want)
    st = s.stats()
    assert st["processed"] == len(want.trace) and st["max_depth"] == want.depth
    lds = [x for x in seen if x[0] == "lds"]
    assert lds and not any(x[2] for x in lds)                # every group is beyond the LDS budget
    assert [x[1:] for x in seen if x[0] == "global"] == [(x[1], True, 3) for x in lds if x[1] >= 2]
    assert st["global_batched"] == sum(x[1] for x in lds if x[1] >= 2) > 0
    assert st["one_by_one"] == sum(x[1] for x in lds if x[1] < 2)            # only the rounds smaller than the hook
    assert st["host_built"] == 0 and st["declined"] == 0
    assert st["global_batched"] + st["one_by_one"] == st["solved"] - 1

    del seen[:]
    s0 = sbb.SingleBranchAndBound(B.to_problem(lp, d), width=4, max_pivots=B.PIVOT_CAP)
    t0 = s0.run()
    assert B.same_trace(s0.trace(), want.trace) and B.same_trace(s0.trace(), s.trace())
    _same_incumbent(d, t0, want)
    assert s0.stats()["global_batched"] == 0 and s0.stats()["one_by_one"] == s0.stats()["solved"] - 1
    assert not [x for x in seen if x[0] == "global"]


def test_public_call_passes_the_keyword_through():
    d, want = G.big_bb_search(False)
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 2
    t = lp.mi355x_simplex_solver(B.to_problem(lp, d), precision="single", branch_and_bound=True, bb_width=4,
                                 max_pivots=B.PIVOT_CAP, beyond_lds=True)
    _same_incumbent(d, t, want)
