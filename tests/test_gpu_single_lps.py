"""Single-float batches built on the device from problem rows (k_slp_assemble behind mi355x_sbatch_create_lps,
single_lps.py) against the float32 model of tests/single_cases.py: what a member starts from -- every entry, sign of
zero included, both bases, zero padding -- and what it ends with -- status, pivot counts per phase, traces, final
basis and every final entry.  build_tableau_single / solve_problems_single are second witnesses; nothing is compared
with the new route's own output.

Every member that is not built for the host route must take the device route: each test asserts
group_lowered_rows_single's host dictionary exactly.

The largest two-phase m x 300: with every row artificial and carrying a slack column the artificial tableau is
(m + 1) x (300 + 2 m + 1); single_lds_bytes gives 159 456 bytes at m = 83 (84 x 467 stored as 84 x 468, plus the pivot
row and the column snapshot) against the budget of 159 744, and 162 720 at m = 84: 83 x 300 is built and solved, 84 x
300 is declined.

On the parent commit every test here fails: there is no single_lps module and no mi355x_sbatch_create_lps symbol."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_lps_cases as C
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
F32 = np.float32
THREADS = [256, 1024]
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)


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


def create(ds, threads=0):
    lp.single.set_batch_threads(threads)
    main, art = lp.SingleBatch.from_lps(*lowered(ds))
    for sb in (main, art):
        if sb is not None:
            info = sb.info()
            assert info["n_lps"] == len(ds) and info["ld"] % 32 == 0 and info["ld"] >= info["cols"]
            assert (info["rows"], info["cols"]) == (sb.rows, sb.cols) and info["members_per_cu"] >= 1
            assert info["lds_bytes_per_member"] == C.lds_bytes(sb.rows, sb.cols)
            assert threads == 0 or info["workgroup_threads"] == threads
    return main, art


def stored(sb, q):
    """Member q as stored: rows x ld, the padding columns included."""
    ld = ctypes.c_int64(0)
    L = capi.lib()
    assert L.mi355x_sbatch_debug_stored(sb._handle, q, None, ctypes.byref(ld)) == capi.MI_OK
    out = np.full((sb.rows, ld.value), np.nan, dtype=F32)
    assert L.mi355x_sbatch_debug_stored(sb._handle, q, out.ctypes.data_as(ctypes.c_void_p), None) == capi.MI_OK
    return out


def check_assembly(ds):
    """Every member before any solve: both tableaux and both bases are the model's build, the padding is +0.0."""
    main, art = create(ds)
    try:
        for q, d in enumerate(ds):
            want = sc.build(d)
            assert (art is None) == (want["art"] is None), q
            for sb, built in ((main, want["main"]), (art, want["art"])):
                if sb is None:
                    continue
                M, basis = built
                G, gb = sb.download(q)
                assert same_bits(G, M), q
                assert np.array_equal(gb, basis), q
                S = stored(sb, q)
                assert same_bits(S[:, :sb.cols], M), q
                assert not S[:, sb.cols:].view(np.uint32).any(), q
        return main.cols, (None if art is None else art.cols)
    finally:
        main.close()
        if art is not None:
            art.close()


# ------------------------------------------------------------------ 1. the assembly alone
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
        # the negated rows hold +0.0 for integer zeros, for what is not mentioned and in the other rows' slack columns
        M = sc.build(ds[0])["main"][0]
        assert (M[2, [1, 2]] == 0).all() and not np.signbit(M[2, [1, 2]]).any() and M[2, -1] == 3
        assert np.signbit(M[0, -1]) and M[0, -1] == 0        # -0.0 stays: the row is not negated


def test_assembly_of_extreme_rows():
    """k_slp_assemble / assemble_member_lds on coefficients near FLT_MAX and below FLT_MIN: the artificial objective
    row is the float sum in INCREASING row order (3e38 + 3e38 - 3e38 = inf, any other order 3e38; 1 + 2**-24 + 2**-24
    = 1, the other way round 1 + 2**-23), a row with a subnormal negative right-hand side is negated exactly (no
    flush) and its sense flipped, a right-hand side -0.0 is not."""
    ds = C.extreme_rows_group()
    assert check_assembly(ds) == (9, 12)
    main, art = create(ds)
    try:
        got = [(art.download(q)[0][-1, 0], art.download(q)[0][-1, 1]) for q in range(3)]
        assert got == [(F32(np.inf), F32(1)), (C.BIG, F32(1)), (C.BIG, F32(1 + 2.0 ** -23))]
        for q in range(3):
            M = main.download(q)[0]
            assert M[3, -1].view(np.uint32) == C.SUB.view(np.uint32)
            assert M[3, 3].view(np.uint32) == F32(3e-39).view(np.uint32)
            assert M[4, -1] == 0 and np.signbit(M[4, -1])
    finally:
        main.close()
        art.close()


@pytest.mark.parametrize("kw,cols", [(dict(main_cols=32), (32, None)), (dict(main_cols=33), (33, None)),
                                     (dict(art_cols=64), (54, 64)), (dict(art_cols=65), (55, 65))])
def test_assembly_at_the_steps_of_the_leading_dimension(kw, cols):
    assert check_assembly(C.ld_step_group(**kw)) == cols


def test_assembly_96x300_single_phase_pair():
    assert check_assembly(C.big_group(False)) == (397, None)


def test_assembly_83x300_two_phase_pair_and_84x300_declined():
    m = C.BIG_TWO_PHASE_M
    assert C.fits(m + 1, 300 + 2 * m + 1) and not C.fits(m + 2, 300 + 2 * (m + 1) + 1)
    assert check_assembly(C.big_group(True)) == (300 + m + 1, 300 + 2 * m + 1)
    L, sense, sums = lowered(C.big_group(True))
    L2 = np.concatenate([L[:, :1], L], axis=1)               # one more `>=` row: m = 84
    s2 = np.concatenate([sense[:, :1], sense], axis=1)
    with pytest.raises(capi.Mi355xError) as e:
        lp.SingleBatch.from_lps(L2, s2, sums)
    assert e.value.code == capi.MI_UNSUPPORTED


# ------------------------------------------------------------------ 2. solves
def solve_group(ds, wants, threads, per_call=0):
    main, art = create(ds, threads)
    n = len(ds)
    is_max = ds[0]["type"] == "max"
    try:
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
            G, gb = main.download(q)
            assert same_bits(G, w["M"]) and np.array_equal(gb, w["mbasis"]), q
            if art is not None:
                assert _pairs(art.trace(q).tolist()) == _pairs(w["art_trace"]), q
                A, ab = art.download(q)
                assert same_bits(A, w["A"]) and np.array_equal(ab, w["abasis"]), q
        assert total.shape == ((n,) if art is None else (n, 2))
    finally:
        main.close()
        if art is not None:
            art.close()


SOLVED = {"outcome": (C.outcome_group, ()), "driveout": (C.driveout_group, ()), "single_phase": (C.single_phase_group, ()),
          "medium_max": (C.medium_group, ("max",)), "medium_min": (C.medium_group, ("min",)),
          "moving": (C.moving_group, ()), "zero_rhs": (C.zero_rhs_group, ()), "extreme_rows": (C.extreme_rows_group, ())}


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("name", sorted(SOLVED))
def test_solves_from_device_built_members(name, threads):
    fn, args = SOLVED[name]
    wants = C.model_solution(fn, *args)
    if name == "outcome":
        assert [w["status"] for w in wants] == C.OUTCOMES
    if name == "driveout":                                   # no phase-1 pivot: the one pivot counted is the drive-out
        assert all(w["status"] == sc.OPTIMAL and w["n"][0] == 1 for w in wants)
        assert all(len(sc.solve(w["build"]["art"][0], w["build"]["art"][1], False)[1]) == 0 for w in wants)
    if name == "single_phase":
        assert [w["status"] for w in wants] == [sc.OPTIMAL, sc.OPTIMAL, sc.UNBOUNDED] and all(len(w["n"]) == 1 for w in wants)
    if name == "extreme_rows":                               # phase 1 pivots with inf and NaN in its objective row
        assert all(w["status"] == sc.INFEASIBLE and w["n"][0] >= 1 for w in wants)
        assert not any(np.isfinite(w["A"][-1]).all() for w in wants)
        assert np.isnan(wants[0]["A"][-1, -1])               # (fp= 0 NaN) in the step between the phases
    if name.startswith("medium"):
        assert all(w["status"] == sc.OPTIMAL and min(w["n"]) > 0 for w in wants)
    solve_group(fn(*args), wants, threads)


@pytest.mark.parametrize("threads", THREADS)
def test_solves_in_calls_of_three_pivots(threads):
    solve_group(C.medium_group(), C.model_solution(C.medium_group), threads, per_call=3)
    solve_group(C.driveout_group(), C.model_solution(C.driveout_group), threads, per_call=1)


def test_solves_of_the_largest_shapes():
    for two_phase in (False, True):
        solve_group(C.big_group(two_phase), C.model_solution(C.big_group, two_phase), 0)


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
    for v in r.problem.vars:
        a, b = lp.tableau_variable(r, v), lp.tableau_variable(w, v)
        assert type(a) is np.float32 and type(b) is np.float32 and a.view(np.uint32) == b.view(np.uint32)
    assert type(lp.tableau_objective_value(r)) is np.float32
    assert lp.tableau_objective_value(r).view(np.uint32) == lp.tableau_objective_value(w).view(np.uint32)


def test_list_route_in_chunks_equals_the_uncapped_run_and_the_model():
    ds = C.medium_group()
    wants = C.model_solution(C.medium_group)
    ps = [C.to_problem(lp, d) for d in ds]
    assert lp.group_lowered_rows_single(ps)[0] == {}
    whole = lp.solve_problems_single_from_rows(ps)
    chunked = lp.solve_problems_single_from_rows(ps, chunk=3)
    for r, r3, w in zip(whole, chunked, wants):
        assert same_bits(r.matrix, w["M"]) and np.array_equal(r.basis_columns, w["mbasis"]) and r.n_pivots == w["n"]
        _same_result(r3, r)
    capped = lp.solve_problems_single_from_rows(ps, max_pivots=4, errorp=False)
    for r, w in zip(capped, lp.single.solve_problems_single(ps, max_pivots=4, errorp=False)):
        _same_result(r, w)


# ------------------------------------------------------------------ 3. the list route on a mixed list
def _mixed_list():
    out, dr, sp = C.outcome_group(), C.driveout_group(), C.single_phase_group()
    ds = [sp[0], C.float_zero_member(), dr[0], C.integer_sum_member(), sp[1], out[0], C.lone_member(), C.declined_member(),
          dr[1], out[1], sp[2], out[2], out[3], dr[2]]
    ps = [C.to_problem(lp, d) for d in ds]
    ps.insert(5, C.to_problem(lp, sp[2], integer_vars=["x"]))
    return ps


@pytest.mark.parametrize("errorp", [False, True])
def test_list_route_on_a_mixed_list(errorp, monkeypatch):
    ps = _mixed_list()
    host, groups = lp.group_lowered_rows_single(ps)
    declined = host.pop(8)
    assert isinstance(declined, lp.UnsupportedConstraintError) and declined.args[0] == ("single", 0.1)
    assert host == {1: "float zero", 3: "integer sum", 5: "integer variables", 7: "alone"}
    assert sorted(sorted(k for k, _ in v) for v in groups.values()) == [[0, 4, 11], [2, 9, 14], [6, 10, 12, 13]]
    calls = {"from_lps": 0, "solve_single": 0}
    real_from_lps, real_solve_single = lp.SingleBatch.from_lps.__func__, lp.single_lps.solve_single

    def from_lps(cls, *a, **kw):
        calls["from_lps"] += 1
        return real_from_lps(cls, *a, **kw)

    def solve_single(*a, **kw):
        calls["solve_single"] += 1
        return real_solve_single(*a, **kw)
    monkeypatch.setattr(lp.SingleBatch, "from_lps", classmethod(from_lps))
    monkeypatch.setattr(lp.single_lps, "solve_single", solve_single)
    if errorp:
        with pytest.raises(lp.SolverError) as e:
            lp.solve_problems_single_from_rows(ps, errorp=True)
        assert calls == {"from_lps": 3, "solve_single": 4}
        with pytest.raises(lp.SolverError) as w:
            lp.single.solve_problems_single(ps, errorp=True)
        assert type(e.value) is type(w.value) and e.value.args == w.value.args
        return
    got = lp.solve_problems_single_from_rows(ps, errorp=False)
    assert calls == {"from_lps": 3, "solve_single": 4}       # three groups on the device; members 1, 3, 5, 7 one by one
    want = lp.single.solve_problems_single(ps, errorp=False)
    for r, w in zip(got, want):
        _same_result(r, w)
    assert isinstance(got[5], lp.UnsupportedConstraintError) and got[5].args[0][0] == "integer"
    assert isinstance(got[8], lp.UnsupportedConstraintError) and got[8].args[0] == ("single", 0.1)
    for ks, fn in (((6, 10, 12, 13), C.outcome_group), ((2, 9, 14), C.driveout_group), ((0, 4, 11), C.single_phase_group)):
        for k, w in zip(ks, C.model_solution(fn)):
            assert isinstance(got[k], lp.SingleTableau if w["status"] == sc.OPTIMAL else lp.SolverError), k
    assert isinstance(got[6], lp.InfeasibleProblemError) and isinstance(got[12], lp.UnboundedProblemError)
    # ... and the model's answer for the members the device built
    for k, w in zip((6, 10, 12, 13), C.model_solution(C.outcome_group)):
        if w["status"] == sc.OPTIMAL:
            assert same_bits(got[k].matrix, w["M"]) and got[k].n_pivots == w["n"]
    for k, w in zip((2, 9, 14), C.model_solution(C.driveout_group)):
        assert same_bits(got[k].matrix, w["M"]) and np.array_equal(got[k].basis_columns, w["mbasis"])
        assert got[k].n_pivots == w["n"]
    # the float-zero member went one by one and kept Lisp's -0.0
    first = sc.build(C.float_zero_member())["main"][0]
    assert np.signbit(first[0, 1]) and same_bits(lp.build_tableau_single(ps[1])[1].matrix, first)


# ------------------------------------------------------------------ 4. the guard at the C entry
def test_from_lps_declines_integer_sums_beyond_2_to_24_and_leaves_no_handle():
    low = lp.single_lps.lower_problem_rows_single(C.to_problem(lp, C.integer_sum_member()))
    L, s, sums = np.stack([low.L] * 2), np.stack([low.sense] * 2), np.stack([low.col_int_sum] * 2)
    with pytest.raises(capi.Mi355xError) as e:
        lp.SingleBatch.from_lps(L, s, sums)
    assert e.value.code == capi.MI_UNSUPPORTED
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    p = [a.ctypes.data_as(ctypes.c_void_p) for a in (L, s, sums)]
    rc = capi.lib().mi355x_sbatch_create_lps(ctypes.byref(hm), ctypes.byref(ha), 2, 3, 2, p[0], p[1], p[2], 0)
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value
    assert b"member 0" in capi.lib().mi355x_last_error()
    # without the sums the entry cannot know: it builds the float running sum, which is NOT the model's
    main, art = lp.SingleBatch.from_lps(L, s, None)
    try:
        assert art.download(0)[0][-1, 0] == F32(2 ** 24) and sc.build(C.integer_sum_member())["art"][0][-1, 0] == F32(2 ** 24 + 2)
    finally:
        main.close()
        art.close()
    with pytest.raises(capi.Mi355xError) as e:
        lp.solve_lps_single(L, s, int_mask=np.ones(L.shape, dtype=bool))
    assert e.value.code == capi.MI_UNSUPPORTED


# ------------------------------------------------------------------ 5. the array front end
@pytest.mark.parametrize("name", ["outcome", "driveout", "single_phase", "medium_min"])
def test_solve_lps_single_reads_back_what_the_model_ends_with(name):
    fn, args = SOLVED[name]
    ds, wants = fn(*args), C.model_solution(fn, *args)
    L, sense, _ = lowered(ds)
    mask = L == np.round(L)                                  # (more than Lisp's integers: the sums stay far below 2^24)
    for int_mask in (None, mask):
        st, npv, rhs, obj_rows, bases = lp.solve_lps_single(L, sense, is_max=ds[0]["type"] == "max", int_mask=int_mask)
        assert rhs.dtype == np.float32 and obj_rows.dtype == np.float32 and bases.dtype == np.int64
        for q, w in enumerate(wants):
            assert int(st[q]) == w["status"] and tuple(np.atleast_1d(npv[q]).tolist()) == w["n"], q
            assert same_bits(rhs[q], w["M"][:, -1]) and same_bits(obj_rows[q], w["M"][-1]), q
            assert np.array_equal(bases[q], w["mbasis"]), q
