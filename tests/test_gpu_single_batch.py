"""Batches of single-float LPs on the GPU (kernels_single_batch.inc behind mi355x_sbatch_*) against the float32 model
of tests/single_cases.py, member by member: status, pivot count, trace, basis and EVERY entry of the final tableau bit
for bit (any NaN equals any NaN).  Every case runs with the workgroup forced to 256 and to 1024 threads.

Shapes (m x n): 24 x 40 (25 x 65, cols = 1 mod 4, 425 quads: two trips at 256 threads) and 61 x 97 (62 x 159, cols = 3
mod 4, 2480 quads: several trips at 1024); 1100 members of 5 x 7 (more members than resident workgroups); 3 x 1100 and
3 x 4200 with ties at the wave, trip and 1024-thread boundaries of pricing, 300 x 6 without slack columns with ties at
rows 63 | 64 and 255 | 256; 97 x 300, the largest m x 300 inside the LDS budget, and 98 x 300, the first outside it.

On the parent commit every test here fails: there is no mi355x_sbatch_* symbol, and solve_problems has no `precision`."""
import ctypes
import functools

import numpy as np
import pytest

from tests import single_cases as sc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
F32 = np.float32
CAP = 2000                                                   # every model solve here ends far below it
THREADS = [256, 1024]
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)
    lp.single.set_batch_launch_cap(0)


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def make_batch(Ms, bs, threads, launch_cap=0):
    lp.single.set_batch_threads(threads)
    lp.single.set_batch_launch_cap(launch_cap)
    sb = lp.SingleBatch.from_arrays(np.stack(Ms), np.stack(bs))
    info = sb.info()
    assert info["workgroup_threads"] == threads and info["n_lps"] == len(Ms) and info["members_per_cu"] >= 1
    assert (info["rows"], info["cols"]) == Ms[0].shape and info["ld"] % 32 == 0 and info["ld"] >= info["cols"]
    return sb


def solve_in_calls(sb, is_max, per_call, factor=1024):
    """Calls of `per_call` pivots until no member is left at MI_MAX_PIVOTS -> (status, pivots summed)."""
    total = np.zeros(sb.n_lps, dtype=np.int64)
    for _ in range(CAP):
        st, npv = sb.solve(is_max, factor, per_call)
        assert sb.last_return == capi.MI_OK
        total += npv
        if not (st == capi.MI_MAX_PIVOTS).any():
            return st, total
    raise AssertionError("the batch did not finish")


def check_members(sb, st, npv, wants):
    """wants: per member the model's (status, trace, M, basis)."""
    assert len(wants) == sb.n_lps
    for q, (wst, wtrace, M, b) in enumerate(wants):
        assert int(st[q]) == wst and int(npv[q]) == len(wtrace), (q, int(st[q]), int(npv[q]), wst, len(wtrace))
        assert _pairs(sb.trace(q).tolist()) == _pairs(wtrace), q
        G, gb = sb.download(q)
        assert np.array_equal(gb, b), q
        assert same_bits(G, M), q


# ------------------------------------------------------------------ shared inputs and the model's answers (computed once)
@functools.lru_cache(maxsize=None)
def synth_batch(n, m, is_max=True, cap=0, seeds=tuple(range(1, 9))):
    ins, wants = [], []
    for seed in seeds:
        M0, b0 = sc.synthetic(n, m, seed=seed)
        if not is_max:
            M0 = M0.copy()
            M0[-1] = -M0[-1]                                 # the mirrored objective row: the same pivots
        want = sc.solve(M0, b0, is_max, 1024, cap)
        for a in (M0, b0) + tuple(want[2:]):
            a.setflags(write=False)
        ins.append((M0, b0))
        wants.append(want)
    return ins, wants


def _run(ins, is_max, threads, **kw):
    sb = make_batch([M for M, _ in ins], [b for _, b in ins], threads, kw.pop("launch_cap", 0))
    st, npv = sb.solve(is_max, 1024, kw.pop("cap", CAP))
    assert sb.last_return == capi.MI_OK
    return sb, st, npv


# ------------------------------------------------------------------ members that finish at different times
@pytest.mark.parametrize("threads", THREADS)
def test_members_that_finish_at_different_times_24x40(threads):
    ins, wants = synth_batch(40, 24)
    assert ins[0][0].shape == (25, 65) and [len(w[1]) for w in wants] == [6, 13, 13, 9, 11, 13, 9, 10]
    assert all(w[0] == sc.OPTIMAL for w in wants)
    sb, st, npv = _run(ins, True, threads)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_members_that_finish_at_different_times_61x97(threads):
    ins, wants = synth_batch(97, 61)
    counts = [len(w[1]) for w in wants]
    assert ins[0][0].shape == (62, 159) and min(counts) == 15 and max(counts) == 28 and len(set(counts)) > 3
    sb, st, npv = _run(ins, True, threads)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_a_batch_of_one(threads):
    ins, wants = synth_batch(40, 24)
    sb, st, npv = _run(ins[2:3], True, threads)
    check_members(sb, st, npv, wants[2:3])


@pytest.mark.parametrize("threads", THREADS)
def test_more_members_than_resident_workgroups(threads):
    ins, wants = synth_batch(7, 5, seeds=tuple(range(1, 1101)))
    counts = {len(w[1]) for w in wants}
    assert all(w[0] == sc.OPTIMAL for w in wants) and min(counts) >= 1 and max(counts) <= 12 and len(counts) > 5
    sb, st, npv = _run(ins, True, threads)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_min_problems(threads):
    ins, wants = synth_batch(40, 24, is_max=False)
    assert [_pairs(w[1]) for w in wants] == [_pairs(w[1]) for w in synth_batch(40, 24)[1]]
    sb, st, npv = _run(ins, False, threads)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ pivot caps and continuation
@pytest.mark.parametrize("threads", THREADS)
def test_max_pivots_is_honoured_exactly_per_member(threads):
    ins, wants = synth_batch(40, 24, cap=7)
    assert [(w[0], len(w[1])) for w in wants] == [(sc.OPTIMAL, 6)] + [(sc.MAX_PIVOTS, 7)] * 7
    sb, st, npv = _run(ins, True, threads, cap=7)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_calls_of_five_pivots_equal_one_call(threads):
    ins, wants = synth_batch(40, 24)
    sb = make_batch([M for M, _ in ins], [b for _, b in ins], threads)
    st, npv = sb.solve(True, 1024, 5)
    assert st.tolist() == [capi.MI_MAX_PIVOTS] * 8 and npv.tolist() == [5] * 8
    st, more = sb.solve(True, 1024, 5)
    counts = [len(w[1]) for w in wants]                       # (the optimality test comes before the cap's)
    assert st.tolist() == [capi.MI_OPTIMAL if c <= 10 else capi.MI_MAX_PIVOTS for c in counts]
    assert more.tolist() == [min(c, 10) - 5 for c in counts] and more[0] == 1
    first = sb.download(0)
    st, rest = solve_in_calls(sb, True, 5)
    assert rest[0] == 0 and same_bits(sb.download(0)[0], first[0])          # a finished member is left as it was
    check_members(sb, st, npv + more + rest, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_launch_cap_of_four_equals_the_default(threads):
    """Launches of four pivots per member: the in-launch "still running" exit, relaunch rounds with some members
    already finished, a finished member left as it was."""
    ins, wants = synth_batch(40, 24)
    sb, st, npv = _run(ins, True, threads, launch_cap=4)
    check_members(sb, st, npv, wants)
    ins, wants = synth_batch(40, 24, cap=7)
    sb, st, npv = _run(ins, True, threads, launch_cap=4, cap=7)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ exact ties: the lowest index wins
@functools.lru_cache(maxsize=None)
def tie_batch(n, m, ties, slack=True):
    ins, wants = [], []
    for tied_cols, tied_rows in ties:
        M0, b0 = sc.tie_tableau(n, m, tied_cols=tied_cols, tied_rows=tied_rows, slack=slack)
        want = sc.solve(M0, b0, True, cap=10)
        assert _pairs(want[1])[0] == (tied_cols[0], tied_rows[0]) and len(want[1]) >= 2
        ins.append((M0, b0))
        wants.append(want)
    return ins, wants


@pytest.mark.parametrize("threads", THREADS)
def test_ties_at_the_wave_and_trip_boundaries_of_pricing(threads):
    """Quads 63 | 64 (columns 255 | 256: the wave boundary) and 255 | 256 (columns 1023 | 1024: the trip boundary at
    256 threads, a wave boundary at 1024)."""
    ins, wants = tie_batch(1100, 3, (((255, 256), (1, 2)), ((1023, 1024), (0, 2))))
    sb, st, npv = _run(ins, True, threads, cap=10)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_ties_at_the_1024_thread_boundary_of_pricing(threads):
    ins, wants = tie_batch(4200, 3, (((4095, 4096), (1, 2)), ((1023, 1024, 4096), (0, 1))))
    sb, st, npv = _run(ins, True, threads, cap=10)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_ties_between_rows(threads):
    ins, wants = tie_batch(6, 300, (((2, 4), (63, 64)), ((2, 4), (255, 256))), slack=False)
    sb, st, npv = _run(ins, True, threads, cap=10)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ NaN rules and member isolation
@pytest.mark.parametrize("threads", THREADS)
def test_overflow_member_beside_an_ordinary_one(threads):
    Mo, bo = sc.overflow_tableau()
    Mn, bn = sc.synthetic(3, 3, seed=5)
    assert Mn.shape == Mo.shape == (4, 7)
    wants = [sc.solve(Mo, bo, True, cap=20), sc.solve(Mn, bn, True, cap=20)]
    assert np.isnan(wants[0][2][-1]).any() and np.isinf(wants[0][2]).any()
    assert np.isfinite(wants[1][2]).all() and len(wants[1][1]) >= 1
    for order in ([0, 1], [1, 0]):
        ins = [(Mo, bo), (Mn, bn)]
        sb, st, npv = _run([ins[k] for k in order], True, threads, cap=20)
        check_members(sb, st, npv, [wants[k] for k in order])


# ------------------------------------------------------------------ two-phase
_hand, small_pairs = sc.hand_problem, sc.small_pairs


@functools.lru_cache(maxsize=None)
def handover_pairs(batch):
    from tests import handover_cases as hc
    out = []
    for name in hc.BATCHES[batch]:
        if name == "5x9-beyond":                             # (its artificial objective is no float32 value)
            continue
        case = hc.CASES[name]
        for a in (case.art, case.main):
            assert np.array_equal(a.astype(F32).astype(np.float64), a), name     # converts to float32 exactly
        out.append((case.art.astype(F32), case.art_basis, case.main.astype(F32), case.main_basis))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def two_phase_wants(which):
    pairs = small_pairs() if which == "small" else handover_pairs(which)
    return pairs, [sc.two_phase(A, ab, M, mb, True) for A, ab, M, mb in pairs]


def _check_two_phase_batch(which, threads, per_call):
    pairs, wants = two_phase_wants(which)
    ab = make_batch([p[0] for p in pairs], [p[1] for p in pairs], threads)
    mb = make_batch([p[2] for p in pairs], [p[3] for p in pairs], threads)
    n = len(pairs)
    total = np.zeros((n, 2), dtype=np.int64)
    for _ in range(CAP):
        st, npv = ab.solve_two_phase(mb, True, 1024, per_call)
        assert ab.last_return == capi.MI_OK and npv.shape == (n, 2)
        total += npv
        if not (st == capi.MI_MAX_PIVOTS).any():
            break
    else:
        raise AssertionError("the pair did not finish")
    for q, w in enumerate(wants):
        assert int(st[q]) == w["status"], (q, int(st[q]), w["status"])
        # (phase 1 + the drive-outs made, as mi355x_stab_solve_two_phase counts them: the artificial trace's length)
        assert total[q].tolist() == [len(w["art_trace"]), w["n2"]], (q, total[q].tolist())
        assert _pairs(ab.trace(q).tolist()) == _pairs(w["art_trace"]), q
        assert _pairs(mb.trace(q).tolist()) == _pairs(w["main_trace"]), q
        A, abasis = ab.download(q)
        M, mbasis = mb.download(q)
        assert same_bits(A, w["A"]) and np.array_equal(abasis, w["abasis"]), q
        assert same_bits(M, w["M"]) and np.array_equal(mbasis, w["mbasis"]), q
    return wants


@pytest.mark.parametrize("per_call", [CAP, 3])
@pytest.mark.parametrize("threads", THREADS)
def test_two_phase_small_members_of_every_outcome(threads, per_call):
    pairs, wants = two_phase_wants("small")
    assert all(p[0].shape == (3, 6) and p[2].shape == (3, 5) for p in pairs)
    assert [w["status"] for w in wants] == [sc.OPTIMAL, sc.INFEASIBLE, sc.OPTIMAL, sc.UNBOUNDED, sc.ART_NONZERO]
    assert len(wants[0]["art_trace"]) == 1                   # one drive-out, no phase-1 pivot
    _check_two_phase_batch("small", threads, per_call)


@pytest.mark.parametrize("per_call", [CAP, 3])
@pytest.mark.parametrize("threads", THREADS)
def test_two_phase_bases_that_are_not_unit_columns(threads, per_call):
    pairs, wants = two_phase_wants("5x9")
    assert [w["status"] for w in wants] == [sc.OPTIMAL, sc.OPTIMAL, sc.OPTIMAL, sc.ART_STUCK]
    assert len(wants[2]["art_trace"]) - len(sc.solve(pairs[2][0], pairs[2][1], False)[1]) == 2     # two drive-outs
    _check_two_phase_batch("5x9", threads, per_call)


@pytest.mark.parametrize("per_call", [CAP, 3])
@pytest.mark.parametrize("threads", THREADS)
def test_two_phase_40x70(threads, per_call):
    pairs, wants = two_phase_wants("40x70")
    assert pairs[0][0].shape == (41, 73) and pairs[0][2].shape == (41, 71)
    assert [w["status"] for w in wants] == [sc.OPTIMAL, sc.OPTIMAL, sc.UNBOUNDED]
    assert [w["n2"] for w in wants] == [55, 30, 59]
    _check_two_phase_batch("40x70", threads, per_call)


# ------------------------------------------------------------------ the LDS budget boundary
def _problem_of(M0, n, m):
    """The LP a synthetic tableau [A | I | b ; -c | 0 | 0] is built from (its numbers are float32 values)."""
    names = ["x%d" % j for j in range(n)]
    return lp.Problem(type="max", vars=names, objective_var="z",
                      objective_func=[(names[j], F32(-M0[m, j])) for j in range(n)],
                      constraints=[("<=", [(names[j], M0[i, j]) for j in range(n)], M0[i, n + m]) for i in range(m)])


def test_lds_budget_boundary():
    ins, wants = synth_batch(300, 97, seeds=(1, 2))
    assert all(w[0] == sc.OPTIMAL and len(w[1]) > 20 for w in wants)
    for threads in THREADS:
        sb, st, npv = _run(ins, True, threads)
        assert sb.info()["lds_bytes_per_member"] <= 156 * 1024 and sb.info()["members_per_cu"] == 1
        check_members(sb, st, npv, wants)
    big = [sc.synthetic(300, 98, seed=s) for s in (1, 2)]
    h = ctypes.c_void_p()
    Ms, bs = np.stack([M for M, _ in big]), np.stack([b for _, b in big])
    rc = capi.lib().mi355x_sbatch_create(ctypes.byref(h), 2, 99, 399, Ms.ctypes.data_as(ctypes.c_void_p),
                                         bs.ctypes.data_as(ctypes.c_void_p), 0)
    assert rc == capi.MI_UNSUPPORTED and not h.value
    # the public function still solves such members, one by one
    got = lp.solve_problems([_problem_of(M, 300, 98) for M, _ in big], precision="single", max_pivots=CAP)
    for g, (M0, b0) in zip(got, big):
        assert isinstance(g, lp.SingleTableau)
        st, tr, M, b = sc.solve(M0, b0, True, cap=CAP)
        assert st == sc.OPTIMAL and g.n_pivots == len(tr)
        assert same_bits(g.matrix, M) and np.array_equal(g.basis_columns, b)


# ------------------------------------------------------------------ cancel
@pytest.mark.parametrize("threads", THREADS)
def test_cancel_before_a_call(threads):
    ins, wants = synth_batch(40, 24)
    sb = make_batch([M for M, _ in ins], [b for _, b in ins], threads, launch_cap=4)
    sb.cancel()
    st, npv = sb.solve(True, 1024, CAP)
    assert sb.last_return == capi.MI_CANCELLED
    assert st.tolist() == [capi.MI_RUNNING] * 8 and npv.tolist() == [4] * 8              # whole pivots only
    st, more = sb.solve(True, 1024, CAP)
    assert sb.last_return == capi.MI_OK
    check_members(sb, st, npv + more, wants)


# ------------------------------------------------------------------ through the public function
def _lp_problem(d, integer_vars=()):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[(b[0], (b[1], b[2])) for b in d["bounds"]],
                      constraints=list(d["constraints"]), integer_vars=list(integer_vars))


def _max2(c, rhs, kind="max"):
    return dict(type=kind, vars=["x", "y"], objective_var="z", objective=[("x", c[0]), ("y", c[1])], bounds=[],
                constraints=[("<=", [("x", 1), ("y", 2)], rhs[0]), ("<=", [("x", 3), ("y", 1)], rhs[1])])


def test_public_function_on_a_mixed_list():
    tiny = sc.tiny_coefficient_problem()
    lone = dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", F32(1.5)), ("y", 1), ("z", 1)],
                bounds=[], constraints=[("<=", [("x", 1), ("y", 1), ("z", 1)], F32(2.5))])
    hand = _hand([("<=", [("x", 1), ("y", 1)], F32(3.5)), (">=", [("x", 1)], F32(0.5))], [("x", 1), ("y", F32(0.5))])
    ds = [_max2((1, F32(0.5)), (4, F32(6.5))), sc.DRIVEOUT_LP, tiny, _max2((F32(2.5), 1), (5, 7)), lone,
          _max2((1, 0.1), (4, 6)), hand, tiny, _max2((F32(0.25), 3), (F32(4.5), 6))]
    ps = [_lp_problem(d) for d in ds] + [_lp_problem(_max2((1, 1), (4, 6)), integer_vars=["x"])]
    slots, groups, groups2 = lp.single.group_single_problems(ps)
    assert sorted(len(v) for v in groups.values()) == [1, 2, 3] and [len(v) for v in groups2.values()] == [2]
    got = lp.solve_problems(ps, precision="single", errorp=False, max_pivots=CAP)
    assert len(got) == len(ps)
    assert isinstance(got[5], lp.UnsupportedConstraintError) and got[5].args[0] == ("single", 0.1)
    assert isinstance(got[9], lp.UnsupportedConstraintError) and got[9].args[0][0] == "integer"
    for k in (0, 1, 2, 3, 4, 6, 7, 8):
        alone = lp.solve_problem(ps[k], precision="single", max_pivots=CAP)
        g = got[k]
        assert isinstance(g, lp.SingleTableau) and g.matrix.dtype == np.float32, k
        assert same_bits(g.matrix, alone.matrix) and np.array_equal(g.basis_columns, alone.basis_columns), k
        assert g.n_pivots == alone.n_pivots, k
        z = lp.solution_objective_value(g)
        assert isinstance(z, np.float32) and z.tobytes() == lp.solution_objective_value(alone).tobytes()
        for v in ds[k]["vars"]:
            x = lp.solution_variable(g, v)
            assert isinstance(x, np.float32) and x.tobytes() == lp.solution_variable(alone, v).tobytes()
        want = sc.solve_problem(ds[k])
        assert same_bits(g.matrix, want["M"]) and g.n_pivots == want["pivots"], k
    # the single-float pricing threshold (7.6e-6) is above the coefficient: no pivot, 0 -- the double thresholds
    # would pivot once and return 1e-6
    for k in (2, 7):
        assert got[k].n_pivots == 0 and lp.solution_objective_value(got[k]) == F32(0)
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problems(ps, precision="single", max_pivots=CAP)
