"""The GLOBAL form of a batch of single-float LPs on the GPU (kernels_single_global.inc behind
mi355x_sbatch_create_global: one workgroup per member, the member's tableau left in HBM) against the float32 model of
tests/single_cases.py, member by member: status, pivot counts, whole trace, basis and EVERY entry of the final tableau
bit for bit (sc.same_bits: any NaN equals any NaN), no tolerance anywhere.  Every case runs with the workgroup forced to
256 and to 1024 threads.

Shapes: 99 x 399 (the first shape the LDS form declines), 257 x 769 (512 x 256: cols = 1 mod 4, ld 800), 1101 x 1107
(several row trips per thread) and 131 x 1161 (several quad trips per row); the boundary cases of the LDS form (ties,
NaN rules, extremes, subnormals, thresholds), which the global form takes as well; more members than the device holds at
once; two-phase pairs of 102 x 405 / 102 x 402 and 111 x 423 / 111 x 411; cancel; the public route
solve_problems(..., precision="single", beyond_lds=True).

On the parent commit every test here fails: mi355x_sbatch_create_global and `beyond_lds` do not exist."""
import functools

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_edge_cases as E
from tests import single_threshold_cases as C
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
F32 = np.float32
CAP = 2000                                                   # every model solve here ends far below it
THREADS = [256, 1024]
LDS_BUDGET = 156 * 1024
CUS = 256                                                    # compute units of an MI355X
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)
    lp.single.set_batch_global_threads(0)
    lp.single.set_batch_launch_cap(0)
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = None


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def make_global(Ms, bs, threads, launch_cap=0):
    lp.single.set_batch_global_threads(threads)
    lp.single.set_batch_launch_cap(launch_cap)
    sb = lp.SingleBatch.from_arrays(np.stack(Ms), np.stack(bs), form="global")
    info = sb.info()
    rows, cols = Ms[0].shape
    assert info["form"] == 3 and info["workgroup_threads"] == threads and info["n_lps"] == len(Ms)
    assert (info["rows"], info["cols"]) == (rows, cols) and info["ld"] % 32 == 0 and info["ld"] >= cols
    # pivot row + column snapshot, each rounded up to a quad: nothing of the tableau
    assert info["lds_bytes_per_member"] == 4 * ((cols + 3) // 4 * 4 + (rows + 3) // 4 * 4)
    assert info["members_per_cu"] >= 1
    return sb


def check_members(sb, st, npv, wants):
    """wants: per member the model's (status, trace, M, basis)."""
    assert len(wants) == sb.n_lps
    for q, (wst, wtrace, M, b) in enumerate(wants):
        assert int(st[q]) == wst and int(npv[q]) == len(wtrace), (q, int(st[q]), int(npv[q]), wst, len(wtrace))
        assert _pairs(sb.trace(q).tolist()) == _pairs(wtrace), q
        G, gb = sb.download(q)
        assert np.array_equal(gb, b), q
        assert same_bits(G, M), q


def check_cases(cases, threads, launch_cap, factor=1024):
    """tests/single_gpu_checks.py's check_batch through the global form: the cases (one shape, one sense, one cap) as
    the members of one batch."""
    is_max, cap = cases[0][2], cases[0][3]
    assert all(c[2] == is_max and c[3] == cap and c[0].shape == cases[0][0].shape for c in cases)
    sb = make_global([c[0] for c in cases], [c[1] for c in cases], threads, launch_cap)
    try:
        st, npv = sb.solve(is_max, factor, cap)
        assert sb.last_return == capi.MI_OK
        check_members(sb, st, npv, [(c[4][0], c[4][1], c[4][2], c[4][3]) for c in cases])
    finally:
        sb.close()


def solve_in_calls(sb, is_max, per_call):
    """Calls of `per_call` pivots until no member is left at MI_MAX_PIVOTS -> (status, pivots summed)."""
    total = np.zeros(sb.n_lps, dtype=np.int64)
    for _ in range(CAP):
        st, npv = sb.solve(is_max, 1024, per_call)
        assert sb.last_return == capi.MI_OK
        total += npv
        if not (st == capi.MI_MAX_PIVOTS).any():
            return st, total
    raise AssertionError("the batch did not finish")


# ------------------------------------------------------------------ shared inputs and the model's answers (computed once)
@functools.lru_cache(maxsize=None)
def synth(n, m, seeds=(1, 2), is_max=True):
    ins, wants = [], []
    for seed in seeds:
        M0, b0 = sc.synthetic(n, m, seed=seed)
        if not is_max:
            M0 = M0.copy()
            M0[-1] = -M0[-1]                                 # the mirrored objective row: the same pivots
        want = sc.solve(M0, b0, is_max, 1024, 0)
        for a in (M0, b0) + tuple(want[2:]):
            a.setflags(write=False)
        ins.append((M0, b0))
        wants.append(want)
    return ins, wants


def _run(ins, is_max, threads, launch_cap=0):
    sb = make_global([M for M, _ in ins], [b for _, b in ins], threads, launch_cap)
    st, npv = sb.solve(is_max, 1024, CAP)
    assert sb.last_return == capi.MI_OK
    return sb, st, npv


# ------------------------------------------------------------------ 1. just past the budget
@pytest.mark.parametrize("threads", THREADS)
def test_just_past_the_lds_budget(threads):
    ins, wants = synth(300, 98)
    assert ins[0][0].shape == (99, 399)
    assert [(w[0], len(w[1])) for w in wants] == [(sc.OPTIMAL, 48), (sc.OPTIMAL, 51)]
    with pytest.raises(capi.Mi355xError) as declined:        # the LDS form still declines the shape
        lp.SingleBatch.from_arrays(np.stack([M for M, _ in ins]), np.stack([b for _, b in ins]))
    assert declined.value.code == capi.MI_UNSUPPORTED
    sb, st, npv = _run(ins, True, threads)
    assert sb.info()["form"] == 3 and sb.info()["lds_bytes_per_member"] == 4 * (400 + 100) < LDS_BUDGET // 50
    check_members(sb, st, npv, wants)
    rhs, obj, basis = lp.single_bb.readback(sb)              # mi355x_sbatch_readback works on either form
    for q, (_, _, M, b) in enumerate(wants):
        assert same_bits(rhs[q], M[:, -1]) and same_bits(obj[q], M[-1]) and np.array_equal(basis[q], b), q


# ------------------------------------------------------------------ 2. config 4's shape
@pytest.mark.parametrize("threads", THREADS)
def test_config_4_shape_in_one_call(threads):
    ins, wants = synth(512, 256)
    assert ins[0][0].shape == (257, 769)
    assert [(w[0], len(w[1])) for w in wants] == [(sc.OPTIMAL, 167), (sc.OPTIMAL, 104)]
    sb, st, npv = _run(ins, True, threads)
    assert sb.info()["ld"] == 800
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_config_4_shape_in_calls_of_seven_pivots(threads):
    ins, wants = synth(512, 256)
    sb = make_global([M for M, _ in ins], [b for _, b in ins], threads)
    st, npv = sb.solve(True, 1024, 7)
    assert st.tolist() == [capi.MI_MAX_PIVOTS] * 2 and npv.tolist() == [7, 7]
    st, more = solve_in_calls(sb, True, 7)
    check_members(sb, st, npv + more, wants)


@pytest.mark.parametrize("threads", THREADS)
def test_config_4_shape_under_a_launch_cap_of_five(threads):
    ins, wants = synth(512, 256)
    sb, st, npv = _run(ins, True, threads, launch_cap=5)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ 3. tall and wide
@pytest.mark.parametrize("threads", THREADS)
def test_tall_members(threads):
    """1101 x 1107: 277 quads per row, several row trips per thread in the update and two trips of the column gather
    at 1024 threads."""
    ins, wants = synth(6, 1100, seeds=(1,))
    assert ins[0][0].shape == (1101, 1107) and (wants[0][0], len(wants[0][1])) == (sc.OPTIMAL, 8)
    sb, st, npv = _run(ins, True, threads)
    check_members(sb, st, npv, wants)


@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("threads", THREADS)
def test_wide_members(threads, is_max):
    """131 x 1161: 291 quads per row (several quad trips per row at 256 threads); the mirrored `min` form as well."""
    ins, wants = synth(1030, 130, seeds=(1,), is_max=is_max)
    assert ins[0][0].shape == (131, 1161) and (wants[0][0], len(wants[0][1])) == (sc.OPTIMAL, 77)
    assert _pairs(wants[0][1]) == _pairs(synth(1030, 130, seeds=(1,))[1][0][1])
    sb, st, npv = _run(ins, is_max, threads)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ 4. the LDS form's boundary cases, through the new loop
@functools.lru_cache(maxsize=None)
def tie_cases(n, m, ties, slack=True):
    cases = []
    for tied_cols, tied_rows in ties:
        M0, b0 = sc.tie_tableau(n, m, tied_cols=tied_cols, tied_rows=tied_rows, slack=slack)
        want = sc.solve(M0, b0, True, cap=10)
        assert _pairs(want[1])[0] == (tied_cols[0], tied_rows[0]) and len(want[1]) >= 2
        cases.append((M0, b0, True, 10, (want[0], _pairs(want[1]), want[2], want[3])))
    return cases


@pytest.mark.parametrize("threads", THREADS)
def test_ties_in_pricing_3x1100(threads):
    """Quads 63 | 64 (the wave boundary) and 255 | 256 (the trip boundary at 256 threads)."""
    check_cases(tie_cases(1100, 3, (((255, 256), (1, 2)), ((1023, 1024), (0, 2)))), threads, 0)


@pytest.mark.parametrize("threads", THREADS)
def test_ties_in_pricing_3x4200(threads):
    check_cases(tie_cases(4200, 3, (((4095, 4096), (1, 2)), ((1023, 1024, 4096), (0, 1)))), threads, 0)


@pytest.mark.parametrize("threads", THREADS)
def test_ties_between_rows_300x6(threads):
    check_cases(tie_cases(6, 300, (((2, 4), (63, 64)), ((2, 4), (255, 256))), slack=False), threads, 0)


@pytest.mark.parametrize("threads", THREADS)
def test_overflow_member_beside_an_ordinary_one(threads):
    Mo, bo = sc.overflow_tableau()
    Mn, bn = sc.synthetic(3, 3, seed=5)
    wants = [sc.solve(Mo, bo, True, cap=20), sc.solve(Mn, bn, True, cap=20)]
    assert np.isnan(wants[0][2][-1]).any() and np.isinf(wants[0][2]).any() and np.isfinite(wants[1][2]).all()
    ins = [(Mo, bo), (Mn, bn)]
    for order in ([0, 1], [1, 0]):
        sb = make_global([ins[k][0] for k in order], [ins[k][1] for k in order], threads)
        st, npv = sb.solve(True, 1024, 20)
        check_members(sb, st, npv, [wants[k] for k in order])


@pytest.mark.parametrize("launch_cap", [0, 4])
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("is_max", [True, False])
def test_pricing_nan_rules(is_max, threads, launch_cap):
    check_cases([E.pricing_case(name, 4200, is_max) for name in E.PRICING], threads, launch_cap)


@pytest.mark.parametrize("launch_cap", [0, 4])
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("rows", [1100, 300])
def test_ratio_nan_rules(rows, threads, launch_cap):
    check_cases([E.ratio_case(name, rows) for name in E.RATIO], threads, launch_cap)


@pytest.mark.parametrize("launch_cap", [0, 4])
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("shape", [(24, 40), (61, 97)])
def test_extreme_and_subnormal_members(shape, threads, launch_cap):
    cases = [E.extreme_case(*shape, k) for k in range(len(E.EXTREME[shape]))]
    if shape == (61, 97):
        cases += [E.subnormal_case(*shape, e) for e in E.SUBNORMAL_EXPONENTS]
    check_cases(cases, threads, launch_cap)


@pytest.mark.parametrize("launch_cap", [0, 4])
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("shape", sorted(C.BATCHES), ids=lambda s: "%dx%d" % s[:2])
def test_thresholds_under_one_factor(shape, threads, launch_cap):
    check_cases(C.batch_cases(*shape), threads, launch_cap, factor=C.BATCHES[shape][1])


@functools.lru_cache(maxsize=None)
def many_small(n):
    return synth(7, 5, seeds=tuple(range(1, n + 1)))


@pytest.mark.parametrize("threads", THREADS)
def test_more_members_than_the_device_holds_at_once(threads):
    probe = make_global(*zip(*synth(7, 5, seeds=(1,))[0]), threads)
    per_cu = probe.info()["members_per_cu"]
    probe.close()
    n = max(1100, per_cu * CUS + 52)
    ins, wants = many_small(2100)
    assert n <= 2100 and ins[0][0].shape == (6, 13)
    counts = {len(w[1]) for w in wants[:n]}
    assert all(w[0] == sc.OPTIMAL for w in wants[:n]) and min(counts) >= 1 and len(counts) > 5
    sb, st, npv = _run(ins[:n], True, threads)
    check_members(sb, st, npv, wants[:n])


# ------------------------------------------------------------------ 5. two-phase beyond the budget
@functools.lru_cache(maxsize=None)
def beyond_pairs(k, seeds=(1, 2, 3)):
    """sc.synthetic(300, 98, seed)'s `<=` rows and objective as a max problem, plus the rows x_j >= 0.125 for j < k."""
    pairs, wants = [], []
    names = ["x%d" % j for j in range(300)]
    for seed in seeds:
        M0, _ = sc.synthetic(300, 98, seed=seed)
        cons = [("<=", [(names[j], M0[i, j]) for j in range(300)], M0[i, 398]) for i in range(98)]
        cons += [(">=", [(names[j], 1)], F32(0.125)) for j in range(k)]
        b = sc.build(dict(type="max", vars=names, objective=[(names[j], F32(-M0[98, j])) for j in range(300)],
                          bounds=[], constraints=cons))
        pair = (b["art"][0], b["art"][1], b["main"][0], b["main"][1])
        pairs.append(pair)
        wants.append(sc.two_phase(*pair, True))
    return pairs, wants


def check_two_phase(pairs, wants, threads, per_call):
    lp.single.set_batch_global_threads(threads)
    ab = lp.SingleBatch.from_arrays(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), form="global")
    mb = lp.SingleBatch.from_arrays(np.stack([p[2] for p in pairs]), np.stack([p[3] for p in pairs]), form="global")
    try:
        assert ab.info()["form"] == 3 and mb.info()["form"] == 3
        assert ab.info()["workgroup_threads"] == threads and mb.info()["workgroup_threads"] == threads
        total = np.zeros((len(pairs), 2), dtype=np.int64)
        for _ in range(CAP):
            st, npv = ab.solve_two_phase(mb, True, 1024, per_call)
            assert ab.last_return == capi.MI_OK and npv.shape == (len(pairs), 2)
            total += npv
            if not (st == capi.MI_MAX_PIVOTS).any():
                break
        else:
            raise AssertionError("the pair did not finish")
        for q, w in enumerate(wants):
            assert int(st[q]) == w["status"], (q, int(st[q]), w["status"])
            assert total[q].tolist() == [len(w["art_trace"]), w["n2"]], (q, total[q].tolist())
            assert _pairs(ab.trace(q).tolist()) == _pairs(w["art_trace"]), q
            assert _pairs(mb.trace(q).tolist()) == _pairs(w["main_trace"]), q
            A, abasis = ab.download(q)
            M, mbasis = mb.download(q)
            assert same_bits(A, w["A"]) and np.array_equal(abasis, w["abasis"]), q
            assert same_bits(M, w["M"]) and np.array_equal(mbasis, w["mbasis"]), q
    finally:
        ab.close()
        mb.close()


@pytest.mark.parametrize("per_call", [CAP, 5])
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("k,shapes", [(3, ((102, 405), (102, 402))), (12, ((111, 423), (111, 411)))])
def test_two_phase_beyond_the_budget(k, shapes, threads, per_call):
    pairs, wants = beyond_pairs(k)
    assert (pairs[0][0].shape, pairs[0][2].shape) == shapes
    assert all(w["status"] == sc.OPTIMAL and len(w["art_trace"]) == k and 45 <= w["n2"] <= 66 for w in wants)
    check_two_phase(pairs, wants, threads, per_call)


@pytest.mark.parametrize("per_call", [CAP, 3])
@pytest.mark.parametrize("threads", THREADS)
def test_two_phase_small_members_of_every_outcome(threads, per_call):
    pairs = sc.small_pairs()
    wants = [sc.two_phase(A, ab, M, mb, True) for A, ab, M, mb in pairs]
    assert [w["status"] for w in wants] == [sc.OPTIMAL, sc.INFEASIBLE, sc.OPTIMAL, sc.UNBOUNDED, sc.ART_NONZERO]
    check_two_phase(pairs, wants, threads, per_call)


def test_a_pair_of_one_lds_and_one_global_handle_is_declined():
    pairs = sc.small_pairs()
    A, abasis, M, mbasis = (np.stack([p[k] for p in pairs]) for k in range(4))
    for art_form, main_form in (("lds", "global"), ("global", "lds")):
        ab = lp.SingleBatch.from_arrays(A, abasis, form=art_form)
        mb = lp.SingleBatch.from_arrays(M, mbasis, form=main_form)
        with pytest.raises(capi.Mi355xError) as err:
            ab.solve_two_phase(mb, True, 1024, CAP)
        assert err.value.code == capi.MI_BAD_ARG
        ab.close()
        mb.close()


# ------------------------------------------------------------------ 6. cancel
@pytest.mark.parametrize("threads", THREADS)
def test_cancel_before_a_call(threads):
    ins, wants = synth(300, 98)
    sb = make_global([M for M, _ in ins], [b for _, b in ins], threads, launch_cap=4)
    sb.cancel()
    st, npv = sb.solve(True, 1024, CAP)
    assert sb.last_return == capi.MI_CANCELLED
    assert st.tolist() == [capi.MI_RUNNING] * 2 and npv.tolist() == [4] * 2              # whole pivots only
    st, more = sb.solve(True, 1024, CAP)
    assert sb.last_return == capi.MI_OK
    check_members(sb, st, npv + more, wants)


# ------------------------------------------------------------------ 7. the public route
def _problem_of(M0, n, m, kind="max"):
    """The LP a synthetic tableau [A | I | b ; -c | 0 | 0] is built from (its numbers are float32 values); kind="min":
    min -c'x, the mirrored problem."""
    names = ["x%d" % j for j in range(n)]
    sign = F32(-1) if kind == "max" else F32(1)
    return lp.Problem(type=kind, vars=names, objective_var="z",
                      objective_func=[(names[j], F32(sign * M0[m, j])) for j in range(n)],
                      constraints=[("<=", [(names[j], M0[i, j]) for j in range(n)], M0[i, n + m]) for i in range(m)])


def _same_result(g, w, k):
    if isinstance(w, Exception):
        assert type(g) is type(w) and g.args == w.args, k
        return
    assert isinstance(g, lp.SingleTableau) and g.matrix.dtype == np.float32, k
    assert same_bits(g.matrix, w.matrix) and np.array_equal(g.basis_columns, w.basis_columns), k
    assert g.n_pivots == w.n_pivots and g.n_pivots > 0, k


def _spies(monkeypatch):
    made, alone = [], []
    real_make, real_alone = lp.SingleBatch.from_arrays, lp.single.solve_single

    def from_arrays(matrices, basis, device=0, **kw):
        sb = real_make(matrices, basis, device=device, **kw)
        made.append((kw.get("form", "lds"), sb.n_lps, sb.rows, sb.cols))
        return sb

    def solve_single(problem, **kw):
        alone.append(problem)
        return real_alone(problem, **kw)
    monkeypatch.setattr(lp.SingleBatch, "from_arrays", staticmethod(from_arrays))
    monkeypatch.setattr(lp.single, "solve_single", solve_single)
    return made, alone


def test_public_route_on_a_mixed_list(monkeypatch):
    big = [_problem_of(sc.synthetic(300, 98, seed=s)[0], 300, 98) for s in (1, 2, 3)]
    big_min = _problem_of(sc.synthetic(300, 98, seed=4)[0], 300, 98, kind="min")
    small = [_problem_of(sc.synthetic(40, 24, seed=s)[0], 40, 24) for s in (1, 2)]
    integer = lp.Problem(type="max", vars=["x", "y"], objective_var="z", objective_func=[("x", 1), ("y", 1)],
                         constraints=[("<=", [("x", 1), ("y", 2)], 4), ("<=", [("x", 3), ("y", 1)], 6)], integer_vars=["x"])
    ps = [big[0], small[0], big_min, big[1], integer, small[1], big[2]]
    want = lp.solve_problems(ps, precision="single", errorp=False, max_pivots=CAP)
    assert isinstance(want[4], lp.UnsupportedConstraintError)
    for k, (M0, b0) in ((0, sc.synthetic(300, 98, seed=1)), (3, sc.synthetic(300, 98, seed=2))):      # the model's answer
        st, tr, M, b = sc.solve(M0, b0, True, cap=CAP)
        assert same_bits(want[k].matrix, M) and want[k].n_pivots == len(tr)

    made, alone = _spies(monkeypatch)
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 2
    got = lp.solve_problems(ps, precision="single", beyond_lds=True, errorp=False, max_pivots=CAP)
    assert sorted(made) == [("global", 3, 99, 399), ("lds", 2, 25, 65)]
    assert [p is q for p, q in zip(alone, [integer, big_min])] == [True, True]
    assert len(got) == len(ps)
    for k, (g, w) in enumerate(zip(got, want)):
        _same_result(g, w, k)

    del made[:], alone[:]
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 4                   # three members are too few now: one by one, as without
    got = lp.solve_problems(ps, precision="single", beyond_lds=True, errorp=False, max_pivots=CAP)
    assert made == [("lds", 2, 25, 65)] and len(alone) == 5
    for k, (g, w) in enumerate(zip(got, want)):
        _same_result(g, w, k)


def test_public_route_places_an_unbounded_members_condition():
    Ms = [sc.synthetic(300, 98, seed=s)[0].copy() for s in (1, 2, 3)]
    Ms[1][:98, 0] = -Ms[1][:98, 0]                           # nothing bounds x0, whose objective coefficient is positive
    ps = [_problem_of(M, 300, 98) for M in Ms]
    lp.single.GLOBAL_BATCH_MIN_MEMBERS = 2
    want = lp.solve_problems(ps, precision="single", errorp=False, max_pivots=CAP)
    got = lp.solve_problems(ps, precision="single", beyond_lds=True, errorp=False, max_pivots=CAP)
    assert isinstance(got[1], lp.conditions.UnboundedProblemError)
    for k, (g, w) in enumerate(zip(got, want)):
        _same_result(g, w, k)
    with pytest.raises(lp.conditions.UnboundedProblemError):
        lp.solve_problems(ps, precision="single", beyond_lds=True, max_pivots=CAP)
