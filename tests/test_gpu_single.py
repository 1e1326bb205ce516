"""The single-float path on the GPU (kernels_single.inc behind mi355x_stab_*) against the float32 model of
tests/single_cases.py: status, pivot trace, basis and EVERY entry of the final tableau bit for bit (any NaN equals
any NaN: its payload is the hardware's choice), in both forms -- the select / update pair and the LDS-resident
solve -- and through the public function.  Every solve carries a finite cap.

Shapes (m x n): 24 x 40 and 61 x 97 (cols = 1 and 3 mod 4) in both forms; the largest m x 300 that fits the LDS
budget mi355x_stab_info reports and the first that does not; 130 x 203 (several workgroups of k_s_update in both
grid dimensions, a row tail); 1030 x 5 (1031 rows: the gather's second batch of the 1024-thread select); 3 x 33001
(33004 columns: the second trip of pricing and of row scaling).

On the parent commit every test here fails: there is no mi355x_stab_* symbol, and precision="single" is swallowed
by the solver's **_ignored, so that the double path answers (1e-6 after one pivot where the single-float path
returns 0 after none)."""
import numpy as np
import pytest

from tests import single_cases as sc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
F32 = np.float32
CAP = 2000                                                   # every model solve here ends far below it
AUTO, PAIR, LDS = 0, 1, 2


@pytest.fixture(autouse=True)
def _form_back_to_auto():
    yield
    lp.single.set_form(AUTO)


same_bits = sc.same_bits


def tableau(M0, b0, is_max):
    return lp.SingleTableau(None, lp.Problem(type="max" if is_max else "min"), np.array(M0, dtype=F32), b0,
                            M0.shape[1] - 1, M0.shape[0] - 1, {})


def run(M0, b0, is_max, form, cap=CAP, chunk=None, factor=1024):
    lp.single.set_form(form)
    t = tableau(M0, b0, is_max)
    t.fp_tolerance_factor = factor
    st, n = lp.single.solve_status(t, max_pivots=cap, chunk=chunk)
    return st, n, [tuple(x) for x in t.pivot_trace().tolist()], t.matrix, t.basis_columns, t.info()["form"]


def check(got, want, form=None):
    st, n, trace, G, bg, took = got
    wst, wtrace, M, b = want
    assert st == wst and n == len(wtrace)
    assert trace == [tuple(x) for x in wtrace]
    assert np.array_equal(bg, b)
    assert same_bits(G, M)
    if form is not None:
        assert took == form


@pytest.mark.parametrize("m,n", [(24, 40), (61, 97)])
def test_both_forms_and_auto_agree_with_the_model(m, n):
    M0, b0, st, tr, M, b = sc.solved_synthetic(n, m)
    assert st == sc.OPTIMAL and len(tr) > 5 and (n + m + 1) % 4 in (1, 3)
    check(run(M0, b0, True, PAIR), (st, tr, M, b), PAIR)
    check(run(M0, b0, True, LDS), (st, tr, M, b), LDS)
    check(run(M0, b0, True, AUTO), (st, tr, M, b), LDS)


def _lds_bytes(m, n):
    rows, cols = m + 1, n + m + 1
    ldl = (cols + 3) // 4 * 4
    return 4 * (rows * ldl + ldl + (rows + 3) // 4 * 4)


def test_lds_budget_boundary():
    """The largest m x 300 that fits the budget mi355x_stab_info reports takes the LDS form, the next one the pair."""
    M0, b0, *_ = sc.solved_synthetic(40, 24)
    budget = tableau(M0, b0, True).info()["lds_budget"]
    assert 150 * 1024 <= budget <= 160 * 1024 - 1024
    m = max(k for k in range(1, 400) if _lds_bytes(k, 300) <= budget)
    assert _lds_bytes(m + 1, 300) > budget and m >= 90
    for mm, form in ((m, LDS), (m + 1, PAIR)):
        M0, b0, st, tr, M, b = sc.solved_synthetic(300, mm)
        assert st == sc.OPTIMAL and len(tr) > 20
        check(run(M0, b0, True, AUTO), (st, tr, M, b), form)


@pytest.mark.parametrize("m,n", [(130, 203), (1030, 5), (3, 33001)])
def test_pair_shapes(m, n):
    M0, b0, st, tr, M, b = sc.solved_synthetic(n, m)
    assert st == sc.OPTIMAL and len(tr) >= 5
    check(run(M0, b0, True, AUTO), (st, tr, M, b), PAIR)


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_min_problems(form):
    M0, b0, st, tr, M, b = sc.solved_synthetic(40, 24, is_max=False)
    assert st == sc.OPTIMAL and tr == sc.solved_synthetic(40, 24)[3]
    check(run(M0, b0, False, form), (st, tr, M, b), form)


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_chunks_of_five_pivots_equal_one_call(form):
    M0, b0, st, tr, M, b = sc.solved_synthetic(97, 61)
    assert len(tr) > 12
    check(run(M0, b0, True, form, chunk=5), (st, tr, M, b), form)


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_max_pivots_is_honoured_exactly(form):
    M0, b0, st, tr, M, b = sc.solved_synthetic(97, 61, cap=7)
    assert st == sc.MAX_PIVOTS and len(tr) == 7
    check(run(M0, b0, True, form, cap=7), (st, tr, M, b), form)


def test_stepwise_pieces_equal_solve():
    M0, b0, st, tr, M, b = sc.solved_synthetic(40, 24)
    t = tableau(M0, b0, True)
    steps = []
    for _ in range(CAP):
        ec = lp.single.find_entering_column(t)
        if ec is None:
            break
        cr = lp.single.find_pivoting_row(t, ec)
        assert cr is not None
        lp.single.n_pivot_row(t, ec, cr)
        steps.append((ec, cr))
    assert steps == [tuple(x) for x in tr]
    assert same_bits(t.matrix, M) and np.array_equal(t.basis_columns, b)
    assert [tuple(x) for x in t.pivot_trace().tolist()] == steps


# ---- exact ties: integer-valued float32 tableaux, ties across lane 63/64 and thread 1023/1024
@pytest.mark.parametrize("form", [PAIR, LDS])
@pytest.mark.parametrize("is_max", [True, False])
def test_ties_at_wave_boundaries_lowest_index_wins(form, is_max):
    M0, b0 = sc.tie_tableau(150, 70, tied_cols=(63, 64, 130), tied_rows=(31, 63, 64), is_max=is_max)
    st, tr, M, b = sc.solve(M0, b0, is_max, cap=40)
    assert tr[0] == (63, 31)
    check(run(M0, b0, is_max, form, cap=40), (st, tr, M, b), form)


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_ties_at_the_1024_thread_boundary(form):
    """Pricing: tied columns 4095 / 4096 (quads 1023 / 1024: the last thread of the first batch and the first of the
    second); ratio test: tied rows 1023 / 1024 -- in the 1024-thread select and in the 1024-thread LDS solve."""
    # (the pair takes its 1024-thread select from 8192 floats per row on; 4 x 8304 floats do not fit the LDS budget)
    M0, b0 = sc.tie_tableau(8300 if form == PAIR else 4200, 3, tied_cols=(4095, 4096), tied_rows=(1, 2))
    st, tr, M, b = sc.solve(M0, b0, True, cap=10)
    assert tr[0] == (4095, 1)
    check(run(M0, b0, True, form, cap=10), (st, tr, M, b), form)
    # (1101 rows with their slack columns are 4.9 MB: the LDS form gets the tableau without them)
    M0, b0 = sc.tie_tableau(6, 1100, tied_cols=(2, 4), tied_rows=(1023, 1024), slack=form == PAIR)
    st, tr, M, b = sc.solve(M0, b0, True, cap=10)
    assert tr[0] == (2, 1023) and len(tr) >= 2
    check(run(M0, b0, True, form, cap=10), (st, tr, M, b), form)


# ---- overflow: inf, then a NaN in the objective row; the trace follows the scan-order rules
@pytest.mark.parametrize("form", [PAIR, LDS])
def test_overflow_case(form):
    M0, b0 = sc.overflow_tableau()
    st, tr, M, b = sc.solve(M0, b0, True, cap=20)
    assert np.isnan(M[-1]).any() and np.isinf(M).any()
    check(run(M0, b0, True, form, cap=20), (st, tr, M, b), form)


# ---- two-phase
def _two_phase_device(A0, ab0, M0, mb0, main_is_max, form, chunk=None):
    lp.single.set_form(form)
    art, main = tableau(A0, ab0, False), tableau(M0, mb0, main_is_max)
    st, npv = lp.single.solve_status([art, main], max_pivots=CAP, chunk=chunk)
    return st, npv, art, main


def _check_two_phase(A0, ab0, M0, mb0, main_is_max, form, chunk=None):
    want = sc.two_phase(A0, ab0, M0, mb0, main_is_max)
    st, npv, art, main = _two_phase_device(A0, ab0, M0, mb0, main_is_max, form, chunk)
    assert st == want["status"] and npv == (want["n1"], want["n2"])
    assert [tuple(x) for x in art.pivot_trace().tolist()] == [tuple(x) for x in want["art_trace"]]
    assert [tuple(x) for x in main.pivot_trace().tolist()] == [tuple(x) for x in want["main_trace"]]
    assert same_bits(art.matrix, want["A"]) and np.array_equal(art.basis_columns, want["abasis"])
    assert same_bits(main.matrix, want["M"]) and np.array_equal(main.basis_columns, want["mbasis"])
    return want


def _golden_problem(golden, name):
    p = golden["cases"][name]["problem"]

    def cv(x):
        return x if isinstance(x, int) or x is None else F32(x)
    return dict(type=p["type"], vars=p["vars"], objective_var=p["objective_var"],
                objective=[(v, cv(c)) for v, c in p["objective"]],
                bounds=[(b[0], cv(b[1]), cv(b[2])) for b in p["bounds"]],
                constraints=[(op, [(v, cv(c)) for v, c in e], cv(r)) for op, e, r in p["constraints"]])


def _lp_problem(d):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[(b[0], (b[1], b[2])) for b in d["bounds"]],
                      constraints=list(d["constraints"]))


@pytest.mark.parametrize("form", [PAIR, LDS])
@pytest.mark.parametrize("name", ["numerical_issue", "variable_bounds_bug"])
def test_two_phase_goldens(golden, name, form):
    d = _golden_problem(golden, name)
    built = sc.build(d)
    tabs = lp.build_tableau_single(_lp_problem(d))
    if built["art"] is None:                                 # (variable_bounds_bug: the shifted row turns into a `<=`)
        assert isinstance(tabs, lp.SingleTableau) and same_bits(tabs.matrix, built["main"][0])
        st, tr, M, b = sc.solve(built["main"][0], built["main"][1], d["type"] == "max")
        check(run(built["main"][0], built["main"][1], d["type"] == "max", form), (st, tr, M, b), form)
    else:
        assert same_bits(tabs[0].matrix, built["art"][0]) and same_bits(tabs[1].matrix, built["main"][0])
        _check_two_phase(built["art"][0], built["art"][1], built["main"][0], built["main"][1], d["type"] == "max", form)
    lp.single.set_form(form)
    sol = lp.solve_problem(_lp_problem(d), precision="single", max_pivots=CAP)
    want = sc.solve_problem(d)
    assert same_bits(sol.matrix, want["M"])
    for v in d["vars"]:
        got = lp.solution_variable(sol, v)
        assert isinstance(got, np.float32) and got.tobytes() == sc.variable(want["M"], want["basis"], want["mapping"], v).tobytes()
    z = lp.solution_objective_value(sol)
    assert isinstance(z, np.float32)
    if name == "numerical_issue":                            # t/integration.lisp:72-80, in single-float
        assert abs(F32(z - F32(0.9372585))) <= F32(F32(16) * sc.EPS_S)
    else:
        assert lp.solution_variable(sol, "x") == 1 and lp.solution_variable(sol, "y") == 1


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_two_phase_drive_out_pivot(form):
    """Phase 1 makes no pivot and leaves an artificial basic at zero: the hand-over's forced pivot drives it out."""
    b = sc.build(sc.DRIVEOUT_LP)
    assert sc.solve(b["art"][0], b["art"][1], False)[1] == []
    want = _check_two_phase(b["art"][0], b["art"][1], b["main"][0], b["main"][1], True, form)
    assert want["status"] == sc.OPTIMAL and want["n1"] == 1 and want["n2"] >= 1


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_two_phase_infeasible(form):
    b = sc.build(sc.INFEASIBLE_LP)
    want = _check_two_phase(b["art"][0], b["art"][1], b["main"][0], b["main"][1], True, form)
    assert want["status"] == sc.INFEASIBLE
    with pytest.raises(lp.InfeasibleProblemError):
        lp.solve_problem(_lp_problem(sc.INFEASIBLE_LP), precision="single", max_pivots=CAP)


@pytest.mark.parametrize("form", [PAIR, LDS])
@pytest.mark.parametrize("name", ["5x9", "5x9-driveout"])
def test_two_phase_handover_bases_that_are_not_unit_columns(name, form):
    from tests import handover_cases as hc
    case = hc.CASES[name]
    for a in (case.art, case.main):
        assert np.array_equal(a.astype(F32).astype(np.float64), a)          # converts to float32 exactly
    _check_two_phase(case.art.astype(F32), case.art_basis, case.main.astype(F32), case.main_basis, True, form, chunk=3)


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_two_phase_ends_art_stuck(form):
    """The host's step between the phases run to MI_ART_STUCK: the artificial of row 3 is basic at zero and the only
    non-zero main entries of its row sit in basic columns."""
    from tests import handover_cases as hc
    case = hc.CASES["5x9-stuck"]
    for a in (case.art, case.main):
        assert np.array_equal(a.astype(F32).astype(np.float64), a)          # converts to float32 exactly
    want = _check_two_phase(case.art.astype(F32), case.art_basis, case.main.astype(F32), case.main_basis, True, form)
    assert want["status"] == sc.ART_STUCK and (want["n1"], want["n2"]) == (0, 0)


@pytest.mark.parametrize("form", [PAIR, LDS])
def test_two_phase_ends_art_nonzero(form):
    """... and to MI_ART_NONZERO: 1e-6 x >= 1e-5 ends phase 1 inside f eps with the artificial still basic at a
    level that is no exact zero."""
    want = _check_two_phase(*sc.small_pairs()[4], True, form)
    assert want["status"] == sc.ART_NONZERO and want["n2"] == 0


# ---- through the public function
def test_tiny_coefficient_through_the_public_function():
    """max 1e-6 x s.t. x <= 1: the single-float pricing threshold is 7.6e-6, so the path makes 0 pivots and returns
    0; the double path (what the parent commit answers with, the keyword swallowed) pivots once and returns 1e-6."""
    d = sc.tiny_coefficient_problem()
    want = sc.solve_problem(d)
    assert want["pivots"] == 0 and sc.objective(want["M"]) == 0
    sol = lp.solve_problem(_lp_problem(d), precision="single", max_pivots=CAP)
    z = lp.solution_objective_value(sol)
    assert isinstance(sol, lp.SingleTableau) and sol.n_pivots == 0
    assert isinstance(z, np.float32) and z == F32(0)
    assert lp.solution_variable(sol, "x") == F32(0)
    dbl = lp.solve_problem(_lp_problem(dict(d, objective=[("x", float(F32(1e-6)))])), max_pivots=CAP)
    assert lp.solution_objective_value(dbl) == float(F32(1e-6))


def test_overflow_through_the_public_function():
    d = dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", 4), ("y", 1), ("z", 2)], bounds=[],
             constraints=[("<=", [("x", F32(0.5)), ("y", F32(3e38)), ("z", F32(0.1))], 1),
                          ("<=", [("x", 1), ("y", 1), ("z", 2)], 4), ("<=", [("y", 1), ("z", 1)], 3)])
    b = sc.build(d)
    assert same_bits(b["main"][0], sc.overflow_tableau()[0])
    want = sc.solve_problem(d)
    sol = lp.solve_problem(_lp_problem(d), precision="single", max_pivots=CAP)
    assert same_bits(sol.matrix, want["M"]) and np.array_equal(sol.basis_columns, want["basis"])
    assert [tuple(x) for x in sol.pivot_trace().tolist()] == [tuple(x) for x in want["trace"]]


def test_epsilon_and_info():
    L = lp.capi.lib()
    assert L.mi355x_epsilon_single() == float(sc.EPS_S) == 5.960465188081798e-08
    M0, b0, *_ = sc.solved_synthetic(40, 24)
    info = tableau(M0, b0, True).info()
    assert (info["rows"], info["cols"]) == M0.shape and info["ld"] % 32 == 0 and info["ld"] >= info["cols"]
