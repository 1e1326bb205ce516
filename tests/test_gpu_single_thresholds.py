"""The three single-float thresholds at the edge, mid-solve, on every single-float path: entries bitwise AT (f/8) eps_s,
0 + (f/2) eps_s and f eps_s and one float beyond them (tests/single_threshold_cases.py; its conditions, and that the
cases tell seven wrong models from the right one, are asserted on the model alone in
tests/test_single_threshold_cases_host.py), under the factors 1024, 16, 2^20, 1000 (all three products round in
float) and 1000.3 (no float32: the library must round the factor first), max and min.

Against the float32 model of tests/single_cases.py: status, pivot count(s), whole trace(s), basis and EVERY entry of
the final tableau(x) bit for bit -- no tolerance anywhere.  Every solve carries a finite cap.  The form that ran is
read back from info(): `form` of a single tableau (1 the select / update pair, 2 the LDS solve), `workgroup_threads`
of a batch.  The pair takes k_s_select<1024> beyond a leading dimension of 8192 floats or 1024 rows (3 x 8300 and
1100 x 6 with slack columns) and k_s_select<256> below (300 x 6, 61 x 97, 96 x 300)."""
import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_threshold_cases as C
from tests.helpers import lp_amd
from tests.single_gpu_checks import (AUTO, LDS, PAIR, check_batch, check_single, check_two_phase_batch,
                                     check_two_phase_single, tableau)

pytestmark = pytest.mark.gpu
lp = lp_amd()
F32 = np.float32
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_form(AUTO)
    lp.single.set_batch_threads(0)
    lp.single.set_batch_launch_cap(0)


# ------------------------------------------------------------------ one tableau: the pair and the LDS solve
@pytest.mark.parametrize("spec", C.PAIR_256, ids=C.spec_id)
def test_pair_with_the_256_thread_select(spec):
    """k_s_select<256> + k_s_update.  T at 301 rows: R = 290 is thread 34's second row, the winner lies in the first
    trip; at 61 x 97 and 96 x 300 the event falls 20 to 30 pivots in.  P: `!(e.v < 0.0f - price_tol)` on the block's
    winner after every other key has gone, under sgn = +1 and -1."""
    assert spec.m + 1 <= 1024 and spec.n + spec.m + 1 <= 8192 - 32
    check_single(C.planted(spec).case, PAIR, factor=spec.f)


@pytest.mark.parametrize("spec", C.PAIR_1024, ids=C.spec_id)
def test_pair_with_the_1024_thread_select(spec):
    """k_s_select<1024> + k_s_update.  T at 1101 rows: R = 1090 is the second trip of the gather; P at 8304 floats per
    row: Y = 8200 is quad 2050, the third trip of pricing."""
    assert spec.m + 1 > 1024 or spec.n + spec.m + 1 > 8192
    check_single(C.planted(spec).case, PAIR, factor=spec.f)


@pytest.mark.parametrize("spec,chunk", C.LDS_CASES, ids=["%s%s" % (C.spec_id(s), "-chunk%d" % c if c else "") for s, c in C.LDS_CASES])
def test_lds_solve(spec, chunk):
    """k_s_solve: the whole loop in one workgroup, the tableau in LDS (1101 rows without slack columns; 4204 floats per
    row: Y = 4100 on the second trip).  chunk = 5: the event step is the first after the tableau came back from HBM and
    was loaded again."""
    check_single(C.planted(spec).case, LDS, chunk=chunk, factor=spec.f)


# ------------------------------------------------------------------ the step-wise pieces
@pytest.mark.parametrize("spec", C.STEPWISE, ids=C.spec_id)
def test_stepwise_pieces_along_the_trace(spec):
    """k_s_price_only and k_s_ratio_only (their own launchers compute the thresholds again from the tableau's factor)
    walked along the model's trace with n_pivot_row, every answer compared, up to and including the event step."""
    p = C.planted(spec)
    M0, b0, is_max, cap, (wst, wtrace, _, _) = p.case
    t = tableau(M0, b0, is_max, spec.f)
    M, b = np.array(M0), np.array(b0)
    for k in range(p.j + 1):
        ec = lp.single.find_entering_column(t)
        assert ec == sc.price(M, is_max, spec.f), k
        if ec is None:
            break
        cr = lp.single.find_pivoting_row(t, ec)
        assert cr == sc.ratio(M, ec, spec.f), k
        if cr is None:
            break
        assert (ec, cr) == wtrace[k], k
        lp.single.n_pivot_row(t, ec, cr)
        sc.pivot(M, b, ec, cr)
        assert same_bits(t.matrix, M) and np.array_equal(t.basis_columns, b), k
    if spec.ev == "T":                                       # the event step was taken: on R (`beyond`) or on the base's row
        assert k == p.j and (ec, cr) == (p.X, p.R if spec.var == "beyond" else p.w)
    else:                                                    # the walk ended at step k_end: nothing enters / no row
        assert k == p.j == len(wtrace) and (ec, wst) == ((None, sc.OPTIMAL) if spec.var == "at" else (p.Y, sc.UNBOUNDED))


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("launch_cap", [0, 4])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("shape", sorted(C.BATCHES), ids=lambda s: "%dx%d" % s[:2])
def test_batches_under_one_factor(shape, threads, launch_cap):
    """k_sb_solve<256|1024>: members of one shape under ONE factor per call -- T-at, T-beyond in row 0, T-beyond in the
    last row, P-at, P-beyond, two untouched ones, T-at in row 0 (3 x 4200: the P members; 1100 x 6 without slack
    columns: the T members).  The events fall at different steps, so that workgroups of one launch decide differently;
    launch_cap = 4 carries the planted entries through HBM between launches."""
    check_batch(C.batch_cases(*shape), threads, launch_cap, factor=C.BATCHES[shape][1])


# ------------------------------------------------------------------ the feasibility threshold
@pytest.mark.parametrize("form", [PAIR, LDS])
@pytest.mark.parametrize("f", C.PAIR_FACTORS)
@pytest.mark.parametrize("name", C.F_NAMES)
def test_feasibility_threshold_single(name, f, form):
    """tp_feasible<float> with single_thresholds(f).feasible in mi355x_stab_solve_two_phase: |0 - objective| bitwise at
    f eps_s hands over and solves the main tableau, one float beyond ends INFEASIBLE with the main tableau untouched."""
    check_two_phase_single(*C.pair_case(name, f), form, None, factor=f)


@pytest.mark.parametrize("per_call", [2000, 3])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("f", C.PAIR_FACTORS)
def test_feasibility_threshold_batch(f, threads, per_call):
    """k_sb_between<256|1024>'s own copy of the feasibility test: F at and beyond with both signs beside an ordinary
    member, and the Q members, whose phase 1 pivots under min and then meets +ptol in the artificial batch (sgn = -1 in
    k_sb_solve: `at` hands over, `beyond` ends phase 1 UNBOUNDED)."""
    check_two_phase_batch([C.pair_case(name, f) for name in C.BETWEEN_MEMBERS], threads, per_call, factor=f)


# ------------------------------------------------------------------ the public routes: the factor reaches the kernels
def _lp_problem(d):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[], constraints=list(d["constraints"]))


def _edge(route):
    f = dict(C.PUBLIC)[route]
    ds = [C.edge_problem(f, var) for var in ("at", "beyond")]
    return f, ds, [sc.solve_problem(d, f) for d in ds]


def _check_solution(sol, want):
    assert isinstance(sol, lp.SingleTableau) and sol.n_pivots == want["pivots"]
    assert same_bits(sol.matrix, want["M"]) and np.array_equal(sol.basis_columns, want["basis"])
    z = lp.solution_objective_value(sol)
    assert isinstance(z, np.float32) and z.tobytes() == sc.objective(want["M"]).tobytes()
    x = lp.solution_variable(sol, "x")
    assert x.tobytes() == sc.variable(want["M"], want["basis"], want["mapping"], "x").tobytes()


def test_solve_problem_passes_the_factor_on():
    """max c x, x <= 1 with c bitwise the pricing threshold of f = 16: 0 pivots; one float above: one pivot."""
    f, ds, wants = _edge("solve_problem")
    for d, want in zip(ds, wants):
        _check_solution(lp.solve_problem(_lp_problem(d), precision="single", fp_tolerance=f, max_pivots=C.CAP), want)


def test_solve_problems_passes_the_factor_on():
    """The two problems are one group: a SingleBatch under f = 1000.3, which the library rounds to a float first."""
    f, ds, wants = _edge("solve_problems")
    sols = lp.solve_problems([_lp_problem(d) for d in ds], precision="single", fp_tolerance=f, max_pivots=C.CAP)
    for sol, want in zip(sols, wants):
        _check_solution(sol, want)


def test_solve_lps_single_passes_the_factor_on():
    """The array front end: rows in column space, the tableaux built on the device, f = 1000."""
    f, ds, wants = _edge("solve_lps_single")
    L = np.array([[[1, 1], [-d["objective"][0][1], 0]] for d in ds], dtype=F32)
    assert all(same_bits(np.array([[L[q, 0, 0], 1, L[q, 0, 1]], [L[q, 1, 0], 0, 0]], dtype=F32), sc.build(d)["main"][0])
               for q, d in enumerate(ds))
    st, npv, rhs, obj_rows, bases = lp.solve_lps_single(L, np.zeros((2, 1), dtype=np.int32), is_max=True, fp_tolerance=f,
                                                        max_pivots=C.CAP)
    for q, want in enumerate(wants):
        assert int(st[q]) == want["status"] and int(npv[q]) == want["pivots"], q
        assert same_bits(rhs[q], want["M"][:, -1]) and same_bits(obj_rows[q], want["M"][-1]), q
        assert np.array_equal(bases[q], want["basis"]), q
