"""The single-float kernels on NaN, infinity and subnormal inputs at shapes with several waves, trips and workgroups
(tests/single_edge_cases.py; its conditions are asserted on the model alone in tests/test_single_edge_cases_host.py)
against the float32 model of tests/single_cases.py: status, pivot count(s), whole trace(s), basis and EVERY entry of
the final tableau(x) bit for bit -- signs of zero and subnormals included, any NaN equal to any NaN, no tolerance
anywhere.  Every solve carries a finite cap.

The form that ran is read back from info(): `form` of a single tableau (1 the select / update pair, 2 the LDS solve),
`workgroup_threads` of a batch.  The pair takes k_s_select<1024> beyond a leading dimension of 8192 floats or 1024
rows (the 8300 column and 1101 row cases) and k_s_select<256> below (the 300 row, 24 x 40, 61 x 97 and 130 x 203 cases)."""
import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_edge_cases as E
from tests.helpers import lp_amd
from tests.single_gpu_checks import (AUTO, LDS, PAIR, check_batch, check_single, check_two_phase_batch,
                                     check_two_phase_single, tableau)

pytestmark = pytest.mark.gpu
lp = lp_amd()
FORMS = [PAIR, LDS]
THREADS = [256, 1024]
LAUNCH_CAPS = [0, 4]
same_bits = sc.same_bits


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_form(AUTO)
    lp.single.set_batch_threads(0)
    lp.single.set_batch_launch_cap(0)


# ------------------------------------------------------------------ a. pricing: s_price_cand / sc_min / sc_block_min
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("name", E.PRICING)
def test_pricing_nan_rules_single(name, is_max, form):
    """s_block_price in k_s_select<1024> (the pair, 8304 floats per row) and in k_s_solve (LDS, 4204 floats: a second
    trip of 1024 threads).  P1: a NaN key is no candidate in the winner's quad, in the next lane, in the next wave and
    in the next trip, under sgn = +1 and -1 (NaN * -1), and the lowest of four tied columns wins across them.  P2: the
    `column == 0` branch of s_price_cand against -inf in another wave and trip (`s == 1` -> optimal).  P3: NaNs in
    column 0's quad mates are no candidates; -inf enters, and k_s_update / the LDS update walk carry -inf * 0 and
    x + inf through every row."""
    check_single(E.pricing_case(name, 8300 if form == PAIR else 4200, is_max), form)


@pytest.mark.parametrize("launch_cap", LAUNCH_CAPS)
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("is_max", [True, False])
def test_pricing_nan_rules_batch(is_max, threads, launch_cap):
    """k_sb_solve<256|1024>: P1, P2 and P3 (n = 4200) as the members of one batch -- at 256 threads the tied columns
    1024 and 4096 and the -inf rivals are further trips of threads 0 and 1; one member ends at once while the others
    pivot."""
    check_batch([E.pricing_case(name, 4200, is_max) for name in E.PRICING], threads, launch_cap)


# ------------------------------------------------------------------ b. ratio test: s_block_gather_ratio
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows", [1100, 300])
@pytest.mark.parametrize("name", E.RATIO)
def test_ratio_nan_rules_single(name, rows, form):
    """s_block_gather_ratio in k_s_select<1024> (1101 rows with slack columns), k_s_select<256> (301 rows) and
    k_s_solve (1024 threads, no slack columns).  R1, R4: the `__syncthreads_or(nanq)` repair -- the block-wide
    minimum of `first` across waves, the re-division, the NaN winner replacing a finite `best` (R4: inf / inf).
    R2, R2b: a thread whose own first eligible row has a NaN quotient still offers a later row of its own (`best.i <
    0` stays true past the NaN), and the repair declines (the block's first eligible row is finite).  R3: NaNs behind
    a finite first row in other waves.  Then the NaN pivot row goes through s_block_scale_row and a whole update."""
    check_single(E.ratio_case(name, rows, slack=form == PAIR), form)


@pytest.mark.parametrize("launch_cap", LAUNCH_CAPS)
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("rows", [1100, 300])
def test_ratio_nan_rules_batch(rows, threads, launch_cap):
    """k_sb_solve<256|1024>: R1 .. R4 as the members of one batch, so that workgroups of one launch take different
    branches of `__syncthreads_or(nanq)`; at 256 threads 1100 rows are five trips of the gather."""
    check_batch([E.ratio_case(name, rows) for name in E.RATIO], threads, launch_cap)


# ------------------------------------------------------------------ step-wise pieces
@pytest.mark.parametrize("n", [4200, 8300])
@pytest.mark.parametrize("is_max", [True, False])
def test_stepwise_pricing(n, is_max):
    """k_s_price_only (1024 threads: one trip and a part of the second at 4204 floats, three at 8304) on P1 .. P3, then
    k_s_ratio_only and k_s_prepare_pivot + k_s_update on the column it names."""
    for name in E.PRICING:
        M0, b0, _, cap, want = E.pricing_case(name, n, is_max)
        t = tableau(M0, b0, is_max)
        ec = lp.single.find_entering_column(t)
        assert ec == sc.price(M0, is_max), name
        if ec is None:
            continue
        cr = lp.single.find_pivoting_row(t, ec)
        assert cr == sc.ratio(M0, ec) and (ec, cr) == want[1][0], name
        lp.single.n_pivot_row(t, ec, cr)
        M, b = np.array(M0), np.array(b0)
        sc.pivot(M, b, ec, cr)
        assert same_bits(t.matrix, M) and np.array_equal(t.basis_columns, b), name


@pytest.mark.parametrize("rows,slack", [(1100, True), (1100, False), (300, True)])
def test_stepwise_ratio(rows, slack):
    """k_s_ratio_only (s_block_gather_ratio at 1024 threads: 1101 rows are a second trip, 301 rows leave waves idle) on
    R1 .. R4, then k_s_prepare_pivot and k_s_update on a pivot row that holds a NaN or an infinity."""
    for name in E.RATIO:
        M0, b0, is_max, cap, want = E.ratio_case(name, rows, slack)
        t = tableau(M0, b0, is_max)
        assert lp.single.find_entering_column(t) == 2, name
        cr = lp.single.find_pivoting_row(t, 2)
        assert cr == E.ratio_geometry(name, rows)[0], name
        lp.single.n_pivot_row(t, 2, cr)
        M, b = np.array(M0), np.array(b0)
        sc.pivot(M, b, 2, cr)
        assert same_bits(t.matrix, M) and np.array_equal(t.basis_columns, b), name


# ------------------------------------------------------------------ c, d. extreme magnitudes and subnormals
#: (shape, form): 130 x 203 is beyond the LDS budget and runs as the pair only
SHAPE_FORMS = [((24, 40), PAIR), ((24, 40), LDS), ((61, 97), PAIR), ((61, 97), LDS), ((130, 203), PAIR)]


@pytest.mark.parametrize("shape,form", SHAPE_FORMS)
def test_extreme_magnitudes_single(shape, form):
    """Eight members per shape that overflow, underflow into subnormals and meet inf - inf at different pivots:
    s_block_scale_row with an infinite or subnormal pivot, the v_div_* division on subnormal operands, k_s_update
    (130 x 203: several workgroups in both grid dimensions and a row tail, 0 * inf away from the first strip) and the
    LDS update walk across row wraps, all under the scan-order NaN rules."""
    for k in range(len(E.EXTREME[shape])):
        check_single(E.extreme_case(*shape, k), form)


@pytest.mark.parametrize("shape,form", SHAPE_FORMS[2:])
def test_subnormal_right_hand_sides_single(shape, form):
    """Denormal mode: subnormal quotients and products must be kept, not flushed, in s_block_gather_ratio's division,
    s_block_scale_row and the update (e = -130: normal inputs, subnormal results; -140: subnormal inputs; -147: the
    rounding inside the subnormal range decides the trace)."""
    for e in E.SUBNORMAL_EXPONENTS:
        check_single(E.subnormal_case(*shape, e), form, chunk=None if e != -140 else 5)


@pytest.mark.parametrize("launch_cap", LAUNCH_CAPS)
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("shape", [(24, 40), (61, 97)])
def test_extreme_and_subnormal_members_batch(shape, threads, launch_cap):
    """k_sb_solve<256|1024>: the extreme members (and at 61 x 97 the subnormal ones) of a shape as one batch; members
    meet their first non-finite value at different pivots and end at different times.  launch_cap = 4 carries NaN, inf
    and subnormal state through HBM between launches."""
    cases = [E.extreme_case(*shape, k) for k in range(len(E.EXTREME[shape]))]
    if shape == (61, 97):
        cases += [E.subnormal_case(*shape, e) for e in E.SUBNORMAL_EXPONENTS]
    check_batch(cases, threads, launch_cap)


# ------------------------------------------------------------------ e. two-phase: the step between the phases
@pytest.mark.parametrize("chunk", [None, 3])
@pytest.mark.parametrize("form", FORMS)
def test_wide_drive_out_single(form, chunk):
    """H1 through stab_handover / tp_drive_out<float> (the host's step between the phases): 604 main columns, the
    drive-outs at columns 290 and 255 with higher non-zeros behind them, column 40 basic."""
    check_two_phase_single(*E.handover_h1(0), form, chunk)


@pytest.mark.parametrize("per_call", [2000, 3])
@pytest.mark.parametrize("threads", THREADS)
def test_wide_drive_out_batch(threads, per_call):
    """k_sb_between<256|1024> beyond one trip: with 604 main columns the `flag[]` fill, the `break` + atomicMin scan
    (row 1: threads 34, 44 and 8 find 290, 300 and 520 on later trips, 290 must win; row 2: thread 255 finds 255 on
    its first trip, thread 0 finds 256 on its second), the forced pivot's prow and update loops and the copy all take
    several trips at 256 threads."""
    check_two_phase_batch([E.handover_h1(0), E.handover_h1(1)], threads, per_call)


@pytest.mark.parametrize("chunk", [None, 3])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", E.HANDOVER_SMALL)
def test_non_finite_hand_overs_single(name, form, chunk):
    """stab_handover / tp_drive_out<float> on non-finite values.  H2: `!(|0 - obj| <= tol)` on a NaN objective ->
    INFEASIBLE.  H3: `A[i][nav] != 0` on a NaN -> ART_NONZERO.  H4: an infinite `scale` in the elimination (inf - inf,
    inf * 0), phase 2 under the NaN rules."""
    check_two_phase_single(*E.handover_small(name), form, chunk)


@pytest.mark.parametrize("per_call", [2000, 3])
@pytest.mark.parametrize("threads", THREADS)
def test_non_finite_hand_overs_batch(threads, per_call):
    """k_sb_between<256|1024>: H2, H3, H4 and an ordinary member in one launch -- the three non-finite branches (the
    NaN objective, the NaN last-column entry, the infinite scale) beside a member that is handed over as usual."""
    check_two_phase_batch([E.handover_small(name) for name in E.HANDOVER_SMALL], threads, per_call)
