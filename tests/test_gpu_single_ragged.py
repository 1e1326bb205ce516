"""Ragged batches of single-float LPs on the GPU (kernels_single_batch.inc over an SrView behind mi355x_sbatch_create_ragged) against
the float32 model of tests/single_cases.py, member by member: status, pivot count, trace, basis and EVERY entry of the
final tableau bit for bit (any NaN equals any NaN); no tolerance appears anywhere.  The lists are those of
tests/single_ragged_cases.py.  Every case runs with the workgroup forced to 256 and to 1024 threads, and with the
classes hook at 0 (the default: one class, the measured choice), at 1 (one class) and at 4 (up to four occupancy
classes, one launch per class).

On the parent commit every test here fails: there is no mi355x_sbatch_create_ragged and no `mixed_shapes`."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests import single_ragged_cases as rc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
F32 = np.float32
CAP = rc.CAP
same_bits = sc.same_bits
#: (workgroup threads, classes hook: 0 the default, 1 one class, 4 the occupancy classes)
MODES = [(threads, classes) for threads in (256, 1024) for classes in (0, 1, 4)]
modes = pytest.mark.parametrize("threads,classes", MODES)


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)
    lp.single.set_batch_launch_cap(0)
    lp.single.set_batch_ragged_classes(0)


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def make_ragged(ins, threads, classes, launch_cap=0):
    """ins: (M0, b0, is_max) per member, is_max None: an artificial batch (every member min)."""
    lp.single.set_batch_threads(threads)
    lp.single.set_batch_launch_cap(launch_cap)
    lp.single.set_batch_ragged_classes(classes)
    senses = [i[2] for i in ins]
    sb = lp.SingleBatch.from_ragged([i[0] for i in ins], [i[1] for i in ins], None if senses[0] is None else senses)
    info = sb.info()
    assert info["form"] == 4 and info["workgroup_threads"] == threads and info["n_lps"] == len(ins)
    assert (info["rows"], info["cols"], info["ld"]) == (0, 0, 0)
    assert info["lds_bytes_per_member"] == max(lp.single.single_lds_bytes(*i[0].shape) for i in ins)
    assert 1 <= info["members_per_cu"] <= 4
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


def _run(ins, threads, classes, cap=CAP, launch_cap=0):
    sb = make_ragged(ins, threads, classes, launch_cap)
    st, npv = sb.solve(None, 1024, cap)
    assert sb.last_return == capi.MI_OK
    return sb, st, npv


def solve_in_calls(sb, per_call):
    total = np.zeros(sb.n_lps, dtype=np.int64)
    for _ in range(CAP):
        st, npv = sb.solve(None, 1024, per_call)
        assert sb.last_return == capi.MI_OK
        total += npv
        if not (st == capi.MI_MAX_PIVOTS).any():
            return st, total
    raise AssertionError("the batch did not finish")


# ------------------------------------------------------------------ 1: four bands, both senses, interleaved
@modes
def test_mixed_shapes_and_senses_in_one_batch(threads, classes):
    ins, wants = rc.mixed()
    sb, st, npv = _run(ins, threads, classes)
    check_members(sb, st, npv, wants)
    # what the occupancy query gives for a member's bytes: read from a batch of ONE shape, capped at four
    lp.single.set_batch_threads(threads)
    own = {}
    for M0, b0, _ in ins:
        if M0.shape not in own:
            uniform = lp.SingleBatch.from_arrays(M0[None], b0[None])
            own[M0.shape] = min(uniform.info()["members_per_cu"], 4)
            uniform.close()
    assert threads != 256 or len(set(own.values())) == 4, own              # four distinct residencies
    largest = own[max(own, key=lambda s: lp.single.single_lds_bytes(*s))]
    for q, (M0, b0, is_max) in enumerate(ins):
        shape = sb.member_shape(q)
        assert (shape["rows"], shape["cols"]) == M0.shape and shape["is_max"] == int(is_max), q
        assert shape["ld"] == (M0.shape[1] + 31) // 32 * 32, q
        assert shape["occupancy_class"] == (own[M0.shape] if classes == 4 else largest), (q, shape, own)
    assert sb.info()["members_per_cu"] == largest


# ------------------------------------------------------------------ 2: more members than resident workgroups
@modes
def test_more_members_than_resident_workgroups(threads, classes):
    ins, wants = rc.small_cycle()
    sb, st, npv = _run(ins, threads, classes)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ 3: a batch of one
@modes
def test_a_batch_of_one(threads, classes):
    ins, wants = rc.mixed()
    for q in (1, 6):
        sb, st, npv = _run(ins[q:q + 1], threads, classes)
        check_members(sb, st, npv, wants[q:q + 1])


# ------------------------------------------------------------------ 4: one shape: the batch of one shape's results
@modes
def test_members_of_one_shape_equal_the_uniform_batch(threads, classes):
    ins, wants = rc.one_shape()
    sb, st, npv = _run(ins, threads, classes)
    check_members(sb, st, npv, wants)
    uniform = lp.SingleBatch.from_arrays(np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins]))
    ust, unpv = uniform.solve(True, 1024, CAP)
    assert np.array_equal(ust, st) and np.array_equal(unpv, npv)
    for q in range(len(ins)):
        (G, gb), (U, ub) = sb.download(q), uniform.download(q)
        assert same_bits(G, U) and np.array_equal(gb, ub), q
        assert np.array_equal(sb.trace(q), uniform.trace(q)), q
        assert sb.member_shape(q)["occupancy_class"] == min(uniform.info()["members_per_cu"], 4)     # (one shape: one class)


# ------------------------------------------------------------------ 5: continuation
@modes
def test_calls_of_five_pivots_equal_one_call(threads, classes):
    ins, wants = rc.mixed()
    sb = make_ragged(ins, threads, classes)
    st, npv = sb.solve(None, 1024, 5)
    assert st.tolist() == [capi.MI_MAX_PIVOTS] * len(ins) and npv.tolist() == [5] * len(ins)
    st, more = solve_in_calls(sb, 5)
    check_members(sb, st, npv + more, wants)


@modes
def test_launch_cap_of_three_equals_the_default(threads, classes):
    ins, wants = rc.mixed()
    sb, st, npv = _run(ins, threads, classes, launch_cap=3)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ 6: exact ties at the boundaries
@modes
def test_ties_at_the_boundaries_in_one_batch(threads, classes):
    ins, wants = rc.tie_members()
    assert [i[0].shape for i in ins] == [(4, 1104), (301, 7), (6, 13), (4, 1104), (301, 7)]
    sb, st, npv = _run(ins, threads, classes, cap=10)
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ 7: outcomes that differ
@modes
def test_one_members_outcome_does_not_change_anothers(threads, classes):
    ins, wants = rc.outcome_members()
    sb, st, npv = _run(ins, threads, classes, cap=rc.OUTCOME_CAP)
    assert [int(s) for s in st] == [capi.MI_OPTIMAL, capi.MI_UNBOUNDED, capi.MI_MAX_PIVOTS, capi.MI_OPTIMAL,
                                    capi.MI_OPTIMAL, capi.MI_MAX_PIVOTS, capi.MI_OPTIMAL, capi.MI_MAX_PIVOTS]
    check_members(sb, st, npv, wants)


# ------------------------------------------------------------------ 8: two-phase
@pytest.mark.parametrize("per_call", [CAP, 3])
@modes
def test_two_phase_members_of_different_shapes_as_one_pair(threads, classes, per_call):
    members, wants = rc.pairs()
    ab = make_ragged([(A, abasis, None) for A, abasis, _, _, _ in members], threads, classes)
    mb = make_ragged([(M, mbasis, is_max) for _, _, M, mbasis, is_max in members], threads, classes)
    n = len(members)
    total = np.zeros((n, 2), dtype=np.int64)
    for _ in range(CAP):
        st, npv = ab.solve_two_phase(mb, None, 1024, per_call)
        assert ab.last_return == capi.MI_OK and npv.shape == (n, 2)
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


# ------------------------------------------------------------------ 9: declines and errors
def _create(ins, senses=True):
    rows = np.array([i[0].shape[0] for i in ins], dtype=np.int64)
    cols = np.array([i[0].shape[1] for i in ins], dtype=np.int64)
    flat = np.concatenate([np.ascontiguousarray(i[0]).ravel() for i in ins])
    basis = np.concatenate([i[1] for i in ins])
    sense = np.array([int(bool(i[2])) for i in ins], dtype=np.int32)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    rc_ = capi.lib().mi355x_sbatch_create_ragged(ctypes.byref(h), len(ins), p(rows), p(cols), p(sense) if senses else None,
                                                 p(flat), p(basis), 0)
    return rc_, h


def _last_error():
    return capi.lib().mi355x_last_error().decode("utf-8", "replace")


def test_a_member_beyond_the_budget_declines_the_batch_and_names_itself():
    import torch
    ins, _ = rc.one_shape()
    big = sc.synthetic(300, 98, seed=1) + (True,)
    assert lp.single.single_lds_bytes(*big[0].shape) > lp.single.LDS_BUDGET
    rc_, h = _create(ins[:2])                                             # (warm: the first create's own allocations)
    assert rc_ == capi.MI_OK
    capi.lib().mi355x_sbatch_destroy(h)
    rc_, h = _create([ins[0], ins[1], big, ins[2]])
    assert rc_ == capi.MI_UNSUPPORTED and not h.value
    assert "member 2" in _last_error() and "99x399" in _last_error()
    # nothing left behind: 200 declined creates of 64 members (whose trace buffers alone would be 1 MiB per create)
    many = [ins[k % len(ins)] for k in range(63)] + [big]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(200):
        rc_, h = _create(many)
        assert rc_ == capi.MI_UNSUPPORTED and not h.value
    assert "member 63" in _last_error()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20
    with pytest.raises(capi.Mi355xError) as e:
        lp.SingleBatch.from_ragged([i[0] for i in (ins[0], big)], [i[1] for i in (ins[0], big)], [True, True])
    assert e.value.code == capi.MI_UNSUPPORTED
    rc_, h = _create([ins[0], ins[1], ins[2]])                            # without it the create succeeds again
    assert rc_ == capi.MI_OK and h.value
    capi.lib().mi355x_sbatch_destroy(h)


def test_argument_errors_on_a_ragged_handle():
    L = capi.lib()
    ins, _ = rc.one_shape()
    members, _ = rc.pairs()
    sb = make_ragged(ins[:2], 256, 0)
    st, npv = np.empty(2, dtype=np.int32), np.empty(4, dtype=np.int64)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    for sense in (1, 0, 2):
        assert L.mi355x_sbatch_solve(sb._handle, sense, 1024.0, CAP, p(st), p(npv)) == capi.MI_BAD_ARG
    assert "form 4" in _last_error()
    rhs, obj, basis = np.empty(256, dtype=F32), np.empty(256, dtype=F32), np.empty(256, dtype=np.int64)
    assert L.mi355x_sbatch_readback(sb._handle, p(rhs), p(obj), p(basis)) == capi.MI_UNSUPPORTED
    assert "form 4" in _last_error()
    # the batch is untouched by the refused calls
    got = sb.solve(None, 1024, CAP)
    assert got[0].tolist() == [capi.MI_OPTIMAL] * 2
    # pairs that do not match
    arts = [(A, abasis, None) for A, abasis, _, _, _ in members]
    mains = [(M, mbasis, is_max) for _, _, M, mbasis, is_max in members]

    def pair_rc(a_ins, m_ins, sense=-1):
        ab, mb = make_ragged(a_ins, 256, 0), make_ragged(m_ins, 256, 0)
        st2, npv2 = np.empty(len(a_ins), dtype=np.int32), np.empty(2 * len(a_ins), dtype=np.int64)
        return L.mi355x_sbatch_solve_two_phase(ab._handle, mb._handle, sense, 1024.0, CAP, p(st2), p(npv2))
    assert pair_rc(arts[:2], mains[:2]) == capi.MI_OK
    assert pair_rc(arts[:2], mains[:2], sense=1) == capi.MI_BAD_ARG       # the sense is the members' own
    assert pair_rc(arts[:2], mains[:3]) == capi.MI_BAD_ARG                # n_lps
    assert pair_rc(arts[:2], [mains[1], mains[0]]) == capi.MI_BAD_ARG     # rows differ per member
    assert pair_rc(mains[:2], arts[:2]) == capi.MI_BAD_ARG                # art cols < main cols
    uniform = lp.SingleBatch.from_arrays(np.stack([mains[0][0]] * 2), np.stack([mains[0][1]] * 2))
    ab = make_ragged([arts[0]] * 2, 256, 0)
    st2, npv2 = np.empty(2, dtype=np.int32), np.empty(4, dtype=np.int64)
    assert L.mi355x_sbatch_solve_two_phase(ab._handle, uniform._handle, -1, 1024.0, CAP, p(st2), p(npv2)) == capi.MI_BAD_ARG


# ------------------------------------------------------------------ 10: the public route
def _lp_problem(d, integer_vars=()):
    return lp.Problem(type=d["type"], vars=list(d["vars"]), objective_var=d.get("objective_var"),
                      objective_func=list(d["objective"]), var_bounds=[(b[0], (b[1], b[2])) for b in d["bounds"]],
                      constraints=list(d["constraints"]), integer_vars=list(integer_vars))


def _problem_of(M0, n, m, kind="max"):
    """The LP a synthetic tableau [A | I | b ; -c | 0 | 0] is built from (its numbers are float32 values)."""
    names = ["x%d" % j for j in range(n)]
    return lp.Problem(type=kind, vars=names, objective_var="z",
                      objective_func=[(names[j], F32(-M0[m, j])) for j in range(n)],
                      constraints=[("<=", [(names[j], M0[i, j]) for j in range(n)], M0[i, n + m]) for i in range(m)])


def test_public_function_with_mixed_shapes(monkeypatch):
    integer = dict(type="max", vars=["x", "y"], objective_var="z", objective=[("x", 1), ("y", 1)], bounds=[],
                   constraints=[("<=", [("x", 1), ("y", 2)], 4), ("<=", [("x", 3), ("y", 1)], 6)])
    ps = [_problem_of(sc.synthetic(40, 24, seed=1)[0], 40, 24), _lp_problem(sc.DRIVEOUT_LP),
          _problem_of(sc.synthetic(7, 5, seed=2)[0], 7, 5, "min"), _lp_problem(rc.PAIR_3),
          _lp_problem(integer, integer_vars=["x"]), _problem_of(sc.synthetic(300, 98, seed=1)[0], 300, 98),
          _lp_problem(sc.INFEASIBLE_LP), _problem_of(sc.synthetic(9, 6, seed=3)[0], 9, 6), _lp_problem(rc.PAIR_4),
          _problem_of(sc.synthetic(11, 3, seed=4)[0], 11, 3)]
    slots, groups, groups2 = lp.single.group_single_problems(ps)
    assert [len(v) for v in groups.values()] == [1] * 5 and sorted(len(v) for v in groups2.values()) == [1, 1, 2]
    made = []
    for name in ("from_ragged", "from_arrays"):
        def counted(*a, _f=getattr(lp.SingleBatch, name), _name=name, **kw):
            made.append(_name)
            return _f(*a, **kw)
        monkeypatch.setattr(lp.SingleBatch, name, counted)
    got = lp.solve_problems(ps, precision="single", mixed_shapes=True, errorp=False, max_pivots=CAP)
    # one ragged batch (4 single-phase members inside the budget), one ragged pair (main + art), no uniform batch
    assert made == ["from_ragged"] * 3
    plain = lp.solve_problems(ps, precision="single", errorp=False, max_pivots=CAP)
    assert len(got) == len(plain) == len(ps)
    assert isinstance(got[4], lp.UnsupportedConstraintError) and got[4].args[0][0] == "integer"
    assert isinstance(got[6], lp.InfeasibleProblemError)
    for k in range(len(ps)):
        if k in (4, 6):
            assert type(plain[k]) is type(got[k]) and plain[k].args == got[k].args
            with pytest.raises(type(got[k])):
                lp.single.solve_single(ps[k], max_pivots=CAP)
            continue
        alone = lp.single.solve_single(ps[k], max_pivots=CAP)
        for g in (got[k], plain[k]):
            assert isinstance(g, lp.SingleTableau) and g.matrix.dtype == np.float32, k
            assert same_bits(g.matrix, alone.matrix) and np.array_equal(g.basis_columns, alone.basis_columns), k
            assert g.n_pivots == alone.n_pivots, k
            assert lp.solution_objective_value(g).tobytes() == lp.solution_objective_value(alone).tobytes(), k
            for v in ps[k].vars:
                x = lp.solution_variable(g, v)
                assert isinstance(x, np.float32) and x.tobytes() == lp.solution_variable(alone, v).tobytes(), (k, v)
                assert lp.solution_reduced_cost(g, v).tobytes() == lp.solution_reduced_cost(alone, v).tobytes(), (k, v)
    with pytest.raises(lp.UnsupportedConstraintError):
        lp.solve_problems(ps, precision="single", mixed_shapes=True, max_pivots=CAP)
