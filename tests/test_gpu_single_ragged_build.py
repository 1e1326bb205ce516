"""Ragged single-float batches BUILT ON THE DEVICE (k_slp_assemble / k_sbb_assemble / k_sb_readback over an SrView behind
mi355x_sbatch_create_lps_ragged, _create_nodes_ragged and _readback_ragged) against the float32 model of
tests/single_cases.py, single_lps_cases.assemble_rows and single_bb_cases.build_node, member by member and bit for bit:
what a member starts from (every stored entry, padding included, both bases) and what it ends with (status, pivot
counts, traces, bases, every entry).  No tolerance appears anywhere; the GPU is never compared with itself.

On the parent commit every test here fails: the symbols and the keywords do not exist."""
import ctypes

import numpy as np
import pytest

from tests import single_bb_cases as B
from tests import single_cases as sc
from tests import single_lps_cases as C
from tests import single_ragged_build_cases as R
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
F32 = np.float32
same_bits = sc.same_bits
CAP = R.CAP
MODES = [(256, 0), (1024, 0), (256, 4), (1024, 4)]          # (workgroup threads, classes hook)
modes = pytest.mark.parametrize("threads,classes", MODES)


@pytest.fixture(autouse=True)
def _hooks_back_to_auto():
    yield
    lp.single.set_batch_threads(0)
    lp.single.set_batch_ragged_classes(0)


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _last_error():
    return capi.lib().mi355x_last_error().decode("utf-8", "replace")


def lows_of(ds):
    lows = [lp.single_lps.lower_problem_rows_single(C.to_problem(lp, d)) for d in ds]
    assert all(low is not None and not low.float_zero for low in lows)
    return lows


def create(ds, threads=0, classes=0):
    lp.single.set_batch_threads(threads)
    lp.single.set_batch_ragged_classes(classes)
    lows = lows_of(ds)
    main, art = lp.SingleBatch.from_lps_ragged([low.L for low in lows], [low.sense for low in lows],
                                               [d["type"] == "max" for d in ds], [low.col_int_sum for low in lows])
    for sb in (main, art):
        if sb is not None:
            info = sb.info()
            assert info["form"] == 4 and info["n_lps"] == len(ds) and sb.ragged
            assert threads == 0 or info["workgroup_threads"] == threads
    return main, art, lows


def stored(sb, q):
    """Member q as stored: rows x ld, the padding columns included."""
    shape = sb.member_shape(q)
    ld = ctypes.c_int64(0)
    L = capi.lib()
    assert L.mi355x_sbatch_debug_stored(sb._handle, q, None, ctypes.byref(ld)) == capi.MI_OK
    assert ld.value == shape["ld"] == (shape["cols"] + 31) // 32 * 32
    out = np.full((shape["rows"], ld.value), np.nan, dtype=F32)
    assert L.mi355x_sbatch_debug_stored(sb._handle, q, _p(out), None) == capi.MI_OK
    return out


def check_member(sb, q, M, basis):
    G, gb = sb.download(q)
    assert same_bits(G, M) and np.array_equal(gb, basis), q
    S = stored(sb, q)
    assert same_bits(S[:, :M.shape[1]], M), q
    assert not S[:, M.shape[1]:].view(np.uint32).any(), q                 # padding: +0.0 over the whole ld


def check_assembly(ds):
    main, art, lows = create(ds)
    try:
        for q, (d, low) in enumerate(zip(ds, lows)):
            M, mb, A, ab = C.assemble_rows(low.L, low.sense, low.col_int_sum)
            want = sc.build(d)                                            # the second witness: the model's own build
            assert same_bits(M, want["main"][0]) and (A is None) == (want["art"] is None) == (art is None), q
            assert main.member_shape(q)["is_max"] == int(d["type"] == "max"), q
            check_member(main, q, M, mb)
            if art is not None:
                assert same_bits(A, want["art"][0])
                check_member(art, q, A, ab)
    finally:
        main.close()
        if art is not None:
            art.close()


# ------------------------------------------------------------------ 1. assembly from rows
@pytest.mark.parametrize("name", ["sweep_single", "sweep_two_phase", "ld_steps_main", "ld_steps_art", "tall_members",
                                  "outcome_pair", "outcome_single"])
def test_assembly_from_rows(name):
    check_assembly(getattr(R, name)())


def test_assembly_keeps_plus_zero_in_a_negated_row_and_extreme_rows():
    ds = [R.negated_zero_member()] + list(C.zero_rhs_group())
    # (the negated row ends `>=`: a two-phase member, as the members beside it) -- inf, sums near FLT_MAX, subnormals
    check_assembly(ds + list(C.extreme_rows_group()))
    M = sc.build(ds[0])["main"][0]
    assert (M[0, [1, 2]] == 0).all() and not np.signbit(M[0, [1, 2]]).any() and M[0, -1] == 3


# ------------------------------------------------------------------ 2. assembly from nodes
def node_batches(base, entries, threads=0, classes=0):
    lp.single.set_batch_threads(threads)
    lp.single.set_batch_ragged_classes(classes)
    g = lp.single_bb.GeneralFormSingle(B.to_problem(lp, base))
    nb = lp.single_bb.Base(g)
    try:
        return nb.create_nodes_ragged(entries)
    finally:
        nb.close()


@pytest.mark.parametrize("art_base,want_art", [(False, False), (False, True), (True, False)])
def test_assembly_from_nodes_of_depths_1_2_3_5(art_base, want_art):
    base, entries = R.node_base(art_base), R.node_entries(want_art)
    assert R.free_variable_rows(entries)
    main, art = node_batches(base, entries)
    assert (art is not None) == (art_base or want_art)
    for q, e in enumerate(entries):
        M, mb, A, ab = B.build_node(base, e)
        check_member(main, q, M, mb)
        assert main.member_shape(q)["is_max"] == int(base["type"] == "max")
        if art is not None:
            check_member(art, q, A, ab)


# ------------------------------------------------------------------ 3. solves
def solve_calls(main, art, per_call):
    total = None
    for _ in range(10 * CAP):
        st, npv = art.solve_two_phase(main, None, 1024, per_call) if art is not None else main.solve(None, 1024, per_call)
        total = npv.copy() if total is None else total + npv
        if not (st == capi.MI_MAX_PIVOTS).any():
            return st, total
    raise AssertionError("the batch did not finish")


def check_solved(name, main, art, st, npv, cap=CAP):
    for q in range(main.n_lps):
        w = R.solution(name, q, cap)
        assert int(st[q]) == w["status"], (q, int(st[q]), w["status"])
        assert np.atleast_1d(npv[q]).tolist() == list(w["n"]), (q, npv[q], w["n"])
        assert _pairs(main.trace(q).tolist()) == _pairs(w["main_trace"]), q
        M, mb = main.download(q)
        assert same_bits(M, w["M"]) and np.array_equal(mb, w["mbasis"]), q
        if art is not None:
            assert _pairs(art.trace(q).tolist()) == _pairs(w["art_trace"]), q
            A, ab = art.download(q)
            assert same_bits(A, w["A"]) and np.array_equal(ab, w["abasis"]), q


@modes
@pytest.mark.parametrize("name", R.SOLVED_LISTS)
def test_solves_equal_the_model(name, threads, classes):
    main, art, _ = create(getattr(R, name)(), threads, classes)
    st, npv = art.solve_two_phase(main, None, 1024, CAP) if art is not None else main.solve(None, 1024, CAP)
    check_solved(name, main, art, st, npv)


@pytest.mark.parametrize("name", R.SOLVED_LISTS)
def test_solves_in_calls_of_three_pivots(name):
    main, art, _ = create(getattr(R, name)(), 256, 0)
    st, npv = solve_calls(main, art, 3)
    check_solved(name, main, art, st, npv)


def test_capped_members_beside_finished_ones():
    main, art, _ = create(R.outcome_single(), 256, 0)
    st, npv = main.solve(None, 1024, 3)
    assert sorted(set(st.tolist())) == [sc.OPTIMAL, sc.UNBOUNDED, sc.MAX_PIVOTS]
    check_solved("outcome_single", main, None, st, npv, cap=3)


@pytest.mark.parametrize("threads,classes,per_call", [m + (0,) for m in MODES] + [(256, 0, 3), (1024, 4, 3)])
@pytest.mark.parametrize("art_base,want_art", [(False, False), (False, True), (True, False)])
def test_node_solves_equal_the_model(art_base, want_art, threads, classes, per_call):
    base, entries = R.node_base(art_base), R.node_entries(want_art)
    main, art = node_batches(base, entries, threads, classes)
    is_max = base["type"] == "max"
    if per_call:
        st, npv = solve_calls(main, art, per_call)
    else:
        st, npv = art.solve_two_phase(main, None, 1024, CAP) if art is not None else main.solve(None, 1024, CAP)
    rhs, obj, basis = lp.single_bb.readback(main)
    for q, e in enumerate(entries):
        M0, mb0, A0, ab0 = B.build_node(base, e)
        if A0 is None:
            wst, tr, M, mb = sc.solve(M0, mb0, is_max, 1024, CAP)
            assert int(npv[q]) == len(tr), q
        else:
            r = sc.two_phase(A0, ab0, M0, mb0, is_max)
            wst, tr, M, mb = r["status"], r["main_trace"], r["M"], r["mbasis"]
            assert _pairs(art.trace(q).tolist()) == _pairs(r["art_trace"]), q
            assert npv[q].tolist() == [len(r["art_trace"]), r["n2"]], q
        assert int(st[q]) == wst, (q, int(st[q]), wst)
        assert _pairs(main.trace(q).tolist()) == _pairs(tr), q
        G, gb = main.download(q)
        assert same_bits(G, M) and np.array_equal(gb, mb), q
        # the light read-back: last column, last row, basis of the member
        assert same_bits(rhs[q], G[:, -1]) and same_bits(obj[q], G[-1]) and np.array_equal(basis[q], gb), q


# ------------------------------------------------------------------ 4. readback_ragged
def test_readback_ragged_equals_the_download_and_declines_a_uniform_batch():
    main, art, _ = create(R.outcome_pair(), 256, 0)
    art.solve_two_phase(main, None, 1024, CAP)
    for sb in (main, art):
        rhs, obj, basis = lp.single_bb.readback(sb)
        for q in range(sb.n_lps):
            G, gb = sb.download(q)
            assert same_bits(rhs[q], G[:, -1]) and same_bits(obj[q], G[-1]) and np.array_equal(basis[q], gb), q
    M0, b0 = sc.synthetic(7, 5, seed=1)
    uniform = lp.SingleBatch.from_arrays(M0[None], b0[None])
    r, o, b = np.empty(64, dtype=F32), np.empty(64, dtype=F32), np.empty(64, dtype=np.int64)
    assert capi.lib().mi355x_sbatch_readback_ragged(uniform._handle, _p(r), _p(o), _p(b)) == capi.MI_UNSUPPORTED
    assert "mi355x_sbatch_readback" in _last_error()
    assert capi.lib().mi355x_sbatch_readback(main._handle, _p(r), _p(o), _p(b)) == capi.MI_UNSUPPORTED


# ------------------------------------------------------------------ 5. declines and errors
def _raw(m, ncv, sense, rhs=1.0):
    L = np.ones((m + 1, ncv + 1), dtype=F32)
    L[:m, -1] = rhs
    return L, np.full(m, sense, dtype=np.int32)


def _create_raw(members, sums=None):
    m = np.array([L.shape[0] - 1 for L, _ in members], dtype=np.int64)
    ncv = np.array([L.shape[1] - 1 for L, _ in members], dtype=np.int64)
    flat, sense = np.concatenate([L.ravel() for L, _ in members]), np.concatenate([s for _, s in members])
    is_max = np.ones(len(members), dtype=np.int32)
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    rc = capi.lib().mi355x_sbatch_create_lps_ragged(ctypes.byref(hm), ctypes.byref(ha), len(members), _p(m), _p(ncv), _p(is_max),
                                                    _p(flat), _p(sense), _p(sums) if sums is not None else None, 0)
    return rc, hm, ha


def _destroy(*hs):
    for h in hs:
        if h.value:
            capi.lib().mi355x_sbatch_destroy(h)


def test_declines_name_the_member_and_leave_nothing_behind():
    import torch
    small = [_raw(3, 2, 0), _raw(5, 4, 0)]
    rc, hm, ha = _create_raw(small)                                       # (warm: the first create's own allocations)
    assert rc == capi.MI_OK and hm.value and not ha.value
    _destroy(hm)
    # single-phase: 99 x 399 is beyond the budget
    rc, hm, ha = _create_raw(small + [_raw(98, 300, 0)])
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value and "member 2" in _last_error() and "99x399" in _last_error()
    # two-phase: the ARTIFICIAL shape decides -- 84 rows `>=` over 300 columns: main 85 x 385 fits, art 85 x 469 does not
    assert C.fits(85, 385) and not C.fits(85, 469)
    rc, hm, ha = _create_raw([_raw(3, 2, 1), _raw(84, 300, 1)])
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value and "member 1" in _last_error() and "85x469" in _last_error()
    # the guard
    sums = np.zeros(3 + 5, dtype=np.float64)
    sums[4] = 2.0 ** 24 + 2
    rc, hm, ha = _create_raw(small, sums)
    assert rc == capi.MI_UNSUPPORTED and "member 1" in _last_error() and "2^24" in _last_error()
    # the mixture of single- and two-phase members
    rc, hm, ha = _create_raw(small + [_raw(3, 2, 1)])
    assert rc == capi.MI_BAD_ARG and "member 2" in _last_error()
    # nothing left behind
    many = [small[k % 2] for k in range(63)] + [_raw(98, 300, 0)]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(200):
        rc, hm, ha = _create_raw(many)
        assert rc == capi.MI_UNSUPPORTED and not hm.value
    assert "member 63" in _last_error()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20
    rc, hm, ha = _create_raw(small)
    assert rc == capi.MI_OK
    _destroy(hm)


def _node_create(handle, g, entries):
    """mi355x_sbatch_create_nodes_ragged itself; entries: tuples of (var name or index, sense, bound)."""
    flat = [r for e in entries for r in e]
    depth = np.array([len(e) for e in entries], dtype=np.int64)
    var = np.array([g.index[v] if isinstance(v, str) else v for v, _, _ in flat], dtype=np.int64)
    sense = np.array([x for _, x, _ in flat], dtype=np.int32)
    bound = np.array([b for _, _, b in flat], dtype=np.int64)
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    rc = capi.lib().mi355x_sbatch_create_nodes_ragged(ctypes.byref(hm), ctypes.byref(ha), handle, len(entries), _p(depth),
                                                      _p(var), _p(sense), _p(bound))
    return rc, hm, ha


def _base(d):
    g = lp.single_bb.GeneralFormSingle(B.to_problem(lp, d))
    return g, lp.single_bb.Base(g)


def test_node_declines_name_the_node_and_leave_nothing_behind():
    import torch
    L = capi.lib()
    g, nb = _base(R.node_base(False))
    single, two = R.node_entries(False), R.node_entries(True)
    # a form-4 handle carries the sense per member: the base has to have been told
    rc, hm, ha = _node_create(nb.handle, g, single[:2])
    assert rc == capi.MI_BAD_ARG and not hm.value and not ha.value and "mi355x_sbb_base_set_sense" in _last_error()
    for bad in (2, -1):
        assert L.mi355x_sbb_base_set_sense(nb.handle, bad) == capi.MI_BAD_ARG
    assert L.mi355x_sbb_base_set_sense(nb.handle, 1) == capi.MI_OK
    rc, hm, ha = _node_create(nb.handle, g, single[:2])                   # (warm: the first create's own allocations)
    assert rc == capi.MI_OK and hm.value and not ha.value
    _destroy(hm)
    # the mixture of single- and two-phase nodes, either way round
    rc, hm, ha = _node_create(nb.handle, g, [single[0], single[1], two[0]])
    assert rc == capi.MI_BAD_ARG and not hm.value and "node 2 has" in _last_error() and "have none" in _last_error()
    rc, hm, ha = _node_create(nb.handle, g, [two[0], single[0]])
    assert rc == capi.MI_BAD_ARG and "node 1 has 0" in _last_error() and "have some" in _last_error()
    # bad node rows: the variable, the sense, the bound, a depth (the row's index in the concatenated arrays is named)
    n_vars = len(g.kind)
    for row in ((n_vars, 0, 1), (-1, 0, 1), (0, 2, 1), (0, -1, 1), (0, 0, -2 ** 63)):
        rc, hm, ha = _node_create(nb.handle, g, [single[0], (row,)])
        assert rc == capi.MI_BAD_ARG and not hm.value and "bad node row 1" in _last_error(), row
    hm, ha = ctypes.c_void_p(), ctypes.c_void_p()
    zero = np.zeros(1, dtype=np.int64)
    assert L.mi355x_sbatch_create_nodes_ragged(ctypes.byref(hm), ctypes.byref(ha), nb.handle, 1, _p(zero), _p(zero),
                                               _p(zero.astype(np.int32)), _p(zero)) == capi.MI_BAD_ARG
    assert "node 0: depth=0" in _last_error()
    # the assembly's LDS (m + 3 d words in 48 KiB): a node of 4100 rows beside a small one
    deep = tuple(("v0", 0, 3 + k) for k in range(4100))
    rc, hm, ha = _node_create(nb.handle, g, [single[0], deep])
    assert rc == capi.MI_UNSUPPORTED and not hm.value and "node 1" in _last_error() and "assembly's LDS" in _last_error()
    nb.close()
    # the guard: single_bb_cases.guard_case's columns sum past 2^24 with any node row
    g, nb = _base(B.guard_case())
    assert L.mi355x_sbb_base_set_sense(nb.handle, 1) == capi.MI_OK
    assert not g.device_ok((("x", 0, 1),))
    rc, hm, ha = _node_create(nb.handle, g, [(("x", 0, 1),), (("y", 0, 2), ("x", 0, 1))])
    assert rc == capi.MI_UNSUPPORTED and not hm.value and "node 0" in _last_error() and "2^24" in _last_error()
    nb.close()
    # the budget, by the ARTIFICIAL shape: 191 redundant rows under kind_case("both") make a depth-2 node 197 x 199
    # (inside the budget) whose two `>=` rows make its artificial tableau 197 x 201 (beyond it)
    d0 = B.kind_case("both")
    big = dict(d0, constraints=list(d0["constraints"]) + [("<=", [("x", 1), ("y", 1)], 100 + i) for i in range(191)])
    over = (("x", 1, 1), ("y", 1, 1))
    M, _, A, _ = B.build_node(big, over)
    assert M.shape == (197, 199) and A.shape == (197, 201) and C.fits(*M.shape) and not C.fits(*A.shape)
    g, nb = _base(big)
    assert L.mi355x_sbb_base_set_sense(nb.handle, 1) == capi.MI_OK
    small = (("x", 1, 1),)
    rc, hm, ha = _node_create(nb.handle, g, [small, small])
    assert rc == capi.MI_OK and hm.value and ha.value
    _destroy(hm, ha)
    rc, hm, ha = _node_create(nb.handle, g, [small, over])
    assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value
    assert "node 1" in _last_error() and "197x201" in _last_error()
    # nothing left behind: 200 declined creates of 64 nodes
    many = [small] * 63 + [over]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(200):
        rc, hm, ha = _node_create(nb.handle, g, many)
        assert rc == capi.MI_UNSUPPORTED and not hm.value and not ha.value
    assert "node 63" in _last_error()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20
    rc, hm, ha = _node_create(nb.handle, g, [small, small])
    assert rc == capi.MI_OK
    _destroy(hm, ha)
    nb.close()


# ------------------------------------------------------------------ 6. routes
def test_from_rows_route_with_mixed_shapes(monkeypatch):
    ds = R.sweep_single()[:5] + R.sweep_two_phase()[:4] + [C.float_zero_member(), C._synthetic_problem(300, 98, 1, False),
                                                            C.declined_member(), dict(R.sweep_single()[6])]
    ps = [C.to_problem(lp, d) for d in ds]
    ps.insert(3, C.to_problem(lp, C.lone_member(), integer_vars=["x0"]))
    made = []
    for name in ("from_lps_ragged", "from_lps"):
        def counted(*a, _f=getattr(lp.SingleBatch, name), _name=name, **kw):
            made.append(_name)
            return _f(*a, **kw)
        monkeypatch.setattr(lp.SingleBatch, name, counted)
    got = lp.single_lps.solve_problems_single_from_rows(ps, mixed_shapes=True, errorp=False, max_pivots=CAP)
    assert made == ["from_lps_ragged"] * 2                                # one ragged batch and one ragged pair
    first_error = None
    for k, p in enumerate(ps):
        try:
            alone = lp.single.solve_single(p, max_pivots=CAP)
        except lp.SolverError as e:
            first_error = first_error or e
            assert type(got[k]) is type(e) and got[k].args == e.args, k
            continue
        g = got[k]
        assert isinstance(g, lp.SingleTableau), (k, g)
        assert same_bits(g.matrix, alone.matrix) and np.array_equal(g.basis_columns, alone.basis_columns), k
        assert g.n_pivots == alone.n_pivots, k
    assert first_error is not None
    with pytest.raises(type(first_error)):
        lp.single_lps.solve_problems_single_from_rows(ps, mixed_shapes=True, errorp=True, max_pivots=CAP)


SEARCHES = [("case", name) for name in B.search_cases()] + [("seed",) + c for c in R.SEARCH_MIXED_TWO]


@pytest.mark.parametrize("case", SEARCHES, ids=lambda c: "-".join(str(x) for x in c))
def test_search_with_mixed_shapes_equals_the_model(case, monkeypatch):
    d, want = B.case(case[1]) if case[0] == "case" else R.search_problem(*case[1:])
    creates = []
    f = lp.single_bb.Base.create_nodes_ragged
    monkeypatch.setattr(lp.single_bb.Base, "create_nodes_ragged", lambda self, es: creates.append(len(es)) or f(self, es))
    for width in (1, 2, 4, 8):
        s = lp.single_bb.SingleBranchAndBound(B.to_problem(lp, d), width=width, max_pivots=B.PIVOT_CAP, mixed_shapes=True)
        del creates[:]
        per_round = []

        def spy(entries, _call=s.rounds.__call__):
            n0 = len(creates)
            out = _call(entries)
            per_round.append(len(creates) - n0)
            return out
        s.rounds = _Rounds(s.rounds, spy)
        if want.status == sc.OPTIMAL:
            t = s.run()
            assert same_bits(t.matrix, want.M) and np.array_equal(t.basis_columns, want.basis), width
        else:
            with pytest.raises(lp.SolverError):
                s.run()
        assert B.same_trace(s.trace(), want.trace), width
        assert max(per_round) <= 2 and all(n >= 2 for n in creates), (width, per_round, creates)
        assert s.stats()["ragged_batched"] == sum(creates) and (width > 1 or not creates), width
        if case[0] == "seed" and width == 4:
            # the host test has these rounds hold two-phase nodes of two depths: they went as ONE pair
            sets = R.round_depth_sets(case[1], case[2], 4)
            assert sorted(creates) == sorted(n for one, two in sets for n in (len(one), len(two)) if n >= 2), creates


class _Rounds:
    """A DeviceRounds whose call goes through a spy; everything else is the original's."""

    def __init__(self, rounds, call):
        self.__dict__["_r"], self.__dict__["_call"] = rounds, call

    def __call__(self, entries):
        return self._call(entries)

    def __getattr__(self, name):
        return getattr(self._r, name)


def test_a_declined_ragged_create_leaves_the_nodes_to_their_groups(monkeypatch):
    d, want = B.case("le_1")

    def declined(self, entries):
        raise capi.Mi355xError(capi.MI_UNSUPPORTED, "mi355x_sbatch_create_nodes_ragged")
    monkeypatch.setattr(lp.single_bb.Base, "create_nodes_ragged", declined)
    s = lp.single_bb.SingleBranchAndBound(B.to_problem(lp, d), width=4, max_pivots=B.PIVOT_CAP, mixed_shapes=True)
    t = s.run()
    assert same_bits(t.matrix, want.M) and B.same_trace(s.trace(), want.trace) and s.stats()["ragged_batched"] == 0


def test_public_call_with_mixed_shapes():
    d, want = B.case("le_1")
    t = lp.mi355x_simplex_solver(B.to_problem(lp, d), precision="single", branch_and_bound=True, bb_width=4,
                                 mixed_shapes=True, max_pivots=B.PIVOT_CAP)
    assert same_bits(t.matrix, want.M) and np.array_equal(t.basis_columns, want.basis)
