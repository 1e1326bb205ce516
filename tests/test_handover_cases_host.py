"""tests/handover_cases.py checked on the oracle alone (no GPU).

  * replay_handover IS the oracle's hand-over: prepare() + replay_handover + oracle.solve give orc_solve_two_phase's
    bits on every case, so tests/test_gpu_handover.py may compare against the replay where it stops before phase 2.
  * Every case has what it claims: scales that the original-coefficient shortcut gets wrong, objective entries
    that differ with them, the drive-out pivots, the edge ingredients.  These are conditions on the INPUTS (the
    seeds and hand-set entries in handover_cases.py were picked so that they hold): they show that a kernel which
    took the shortcut would fail the GPU comparison on that case."""
import numpy as np
import pytest

import oracle
from tests import handover_cases as hc

REACHES = [n for n in hc.CASES if hc.handed_over(hc.CASES[n])[1] is not None]


@pytest.mark.parametrize("name", list(hc.CASES))
def test_replay_is_the_oracles_handover(name):
    case = hc.CASES[name]
    want = hc.expected(case)
    p, M = hc.handed_over(case)
    if M is None:
        assert want.status == p.status != oracle.OPTIMAL and want.npv == (p.n_phase1, 0)
        assert hc.same_bits(want.art, p.art) and np.array_equal(want.art_basis, p.art_basis)
        assert hc.same_bits(want.main, case.main)                            # untouched
        return
    M, mb = M.copy(), p.art_basis.copy()
    with np.errstate(all="ignore"):
        st, n2, _ = oracle.solve(M, mb, is_max=True, factor=hc.F)
    assert (st, (p.n_phase1, n2)) == (want.status, want.npv)
    assert hc.same_bits(want.art, p.art) and np.array_equal(want.art_basis, p.art_basis)
    assert hc.same_bits(want.main, M) and np.array_equal(want.main_basis, mb)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_bases_are_in_range_and_distinct(name):
    case = hc.CASES[name]
    b, nav = case.art_basis, case.art.shape[1] - 1
    assert b.min() >= 0 and b.max() < nav and len(set(b.tolist())) == len(b)
    p, _ = hc.handed_over(case)
    assert p.art_basis.min() >= 0 and p.art_basis.max() < nav and len(set(p.art_basis.tolist())) == len(b)


@pytest.mark.parametrize("name", REACHES)
def test_the_shortcut_would_be_seen(name):
    case = hc.CASES[name]
    c = hc.census(case)
    m = hc.SHAPE[name][0]
    p, M = hc.handed_over(case)
    if "unit" in case.ingredients:                       # the one unit-basis member of a batch: nothing to see
        assert c == (0, 0, 0, 0)
        return
    if "lived" in case.ingredients:
        assert c.scales >= 3 and p.n_phase1 - c.driveouts >= 1, c
    elif c.driveouts == 0:
        assert c.scales >= 2, c
        if m >= 40:
            assert c.scales >= m / 2, c
    if np.all(np.isfinite(M)):
        assert c.objective >= 1, c
    else:
        Ms, _ = hc.replay_handover(p.art, p.art_basis, case.main, shortcut=True)
        assert not np.array_equal(np.isnan(M[-1]), np.isnan(Ms[-1]))


@pytest.mark.parametrize("name", hc.UNBOUNDED_AT_ONCE)
def test_unbounded_at_once_leaves_the_pure_handover_output(name):
    case = hc.CASES[name]
    want = hc.expected(case)
    assert want.status == oracle.UNBOUNDED and want.npv == (0, 0)
    assert hc.same_bits(want.main, hc.handed_over(case)[1])


def _scales(name):
    case = hc.CASES[name]
    p, _ = hc.handed_over(case)
    _, s = hc.replay_handover(p.art, p.art_basis, case.main)
    return case, p, s, case.main[-1][p.art_basis]


@pytest.mark.parametrize("name", [n for n in hc.CASES if "a" in hc.CASES[n].ingredients])
def test_ingredients_a_b_c(name):
    case, p, s, c0 = _scales(name)
    assert np.any((c0 != 0.0) & (s == 0.0))                                  # (a) non-zero coefficient, zero scale
    assert np.any((c0 == 0.0) & ~np.signbit(c0) & (s != 0.0))                # (b) +0.0 coefficient, non-zero scale
    assert np.any((c0 == 0.0) & np.signbit(c0))                              # (c) a -0.0 coefficient
    B = p.art[:-1][:, p.art_basis]
    above = np.triu(B, 1) != 0.0
    assert np.any(above & (s != 0.0)[:, None])                               # above the diagonal, in a row that is not skipped
    assert np.array_equal(np.diag(B), np.ones(len(s))) and not np.array_equal(B, np.eye(len(s)))


@pytest.mark.parametrize("name", [n for n in hc.CASES if "d" in hc.CASES[n].ingredients])
def test_ingredient_d(name):
    case, p, s, c0 = _scales(name)
    assert np.sum(np.isinf(c0)) == 1 and np.all(np.isfinite(np.delete(case.main[-1], p.art_basis[np.isinf(c0)])))
    assert np.any(np.isnan(s)) and not np.array_equal(p.art[:-1][:, p.art_basis], np.eye(len(s)))
    want = hc.expected(case)
    assert want.status == oracle.OPTIMAL and want.npv == (0, 0) and np.isnan(want.main[-1, 0])


def test_ingredients_e_and_f():
    case = hc.CASES["5x9-driveout"]
    p, _ = hc.handed_over(case)
    nv = hc.SHAPE[case.name][1]
    rows = np.flatnonzero(case.art_basis >= nv)
    assert len(rows) == 2 and np.all(case.art[rows, -1] == 0.0) and np.all(p.art_basis < nv)
    assert p.status == oracle.OPTIMAL and len(p.driveout_elements) == 2
    assert p.driveout_elements[0] > 0.0 > p.driveout_elements[1]
    for r in rows:                                                           # a basic column with a non-zero entry comes first
        first = np.flatnonzero(case.art[r, :nv])[0]
        assert first in case.art_basis
    stuck = hc.CASES["5x9-stuck"]
    (r,) = np.flatnonzero(stuck.art_basis >= nv)
    nz = np.flatnonzero(stuck.art[r, :nv])
    assert len(nz) >= 1 and all(j in stuck.art_basis for j in nz) and stuck.art[r, -1] == 0.0
    assert hc.expected(stuck).status == oracle.ART_STUCK and hc.handed_over(stuck)[0].status == oracle.ART_STUCK
    assert not np.array_equal(stuck.art[:-1][:, stuck.art_basis], np.eye(5))


def test_ingredient_g():
    case, twin = hc.CASES["5x9-nonzero"], hc.CASES["5x9-driveout"]
    nv = hc.SHAPE[case.name][1]
    differs = np.argwhere(case.art != twin.art).tolist()
    assert differs == [[3, case.art.shape[1] - 1]] and np.array_equal(case.art_basis, twin.art_basis)
    value = case.art[3, -1]
    assert 0.0 < value <= hc.F * oracle.EPSILON                              # an fp= test would let it pass: /= 0 does not
    p, M = hc.handed_over(case)
    assert M is None and p.status == oracle.ART_NONZERO
    assert p.n_phase1 == 1 and len(p.driveout_elements) == 1                 # row 1 was driven out before row 3 stopped the step
    assert p.art_basis[1] < nv <= p.art_basis[3] and p.art[3, -1] == value
    want = hc.expected(case)
    assert want.status == oracle.ART_NONZERO and want.npv == (1, 0)
    # as a batch member it stands between members that go on
    assert [hc.handed_over(hc.CASES[n])[0].status for n in hc.BATCHES["5x9-nonzero"]] == \
        [oracle.OPTIMAL, oracle.ART_NONZERO, oracle.OPTIMAL]


@pytest.mark.parametrize("name", hc.BOUNDARY + ["5x9-beyond"])
def test_feasibility_boundary(name):
    case = hc.CASES[name]
    edge = hc.F * oracle.EPSILON
    value = abs(case.art[-1, -1])
    want = hc.expected(case)
    if "beyond" in case.ingredients:
        assert value == np.nextafter(edge, np.inf) and want.status == oracle.INFEASIBLE and want.npv == (0, 0)
    else:
        assert value == edge and want.status in (oracle.OPTIMAL, oracle.UNBOUNDED)
    assert hc.handed_over(case)[0].status == (oracle.INFEASIBLE if "beyond" in case.ingredients else oracle.OPTIMAL)
    assert {np.sign(hc.CASES[n].art[-1, -1]) for n in hc.BOUNDARY} == {-1.0, 1.0}
