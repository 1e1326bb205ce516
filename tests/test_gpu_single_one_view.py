"""Single-float batches: what the forms share.  A batch of one shape (form 2, LDS; form 3, global) is a ragged batch
(form 4) whose descriptors can be computed, so the same members must read the same through either: the light
read-back (mi355x_sbatch_readback against the per-member slices of mi355x_sbatch_readback_ragged, bases included),
and mi355x_sbatch_download, mi355x_sbatch_debug_stored and mi355x_sbatch_member_shape on the first and the last
member of every form.  Bit for bit; what a member ends with is also checked against the float32 model of
tests/single_cases.py, so the GPU is never only compared with itself."""
import ctypes

import numpy as np
import pytest

from tests import single_cases as sc
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
capi = lp.capi
F32 = np.float32
same_bits = sc.same_bits

#: 3 x 5 (two constraints, two variables; ld 32: 27 padding columns), three different members
SMALL = [sc.synthetic(2, 2, seed=s) for s in (11, 12, 13)]
#: 1 x 2: an objective row alone, no basis entry
BARE = (np.array([[1.0, 0.0]], dtype=F32), np.zeros(0, dtype=np.int64))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _uniform(members, form="lds"):
    sb = lp.SingleBatch.from_arrays(np.stack([M for M, _ in members]), np.stack([b for _, b in members]), form=form)
    sb.solve(True)
    return sb


def _ragged(members):
    sb = lp.SingleBatch.from_ragged([M for M, _ in members], [b for _, b in members], [True] * len(members))
    sb.solve(None)
    return sb


def _same_readback(got, want, q):
    for g, w in zip(got[:2], want[:2]):
        assert same_bits(np.asarray(g), np.asarray(w)), q
    assert np.array_equal(got[2], want[2]), q


def test_readback_of_one_shape_equals_the_ragged_slices():
    """Three 3 x 5 members as a form-2 batch and as a form-4 batch."""
    u, r = _uniform(SMALL), _ragged(SMALL)
    assert u.info()["form"] == 2 and r.info()["form"] == 4
    urhs, uobj, ubasis = lp.single_bb.readback(u)
    rrhs, robj, rbasis = lp.single_bb.readback(r)
    for q, (M0, b0) in enumerate(SMALL):
        _same_readback((rrhs[q], robj[q], rbasis[q]), (urhs[q], uobj[q], ubasis[q]), q)
        st, _, M, basis = sc.solve(M0, b0, True)
        assert st == sc.OPTIMAL
        _same_readback((urhs[q], uobj[q], ubasis[q]), (M[:, -1], M[-1], basis), q)


def test_readback_behind_a_member_without_basis_entries():
    """A 1 x 2 member first (rows - 1 = 0 basis entries), a 3 x 5 member behind it."""
    members = [BARE, SMALL[0]]
    r = _ragged(members)
    rrhs, robj, rbasis = lp.single_bb.readback(r)
    for q, member in enumerate(members):
        u = _uniform([member])
        urhs, uobj, ubasis = lp.single_bb.readback(u)
        assert ubasis.shape == (1, member[0].shape[0] - 1)
        _same_readback((rrhs[q], robj[q], rbasis[q]), (urhs[0], uobj[0], ubasis[0]), q)
    st, _, M, basis = sc.solve(*SMALL[0], True)
    _same_readback((rrhs[1], robj[1], rbasis[1]), (M[:, -1], M[-1], basis), 1)
    assert same_bits(rrhs[0], BARE[0][:, -1]) and same_bits(robj[0], BARE[0][-1]) and rbasis[0].size == 0


#: form 4 with a smaller member between the two 3 x 5 ones, so that member n - 1 does not sit at a multiple of a stride
MIXED = [SMALL[0], sc.synthetic(2, 1, seed=14), SMALL[2]]


@pytest.mark.parametrize("form", [2, 3, 4])
def test_download_stored_layout_and_member_shape_agree(form):
    members = MIXED if form == 4 else SMALL
    sb = _ragged(members) if form == 4 else _uniform(members, "global" if form == 3 else "lds")
    assert sb.info()["form"] == form
    L = capi.lib()
    for q in (0, len(members) - 1):
        M0, b0 = members[q]
        G, gb = sb.download(q)
        shape = sb.member_shape(q)
        assert (shape["rows"], shape["cols"]) == G.shape == M0.shape
        ld = ctypes.c_int64(0)
        assert L.mi355x_sbatch_debug_stored(sb._handle, q, None, ctypes.byref(ld)) == capi.MI_OK
        assert ld.value == shape["ld"] == 32
        S = np.full((shape["rows"], ld.value), np.nan, dtype=F32)
        assert L.mi355x_sbatch_debug_stored(sb._handle, q, _p(S), None) == capi.MI_OK
        assert same_bits(S[:, :shape["cols"]], G), q
        assert not np.isnan(S).any(), q                                       # (every stored float was copied)
        st, _, M, basis = sc.solve(M0, b0, True)
        assert st == sc.OPTIMAL and same_bits(G, M) and np.array_equal(gb, basis), q
