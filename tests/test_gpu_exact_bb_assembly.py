"""mi355x_xbatch_create_nodes on the GPU: every entry T / D and both bases of every member, downloaded
before any solve, against rational_ref.build_tableau of the node problem (tests/exact_bb_cases.py; the
same expectation is pinned against the host restatement in test_exact_bb_host.py)."""
import ctypes
import importlib
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_bb_cases as X
from tests.helpers import lp_amd

pytestmark = pytest.mark.gpu
lp = lp_amd()
xbb = importlib.import_module("linear-programming_amd.exact_bb")
_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _download(xb, q):
    R, C = xb.rows, xb.cols
    T = np.empty(R * C * 2, dtype=np.int64)
    D = np.empty(2, dtype=np.int64)
    b = np.empty(R - 1, dtype=np.int64)
    lp.exact.check(lp.capi.lib().mi355x_xbatch_download(xb.handle, q, _ptr(T), _ptr(D), _ptr(b)), "download")
    to_int = lp.exact._int128
    d = to_int(D[0], D[1])
    vals = [Fraction(to_int(lo, hi), d) for lo, hi in T.reshape(-1, 2).tolist()]
    return [vals[r * C:(r + 1) * C] for r in range(R)], b.tolist(), d


def _bits(xb, q):
    b = ctypes.c_int(0)
    lp.capi.check(lp.capi.lib().mi355x_xbatch_bits(xb.handle, q, ctypes.byref(b)), "bits")
    return b.value


@pytest.mark.parametrize("min_bits", (0, 128))
@pytest.mark.parametrize("name", X.ASSEMBLY_CASES)
def test_assembled_members_are_build_tableau_of_the_node_problems(name, min_bits):
    p, nodes = X.assembly_case(name)
    g = xbb.GeneralForm(p)
    base = xbb.Base(g)
    main, art = base.create_nodes(nodes, min_bits)
    bits = []
    for q, e in enumerate(nodes):
        rm, rmb, ra, rab = X.reference_tableaux(p, e)
        M, mb, d = _download(main, q)
        assert d == g.Db and M == rm and mb == rmb, (name, q)
        assert (art is None) == (ra is None)
        if art is not None:
            A, ab, d = _download(art, q)
            assert d == g.Db and A == ra and ab == rab, (name, q)
            assert _bits(art, q) == _bits(main, q)
        bits.append(_bits(main, q))
    if min_bits == 128:
        assert bits == [128] * len(nodes)
    elif name == "big_scale":
        assert bits == [128, 128, 64]          # bound * Db leaves 64 bits for the first two members only
    else:
        assert bits == [64] * len(nodes)


def test_nodes_of_different_groups_are_refused():
    p, nodes = X.assembly_case("small_d1_art")
    base = xbb.Base(xbb.GeneralForm(p))
    v, s, b = nodes[0][0]
    with pytest.raises(lp.capi.Mi355xError):
        base.create_nodes([nodes[0], ((v, 1 - s, b),)])
