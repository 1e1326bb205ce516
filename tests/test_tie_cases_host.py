"""tests/tie_cases.py checked on the oracle alone (no GPU): every case tests/test_gpu_ties.py uses really
meets exact ties -- often enough, at a non-zero quotient, between indices exactly as far apart as the case
says.  These are conditions on the INPUTS (the seeds in tie_cases.py were picked so that they hold); what a
kernel makes of the ties is test_gpu_ties.py's business.

Slot order against logical order: in every compact case the census also follows the slots of the non-basic
columns and counts the tied pricing steps at which the lower LOGICAL column sat in the HIGHER slot (between
twins it never does; the gadgets of tie_cases.py provide these steps): at least one per gadget -- 6 per single
tableau (4 on the 40-row shapes), 2 per batch member with duplicates -- with the winner in the last slots and
its partner in the first, i.e. in another wave, workgroup, exchange record, strip and shard in every case."""
import functools

import numpy as np
import pytest

import oracle
from tests import tie_cases as tc

SINGLE_MIN_TIES = 12                                       # tied pricing steps / tied non-zero ratio steps per case
MEMBER_MIN_TIES = 4                                        # ... per batch member

DENSE = sorted(set(tc.COLPART.values()))
SINGLE = [(case, False) for case in tc.SEEDS] + [(case, True) for case in DENSE]


@functools.lru_cache(maxsize=None)
def _census(case, dense):
    M0, b0 = tc.single(*case, "max", dense)
    return tc.census(M0, b0)


def _ids(params):
    return ["%dx%d-r%d-c%d%s" % (case + ("-dense" if dense else "",)) for case, dense in params]


@pytest.mark.parametrize("case,dense", SINGLE, ids=_ids(SINGLE))
def test_single_case_has_the_ties_it_claims(case, dense):
    n, m, row_d, col_d = case
    c = _census(case, dense)
    G = tc.gadgets_of(case)
    ref = tc.single_reference(*case, "max", dense)
    assert c.pivots == ref.pivots and np.array_equal(c.trace, ref.trace)      # the replay IS the oracle's solve
    twins = [p for p in c.price_pairs if p[0] >= G]                           # tied steps between duplicated columns
    assert len(twins) >= SINGLE_MIN_TIES and all(p[1] - p[0] == col_d for p in twins), c[:7]
    assert c.ratio_ties_nonzero >= SINGLE_MIN_TIES and c.ratio_ties_nonzero == c.ratio_ties, c[:7]
    assert c.ratio_dist == (row_d, row_d), c[:7]
    if dense:                                                                 # (no slots; the doubled basic column u is no copy of j)
        assert len(twins) == c.price_ties
    else:
        _gadget_ties_invert_the_slots(c, G, n, col_d)
    # the min form is the same LP with the objective row negated: the same pivots, hence the same ties
    # (negation is exact, and rounding is symmetric in the sign)
    ref_min = tc.single_reference(*case, "min", dense)
    assert (ref_min.status, ref_min.pivots) == (ref.status, ref.pivots) and np.array_equal(ref_min.trace, ref.trace)
    assert np.array_equal(ref_min.M[:-1], ref.M[:-1]) and np.array_equal(ref_min.M[-1], -ref.M[-1])


def _gadget_ties_invert_the_slots(c, G, n, col_d):
    """Every tied pricing step is between twins (distance col_d) or a gadget's (u, j), u < G; each gadget
    gives one, with u -- the winner, the lower logical column -- in D1's slot, one of the last G, and j in one
    of the first G."""
    gadget = [p for p in c.price_pairs if p[0] < G]
    assert sorted(p[0] for p in gadget) == list(range(G)), gadget
    for w, p, ws, ps in gadget:
        assert (p, ws, ps) == (G + w, n - G + w, w), (w, p, ws, ps)
    assert c.inverted >= G                                 # (a twin that left the basis and came back may add more)


@pytest.mark.parametrize("shards", sorted(tc.COLPART))
@pytest.mark.parametrize("dense", [False, True], ids=["compact", "dense"])
def test_column_partition_ties_cross_shards(shards, dense):
    """Compact shards hold the slots in contiguous parts: the twins' ties have the partner in a later shard
    (all of them while neither twin has moved), a gadget's tie has the winner in the last shard and the partner in
    the first.  Dense shards deal out all columns: at least SINGLE_MIN_TIES tied steps
    cross shards (the others meet inside one shard's reduction)."""
    case = tc.COLPART[shards]
    n, m, _, col_d = case
    assert col_d == -(-n // shards)
    c = _census(case, dense)
    G = tc.gadgets_of(case)
    # dense shards hold logical columns, compact shards slots (a leaving column takes the entering one's slot)
    where = [(tc.shard_of(a, n + m, shards), tc.shard_of(b, n + m, shards)) if dense else
             (tc.shard_of(sa, n, shards), tc.shard_of(sb, n, shards)) for a, b, sa, sb in c.price_pairs]
    twins = [w for w, p in zip(where, c.price_pairs) if p[0] >= G]
    crossing = [w for w in twins if w[0] < w[1]]
    assert len(crossing) >= SINGLE_MIN_TIES, (len(crossing), len(twins))
    if not dense:
        gadget = [w for w, p in zip(where, c.price_pairs) if p[0] < G]
        assert len(gadget) == G and all(w == (shards - 1, 0) for w in gadget)  # winner in the LAST shard, partner in the first


def test_shard_of_is_the_library_partition():
    for count, shards in ((700, 2), (700, 3), (700, 8), (1033, 8), (5, 5)):
        base, extra = divmod(count, shards)
        bounds = [r * base + min(r, extra) for r in range(shards + 1)]       # cp_partition
        for col in range(count):
            r = tc.shard_of(col, count, shards)
            assert bounds[r] <= col < bounds[r + 1]


BATCH = sorted(tc.BATCH_SEEDS)


@pytest.mark.parametrize("case", BATCH, ids=["%dx%d-r%d-c%d" % c for c in BATCH])
def test_batch_members_have_the_ties_they_claim(case):
    n, m, row_d, col_d = case
    Ms, Bs = tc.batch(*case, "max")
    assert Ms.shape[0] == tc.BATCH_MEMBERS
    full = tc.batch_reference(*case, "max", 0)
    pivots = set()
    for k in range(tc.BATCH_MEMBERS):
        c = tc.census(Ms[k], Bs[k], cap=tc.BATCH_UNCAPPED_LIMIT)
        assert c.status != oracle.MAX_PIVOTS, (k, c[:7])                      # the uncapped solve ends
        assert (full[k].status, full[k].pivots) == (c.status, c.pivots) and np.array_equal(full[k].trace, c.trace)
        pivots.add(c.pivots)
        if k == tc.BATCH_MEMBERS - 1:                                         # the member without duplicates
            assert (c.price_ties, c.ratio_ties) == (0, 0), (k, c[:7])
            continue
        twins = [p for p in c.price_pairs if p[0] >= tc.MEMBER_GADGETS]
        assert all(p[1] - p[0] == col_d for p in twins)
        assert len(twins) >= MEMBER_MIN_TIES and c.ratio_ties_nonzero >= MEMBER_MIN_TIES, (k, c[:7])
        assert c.ratio_ties_nonzero == c.ratio_ties and c.ratio_dist == (row_d, row_d), (k, c[:7])
        _gadget_ties_invert_the_slots(c, tc.MEMBER_GADGETS, n, col_d)
    assert len(pivots) > 2                                                    # members finish at different times


@pytest.mark.parametrize("hi", tc.SZ_HIGHER, ids=["same-wave", "other-wave"])
@pytest.mark.parametrize("negative_in_lower_row", [False, True], ids=["lower+0-higher-0", "lower-0-higher+0"])
def test_signed_zero_case_on_the_oracle(negative_in_lower_row, hi):
    M0, b0 = tc.signed_zero_case(negative_in_lower_row, hi)
    M, b = M0.copy(), b0.copy()
    lo, col = tc.SZ_LO, tc.SZ_COL
    assert lo // 64 == tc.SZ_HIGHER[0] // 64 != tc.SZ_HIGHER[1] // 64
    assert np.signbit(M[lo, -1]) == negative_in_lower_row and np.signbit(M[hi, -1]) != negative_in_lower_row
    assert oracle.price(M) == col
    thr = 512 * oracle.EPSILON
    assert M[lo, col] > thr and M[hi, col] > thr and (M[:-1, -1] == 0.0).sum() == 2
    assert oracle.ratio(M, col) == lo                                         # equal keys: the lowest row
    oracle.pivot(M, b, col, lo)
    assert b[lo] == col
    # the bits keep the signs: 0 / pivot in the pivot row, x - a * 0 in the other one
    assert M[lo, -1] == 0.0 and np.signbit(M[lo, -1]) == negative_in_lower_row
    assert M[hi, -1] == 0.0 and np.signbit(M[hi, -1]) != negative_in_lower_row
    c = tc.census(M0, b0)
    assert tuple(c.trace[0]) == (col, lo) and c.ratio_dist[0] <= hi - lo and c.status == oracle.OPTIMAL
