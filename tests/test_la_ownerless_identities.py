"""Why k_la_block needs no owner for the objective row and for the RHS column (csrc/kernels_la_block.inc).

The persistent look-ahead keeps, per step J of a block, the objective row `z` and the RHS column `b` up to
date through the pending pivots, and chains the entering column col_J and the pivot row prow_J from the
stored tableau through the same pending pivots.  Two entries are then available twice:

    col_J[m]   (objective-row entry of the entering column)  ==  z[slot_J]
    M[cr][vc]  chained (RHS entry of the pivot row, before the division by the pivot)  ==  b[cr_J]

bit for bit -- the same reset-or-subtract on the same operands in the same order.  This file replays a block
of 24 pending pivots in numpy float64 (product and difference rounded separately, as the kernels are built)
the way the kernel keeps its state, and asserts both identities at every step, including a pivot whose
entering slot an earlier pending pivot gave up and a pivot row that is an earlier pending pivot's row."""
import numpy as np
import pytest

BLOCK = 24


def _link(x, is_slot, is_cr, colv, rowv):
    """la_link / pend: element x under pending pivot i (colv = col_i[row], rowv = prow_i[column])."""
    x = np.where(is_slot, np.where(is_cr, 1.0, 0.0), x)
    prod = colv * rowv                                     # rounded product
    d = x - prod                                           # rounded difference
    return np.where(is_cr, rowv, d)


def _replay(n, m, seed, forced):
    """forced: {step: ("slot" | "row", earlier step)} -- reuse that pivot's slot / row."""
    rng = np.random.default_rng(seed)
    vc = n                                                 # compact tableau: n non-basic columns, then the RHS
    M = rng.uniform(-2.0, 2.0, (m + 1, vc + 1)) * 10.0 ** rng.integers(-3, 4, (m + 1, vc + 1))
    z = M[m].copy()                                        # objective row (pair side)
    b = M[:m, vc].copy()                                   # RHS column (row side)
    rows, cols = np.arange(m + 1), np.arange(vc + 1)
    col, prow, crs, slots = [], [], [], []
    for J in range(BLOCK):
        slot = int(rng.integers(0, vc))
        cr = int(rng.integers(0, m))
        if J in forced:
            kind, i = forced[J]
            if kind == "slot":
                slot = slots[i]
            else:
                cr = crs[i]
        # ---- entering column through the pending chain (row side, every row up to the objective row)
        a = M[:, slot].copy()
        for i in range(J):
            a = _link(a, slots[i] == slot, rows == crs[i], col[i], prow[i][slot])
        # identity 1: the objective-row entry is the pair side's z[slot]
        assert z[slot].tobytes() == a[m].tobytes(), (J, slot, z[slot], a[m])
        cmj = z[slot]
        piv = a[cr]
        assert piv != 0.0 and np.isfinite(piv)
        # ---- pivot row through the pending chain (pair side, every column up to the RHS)
        y = M[cr].copy()
        for i in range(J):
            y = _link(y, cols == slots[i], crs[i] == cr, col[i][cr], prow[i])
        # identity 2: the RHS entry before the division is the row side's b[cr]
        assert b[cr].tobytes() == y[vc].tobytes(), (J, cr, b[cr], y[vc])
        y[slot] = 1.0                                      # scale_pair: the slot takes the leaving unit column
        pr = y / piv
        assert (b[cr] / piv).tobytes() == pr[vc].tobytes()
        # ---- the kept state through pivot J
        z = _link(z, cols == slot, False, cmj, pr)
        b = _link(b, False, rows[:m] == cr, a[:m], pr[vc])
        col.append(a); prow.append(pr); crs.append(cr); slots.append(slot)
    # the replay is the blocked update: applying the pivots one by one to the tableau gives z and b
    T = M.copy()
    for i in range(BLOCK):
        c, p = T[:, slots[i]].copy(), T[crs[i]].copy()
        p[slots[i]] = 1.0
        p = p / c[crs[i]]
        unit = np.where(rows == crs[i], 1.0, 0.0)
        T[:, slots[i]] = unit
        newT = T - c[:, None] * p[None, :]
        newT[crs[i]] = p
        T = newT
    assert T[m].tobytes() == z.tobytes()
    assert T[:m, vc].tobytes() == b.tobytes()
    return slots, crs


@pytest.mark.parametrize("n,m,seed", [(62, 40, 1), (61, 40, 2), (33, 70, 3)], ids=["even-vc", "odd-vc", "tall"])
def test_objective_and_rhs_entries_are_held_twice(n, m, seed):
    forced = {5: ("slot", 2), 9: ("row", 4), 14: ("slot", 5), 15: ("row", 9), 20: ("slot", 3), 21: ("row", 3)}
    slots, crs = _replay(n, m, seed, forced)
    assert slots[5] == slots[2] and slots[14] == slots[2]          # a slot an earlier pending pivot gave up (twice over)
    assert crs[9] == crs[4] and crs[15] == crs[4]                  # the row of an earlier pending pivot
    assert slots[20] == slots[3] and crs[21] == crs[3]
