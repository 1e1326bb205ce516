"""The mixed lists of tests/test_single_ragged_host.py and tests/test_gpu_single_ragged.py: members of different
shapes and senses for ONE ragged single-float batch, with the answers of the float32 model (tests/single_cases.py),
computed once per process and read-only.  Nothing here touches the library.

Shapes are m x n (constraints x variables) of sc.synthetic: the tableau is (m + 1) x (n + m + 1)."""
import functools

import numpy as np

from tests import single_cases as sc

F32 = np.float32
CAP = 2000                                                   # every model solve here ends far below it
#: (m, n) and the dynamic LDS of the member (single_lds_bytes): four size bands, so four residencies per compute unit
BANDS = (((24, 40), 7184), ((61, 97), 40576), ((64, 150), 57296), ((80, 200), 93488))
#: position -> band: neighbours differ in band, and every band is once at an even and once at an odd position
MIXED_ORDER = (0, 1, 2, 3, 1, 0, 3, 2)
#: (m, n) of the members of the long list: cols 13, 16, 15, 6 -- every residue mod 4 -- and rows - 1 = 5, 6, 3, 1
SMALL_CYCLE = ((5, 7), (6, 9), (3, 11), (1, 4))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def member(m, n, seed, is_max, cap=CAP):
    """-> ((M0, b0, is_max), the model's (status, trace, M, basis)); a min member is the mirrored max problem."""
    M0, b0 = sc.synthetic(n, m, seed=seed)
    if not is_max:
        M0[-1] = -M0[-1]
    want = sc.solve(M0, b0, is_max, 1024, cap)
    _frozen(M0, b0, want[2], want[3])
    return (M0, b0, is_max), want


@functools.lru_cache(maxsize=None)
def mixed(cap=CAP):
    """Eight members: the four bands, two seeds each, the senses alternating (position k is a max problem for even k),
    so neighbours differ in band and in sense and every band has a member of either sense."""
    seen, ins, wants = {}, [], []
    for k, band in enumerate(MIXED_ORDER):
        (m, n), _ = BANDS[band]
        seen[band] = seen.get(band, 0) + 1
        i, w = member(m, n, seen[band], k % 2 == 0, cap)
        ins.append(i)
        wants.append(w)
    return tuple(ins), tuple(wants)


@functools.lru_cache(maxsize=None)
def small_cycle(count=1100):
    ins, wants = [], []
    for k in range(count):
        m, n = SMALL_CYCLE[k % len(SMALL_CYCLE)]
        i, w = member(m, n, k + 1, k % 3 != 0)
        ins.append(i)
        wants.append(w)
    return tuple(ins), tuple(wants)


@functools.lru_cache(maxsize=None)
def one_shape(count=6):
    """Members of ONE shape and sense (24 x 40, max): the ragged batch against the batch of one shape."""
    pairs = [member(24, 40, seed, True) for seed in range(1, count + 1)]
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


@functools.lru_cache(maxsize=None)
def tie_members():
    """3 x 1100 with ties across the wave and trip boundaries of pricing, 300 x 6 without slack columns with ties
    across rows 63 | 64 and 255 | 256 (as in tests/test_gpu_single_batch.py), beside a 5 x 7 member."""
    ins, wants = [], []
    for n, m, cols, rows, slack in ((1100, 3, (255, 256), (1, 2), True), (6, 300, (2, 4), (63, 64), False),
                                    (1100, 3, (1023, 1024), (0, 2), True), (6, 300, (2, 4), (255, 256), False)):
        M0, b0 = sc.tie_tableau(n, m, tied_cols=cols, tied_rows=rows, slack=slack)
        want = sc.solve(M0, b0, True, cap=10)
        assert tuple(int(x) for x in want[1][0]) == (cols[0], rows[0]) and len(want[1]) >= 2
        _frozen(M0, b0, want[2], want[3])
        ins.append((M0, b0, True))
        wants.append(want)
    i, w = member(5, 7, 3, True, cap=10)
    ins.insert(2, i)
    wants.insert(2, w)
    return tuple(ins), tuple(wants)


OUTCOME_CAP = 7


@functools.lru_cache(maxsize=None)
def outcome_members():
    """Under a cap of 7 pivots per member: an unbounded member, two 24 x 40 members the cap stops (one of each sense),
    a member with a NaN in column 0 of its objective row, each beside members that end optimal."""
    ins, wants = [], []

    def add(M0, b0, is_max):
        want = sc.solve(M0, b0, is_max, 1024, OUTCOME_CAP)
        _frozen(M0, b0, want[2], want[3])
        ins.append((M0, b0, is_max))
        wants.append(want)

    for m, n, seed, is_max, change in (
            (5, 7, 1, True, None), (6, 9, 2, True, "unbounded"), (24, 40, 2, True, None), (3, 11, 3, False, None),
            (6, 9, 4, False, "nan"), (24, 40, 3, False, None), (1, 4, 5, True, None), (24, 40, 6, True, None)):
        M0, b0 = sc.synthetic(n, m, seed=seed)
        if change == "unbounded":
            M0[:m, 2] = -M0[:m, 2]                           # no eligible row in the most attractive column ...
            M0[m, 2] = F32(-50)                              # ... and it is the one that enters
        if not is_max:
            M0[-1] = -M0[-1]
        if change == "nan":
            M0[-1, 0] = F32("nan")
        add(M0, b0, is_max)
    return tuple(ins), tuple(wants)


# ------------------------------------------------------------------ two-phase members
PAIR_3 = dict(type="max", vars=["x", "y", "z"], objective_var="w", objective=[("x", 1), ("y", 2), ("z", F32(1.5))],
              bounds=[], constraints=[("<=", [("x", 1), ("y", 1), ("z", 1)], 10), (">=", [("x", 1)], F32(1.5)),
                                      (">=", [("y", 1), ("z", 1)], 2)])
PAIR_4 = dict(type="min", vars=["x", "y"], objective_var="w", objective=[("x", 2), ("y", F32(3.5))], bounds=[],
              constraints=[("=", [("x", 1), ("y", 1)], 4), ("<=", [("x", 1)], 3), (">=", [("y", 1)], F32(0.5)),
                           ("<=", [("x", 1), ("y", 2)], 7)])


@functools.lru_cache(maxsize=None)
def pairs():
    """Seven two-phase members (art, art basis, main, main basis, main_is_max): sc.small_pairs() -- optimal after one
    drive-out pivot, infeasible in phase 1, optimal, unbounded, an artificial left basic at a non-zero level -- with
    a 3-constraint max and a 4-constraint min pair between them, and what sc.two_phase makes of each."""
    small = [p + (True,) for p in sc.small_pairs()]
    built = []
    for d in (PAIR_3, PAIR_4):
        b = sc.build(d)
        built.append((b["art"][0], b["art"][1], b["main"][0], b["main"][1], d["type"] == "max"))
    members = (small[0], built[0], small[1], small[2], built[1], small[3], small[4])
    wants = tuple(sc.two_phase(A, ab, M, mb, is_max) for A, ab, M, mb, is_max in members)
    return members, wants
