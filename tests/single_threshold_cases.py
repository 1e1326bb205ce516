"""Float32 tableaux in which an entry sits exactly AT one of the three single-float thresholds, or one float beyond
it, at a CHOSEN moment of the solve (host only) -- the float twins of the events of tests/threshold_cases.py, and the
float32 model's answers to them.

The single-float path decides by strict comparisons against (f/8) eps_s, 0 + (f/2) eps_s and f eps_s, all computed in
float from single-float-epsilon = 2^-24 (1 + 2^-23) (sc.thresholds): a column enters only if key < 0 - ptol, a row is
eligible only if thr < a, and the step between the phases goes on only if |0 - objective| <= f eps_s.  Uniform floats
never come near any of them.  Everything is built from tests/single_cases.py (`synthetic`, `solve`, `two_phase`,
`thresholds`); nothing here touches the library.  Every function is cached and what it returns is read-only.

Events ("step j" = pivot index j of the model's trace on the planted tableau):
  T   ratio threshold at step j >= 1.  Row R has structural entries 0; X, the structural column the model brings in at
      step j for the first time, gets M[R, X] = thr (`at`) or nextafter(thr, inf) (`beyond`), and b[R] = M[R, X] *
      2^-10, rounded to float.  No earlier pivot touches row R (its entry in every earlier entering column is 0).
      `at`: R is not eligible, step j is the base's.  `beyond`: step j pivots on (X, R); the numbers stay finite.
      R lies in a LATER trip or wave of the gather than the ordinary winner (t_unit), or is row 0 / the last row.
      The builder searches j upwards from the spec's j0 for such a step and the host file asserts what it found (at
      300 x 6 that is j = 1: at j = 2 the base's own row, 293, shares R's trip; at 61 x 97 j = 20 names a column that
      had entered before and j = 21 is taken).
  P   pricing threshold at the LAST step.  Column Y is zero but for its key sgn (0 - ptol) (`at`) or one float beyond
      (`beyond`); it is zero in every pivot row, so its key keeps its bits.  `at`: OPTIMAL after k_end pivots.
      `beyond`: Y enters at step k_end and has no eligible row: the same trace, then UNBOUNDED.
  F   feasibility threshold.  A pair whose phase 1 has nothing to price in; the artificial objective entry is
      +-f eps_s (`at`: the hand-over is made and the main solve runs) or one float beyond in magnitude (`beyond`:
      INFEASIBLE, no hand-over).
  Q   a pair of F's shape whose phase 1 really pivots under min and then ends on a P event: the sgn = -1 threshold
      of the artificial tableau.

A min case is its max twin with the objective row mirrored: the same pivots.  Every case carries its tolerance
factor; 1000.3 is no float32, the model rounds it first (F32(factor)).  tests/test_single_threshold_cases_host.py
asserts on the model alone that every case is what it claims and that every list below tells seven wrong models
from the right one."""
import functools
from collections import namedtuple

import numpy as np

from tests import single_cases as sc

F32 = np.float32
F, F_SMALL, F_LARGE, F_ROUNDS, F_NO_FLOAT = 1024, 16, 2.0 ** 20, 1000, 1000.3
FACTORS = (F, F_SMALL, F_LARGE, F_ROUNDS, F_NO_FLOAT)
CAP = 400                                                    # every model solve here ends far below it

# ev "T" | "P" | None (an untouched synthetic member: `seed`); var "at" | "beyond"; row (T) "named" | "first" | "last";
# j0 (T) the first step tried; mult (T) the step must be a multiple of it
Spec = namedtuple("Spec", "ev var m n f is_max slack row j0 mult seed",
                  defaults=(True, True, "named", 1, 1, None))
# case: (M0, b0, is_max, cap, (status, trace, M, basis)); j: the event step (P: k_end); w: the base's row at step j
Planted = namedtuple("Planted", "case f R X Y j w base_trace")


def spec_id(s):
    if s.ev is None:
        return "%dx%d-plain%s" % (s.m, s.n, s.seed)
    return "%dx%d%s-%s(%s)-%s-f%g%s" % (s.m, s.n, "" if s.slack else "-noslack", s.ev, s.var, "max" if s.is_max else "min",
                                       s.f, "" if s.row == "named" or s.ev != "T" else "-" + s.row) + \
        ("" if s.j0 == 1 else "-j%d" % s.j0) + ("" if s.mult == 1 else "-x%d" % s.mult) + ("" if s.seed is None else "-s%d" % s.seed)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _pairs(trace):
    return [tuple(int(v) for v in x) for x in trace]


def beyond(x):
    """The next float32 away from zero."""
    return np.nextafter(F32(x), F32(np.inf) if x > 0 else F32(-np.inf))


def base_tableau(m, n, is_max=True, slack=True, seed=None):
    """sc.synthetic(n, m); slack=False leaves the slack columns out ([A | b ; -c | 0], basis entries all 0: the same
    arithmetic and scans, and the only way to 1101 rows inside the LDS budget); min: the mirrored objective row."""
    M0, b0 = sc.synthetic(n, m, seed)
    M0 = M0.copy()
    if not slack:
        M0 = np.ascontiguousarray(np.delete(M0, np.s_[n:n + m], axis=1))
        b0 = np.zeros(m, dtype=np.int64)
    if not is_max:
        M0[-1] = -M0[-1]
    return M0, b0


def t_row(m, row):
    """R: row 1090 of 1100 and 290 of 300 (a later trip of 1024 / 256 threads), else the last row; or row 0."""
    return {"first": 0, "last": m - 1}.get(row, {1100: 1090, 300: 290}.get(m, m - 1))


def t_unit(m):
    """The rows one trip (1100, 300 rows) or one wave (above 64 rows) of the gather covers; None: one wave holds all."""
    return 1024 if m > 1024 else 256 if m > 256 else 64 if m > 64 else None


def p_column(n):
    """Y: a later trip than column 0's at 1024 threads (n >= 4200: column 4100 / 8200, quads beyond 1023; 4100 is a
    later trip at 256 threads too), a later wave at 300 columns, else the last structural column."""
    return {8300: 8200, 4200: 4100, 300: 290}.get(n, n - 1)


def _case(M0, b0, is_max, f):
    st, tr, M, b = sc.solve(M0, b0, is_max, f, CAP)
    _frozen(M0, b0, M, b)
    return M0, b0, is_max, CAP, (st, _pairs(tr), M, b)


@functools.lru_cache(maxsize=None)
def planted(spec):
    """The planted tableau of a spec with the model's answer and the indices of its event."""
    ev, var, m, n, f, is_max, slack, row, j0, mult, seed = spec
    ptol, thr, _ = sc.thresholds(f)
    M0, b0 = base_tableau(m, n, is_max, slack, seed)
    if ev is None:
        return Planted(_case(M0, b0, is_max, f), f, None, None, None, None, None, None)
    if ev == "P":
        Y = p_column(n)
        M0[:, Y] = 0
        key = F32(F32(0) - ptol)
        M0[m, Y] = (key if var == "at" else beyond(key)) * F32(1 if is_max else -1)
        case = _case(M0, b0, is_max, f)
        return Planted(case, f, None, None, Y, len(case[4][1]), None, None)
    assert ev == "T"
    R, unit = t_row(m, row), t_unit(m)
    M0[R, :n] = 0
    base = _pairs(sc.solve(M0, b0, is_max, f, j0 + 60)[1])
    for j in range(max(j0, 1), len(base)):                   # the first step with a fresh structural column whose
        X, w = base[j]                                       # ordinary winner lies in an earlier trip than R
        early = w != R if unit is None or R == 0 else w // unit < R // unit
        if j % mult == 0 and X < n and all(c != X for c, _ in base[:j]) and early:
            break
    else:
        raise AssertionError("no step of %s has a fresh structural column" % (spec_id(spec),))
    M0[R, X] = thr if var == "at" else beyond(thr)
    M0[R, -1] = F32(M0[R, X] * F32(2.0 ** -10))
    return Planted(_case(M0, b0, is_max, f), f, R, X, None, j, w, base[:j + 1])


# ------------------------------------------------------------------ the single-tableau lists, one per path
def _t(var, m, n, f, **kw):
    return Spec("T", var, m, n, f, **kw)


def _p(var, m, n, f, **kw):
    return Spec("P", var, m, n, f, **kw)


# k_s_select<256> + k_s_update: 301 rows with slack columns (a second trip of the gather), 61 x 97 and 96 x 300
PAIR_256 = [_t("at", 300, 6, F), _t("beyond", 300, 6, F_ROUNDS), _t("at", 300, 6, F_SMALL, is_max=False),
            _t("at", 61, 97, F_NO_FLOAT, is_max=False, j0=20), _t("beyond", 61, 97, F_SMALL, j0=20),
            _t("at", 96, 300, F_LARGE, j0=30), _t("beyond", 96, 300, F, is_max=False, j0=25),
            _p("at", 61, 97, F_ROUNDS), _p("beyond", 61, 97, F, is_max=False),
            _p("at", 96, 300, F_SMALL, is_max=False), _p("beyond", 96, 300, F_NO_FLOAT)]
# k_s_select<1024> + k_s_update: 1101 rows with slack columns, 8304 floats per row
PAIR_1024 = [_t("at", 1100, 6, F_ROUNDS, j0=2), _t("beyond", 1100, 6, F, j0=2), _t("at", 1100, 6, F_SMALL, is_max=False),
             _t("beyond", 1100, 6, F_LARGE, is_max=False),
             _p("at", 3, 8300, F), _p("beyond", 3, 8300, F_ROUNDS), _p("at", 3, 8300, F_NO_FLOAT, is_max=False),
             _p("beyond", 3, 8300, F_SMALL, is_max=False)]
# k_s_solve: (spec, chunk); chunk = 5 with the event step a multiple of 5: the first step after the tableau comes
# back from HBM
LDS_CASES = [(_t("at", 1100, 6, F, slack=False), None), (_t("beyond", 1100, 6, F_NO_FLOAT, slack=False, j0=2), None),
             (_t("at", 1100, 6, F_ROUNDS, slack=False, is_max=False), None),
             (_p("at", 3, 4200, F_ROUNDS), None), (_p("beyond", 3, 4200, F_LARGE), None),
             (_p("beyond", 3, 4200, F, is_max=False), None),
             (_t("at", 96, 300, F_SMALL, j0=30), None), (_t("beyond", 96, 300, F_ROUNDS, j0=20), None),
             (_p("at", 96, 300, F), None), (_p("beyond", 96, 300, F_SMALL, is_max=False), None),
             (_t("at", 96, 300, F_ROUNDS, j0=20, mult=5), 5), (_t("beyond", 96, 300, F, j0=20, mult=5, is_max=False), 5),
             (_p("at", 96, 300, F_ROUNDS, seed=2), 5), (_p("beyond", 61, 97, F, seed=5, is_max=False), 5)]
# k_s_price_only / k_s_ratio_only (1024 threads): walked along the model's trace up to the event step
STEPWISE = [_t("at", 1100, 6, F_ROUNDS), _t("beyond", 1100, 6, F_NO_FLOAT, is_max=False),
            _p("at", 3, 8300, F_NO_FLOAT, is_max=False), _p("beyond", 3, 8300, F_ROUNDS)]


# ------------------------------------------------------------------ batches: members of one shape, ONE factor per call
# (event, variant, row, first step tried): T-at, T-beyond in row 0, T-beyond in the last row, P-at, P-beyond, two
# untouched ones, T-at in row 0
BATCH_MEMBERS = [("T", "at", "named", 3), ("T", "beyond", "first", 5), ("T", "beyond", "last", 2), ("P", "at", None, None),
                 ("P", "beyond", None, None), None, None, ("T", "at", "first", 4)]
# (m, n, slack): (is_max, factor, events kept); 3 x 4200 holds P members only, 1100 x 6 without slack T members only
BATCHES = {(24, 40, True): (True, F, "TP"), (96, 300, True): (False, F_ROUNDS, "TP"),
           (3, 4200, True): (True, F_NO_FLOAT, "P"), (1100, 6, False): (False, F_SMALL, "T")}


def batch_specs(m, n, slack):
    is_max, f, events = BATCHES[(m, n, slack)]
    tall = m > 1024                                          # (three pivots in all: the events fall at steps 1 and 2)
    specs = []
    for k, member in enumerate(BATCH_MEMBERS):
        if member is None:
            specs.append(Spec(None, None, m, n, f, is_max, slack, seed=100 + k))
        elif member[0] in events:
            ev, var, row, j0 = member
            if ev == "T":
                specs.append(Spec("T", var, m, n, f, is_max, slack, row, (1 + j0 % 2) if tall else j0 + (20 if m == 96 else 0)))
            else:
                specs.append(Spec("P", var, m, n, f, is_max, slack))
    return specs


def batch_cases(m, n, slack):
    return [planted(s).case for s in batch_specs(m, n, slack)]


# ------------------------------------------------------------------ F and Q: pairs for the step between the phases
PAIR_FACTORS = (F, F_ROUNDS)
F_NAMES = ("F+at", "F-at", "F+beyond", "F-beyond")
BETWEEN_MEMBERS = F_NAMES + ("H0", "Q-at", "Q-beyond")


def _small_pair():
    """sc.small_pairs()' OPTIMAL member (3 x 6 artificial, 3 x 5 main: x + y <= 3.5, x >= 0.5, max x + 0.5 y), copied."""
    return [np.array(a) for a in sc.small_pairs()[2]]


@functools.lru_cache(maxsize=None)
def pair_case(name, f):
    """-> ((art, art basis, main, main basis), the model's two_phase answer under factor f).
    F    the artificial tableau as phase 1 leaves it (no artificial basic), its objective row made <= 0 so that phase 1
         has nothing to price in, and the artificial objective entry +-f eps_s (`at`) or one float beyond.
    Q    y's column zeroed in both tableaux; its artificial objective entry is +ptol (`at`: not priced in under min) or
         one float beyond (`beyond`: phase 1 pivots on x, then brings y in and ends UNBOUNDED).  Phase 1 pivots once on
         (x, row 1) and leaves that entry untouched (the pivot row is 0 in column y).
    H0   the unchanged pair."""
    ptol, _, feas = sc.thresholds(f)
    A, ab, M, mb = _small_pair()
    m, nav = A.shape[0] - 1, A.shape[1] - 1
    if name in F_NAMES:
        st, tr, A, ab = sc.solve(A, ab, False, f)
        assert st == sc.OPTIMAL and tr and (ab < M.shape[1] - 1).all()
        A[m, :nav] = -np.abs(A[m, :nav])
        A[m, nav] = (feas if name.endswith("at") else beyond(feas)) * F32(1 if name[1] == "+" else -1)
    elif name[0] == "Q":
        A[:m, 1] = M[:, 1] = 0
        A[m, 1] = ptol if name == "Q-at" else beyond(ptol)
    else:
        assert name == "H0"
    _frozen(A, ab, M, mb)
    want = sc.two_phase(A, ab, M, mb, True, f)
    for key in ("art_trace", "main_trace"):
        want[key] = _pairs(want[key])
    _frozen(want["A"], want["abasis"], want["M"], want["mbasis"])
    return (A, ab, M, mb), want


# ------------------------------------------------------------------ the public routes
@functools.lru_cache(maxsize=None)
def edge_problem(f, var):
    """max c x  s.t. x <= 1 with c exactly the pricing threshold of factor f (`at`: 0 pivots, the objective 0) or one
    float above it (`beyond`: one pivot, the objective c) -- sc.tiny_coefficient_problem moved onto the edge."""
    ptol = sc.thresholds(f)[0]
    return dict(type="max", vars=["x"], objective_var="z", objective=[("x", ptol if var == "at" else beyond(ptol))],
                bounds=[], constraints=[("<=", [("x", 1)], 1)])


# (route, factor): solve_problem, solve_problems (both problems as one group) and single_lps.solve_lps_single
PUBLIC = [("solve_problem", F_SMALL), ("solve_problems", F_NO_FLOAT), ("solve_lps_single", F_ROUNDS)]


# ------------------------------------------------------------------ what each path of the table is given
def answer(item):
    """(status, trace or traces) of the model on an item of ROWS: a Spec, (pair name, f) or (edge_problem variant, f).
    It solves the INPUTS again, so under a patched model (the host file's mutants) it is that model's answer."""
    if isinstance(item, Spec):
        M0, b0, is_max, cap, _ = planted(item).case
        st, tr, _, _ = sc.solve(M0, b0, is_max, item.f, cap)
        return st, _pairs(tr)
    name, f = item
    if name in ("at", "beyond"):
        r = sc.solve_problem(edge_problem(f, name), f)
        return r["status"], _pairs(r["trace"])
    (A, ab, M, mb), _ = pair_case(name, f)
    r = sc.two_phase(A, ab, M, mb, True, f)
    return r["status"], _pairs(r["art_trace"]), _pairs(r["main_trace"])


def event_of(item):
    return item.ev if isinstance(item, Spec) else "F" if item[0][0] == "F" else None if item[0] == "H0" else "P"


ROWS = {
    "k_s_select<256> + k_s_update": PAIR_256,
    "k_s_select<1024> + k_s_update": PAIR_1024,
    "k_s_solve": [s for s, _ in LDS_CASES],
    "k_s_price_only / k_s_ratio_only": STEPWISE,
    "k_sb_solve": [s for shape in BATCHES for s in batch_specs(*shape)],
    "tp_feasible<float>": [(name, f) for f in PAIR_FACTORS for name in F_NAMES],
    "k_sb_between": [(name, f) for f in PAIR_FACTORS for name in BETWEEN_MEMBERS],
    "public routes": [(var, f) for _, f in PUBLIC for var in ("at", "beyond")],
}
