"""The list driver behind solve_problems(list), without a GPU and without the library: the two bounded-call loops
and the two grouping helpers of lists.py on scripted input, and the five routes -- default, from_rows, exact, exact
with device_build, precision="single" -- on one mixed list of tiny problems with the batch layer and the
one-problem solvers replaced by scripted stand-ins: which members every batch and every one-by-one call received and
in which order, where every result landed, and what errorp does.

The routing tests use no name of lists.py: they pin what the routes did before their shared parts moved there."""
from collections import namedtuple

import numpy as np
import pytest

from tests.helpers import lp_amd

lp = lp_amd()
capi = lp.capi
OPT, UNB, INF, MAXP, CANC = capi.MI_OPTIMAL, capi.MI_UNBOUNDED, capi.MI_INFEASIBLE, capi.MI_MAX_PIVOTS, capi.MI_CANCELLED


# ------------------------------------------------------------------ the loop by pivots counted
def _scripted(script):
    """call(cap) that hands out script's answers in turn and notes the caps it was given."""
    caps, answers = [], iter(script)

    def call(cap):
        caps.append(cap)
        return next(answers)
    return call, caps


def test_solve_in_chunks_caps_by_the_pivots_counted():
    call, caps = _scripted([(MAXP, 4), (MAXP, 4), (MAXP, 2), (OPT, 9)])
    assert lp.lists.solve_in_chunks(call, 3, 5, 10, chunk=4) == (MAXP, 10)
    assert caps == [4, 4, 2]
    # fewer pivots than granted (a phase ended inside the call): the next cap is what is left of max_pivots
    call, caps = _scripted([(MAXP, 3), (MAXP, 4), (MAXP, 3), (OPT, 9)])
    assert lp.lists.solve_in_chunks(call, 3, 5, 10, chunk=4) == (MAXP, 10)
    assert caps == [4, 4, 3]


def test_solve_in_chunks_ends_at_the_first_other_status():
    call, caps = _scripted([(MAXP, 4), (UNB, 1), (OPT, 9)])
    assert lp.lists.solve_in_chunks(call, 3, 5, 10, chunk=4) == (UNB, 5)
    assert caps == [4, 4]


def test_solve_in_chunks_without_a_cap_stops_on_the_status_alone():
    call, caps = _scripted([(MAXP, 4)] * 5 + [(OPT, 1), (OPT, 9)])
    assert lp.lists.solve_in_chunks(call, 3, 5, 0, chunk=4) == (OPT, 21)
    assert caps == [4] * 6


def test_the_default_chunk_is_chunk_pivots_of_the_shape():
    assert lp.simplex.chunk_pivots is lp.lists.chunk_pivots
    for rows, cols in ((3, 5), (2000, 3000), (100000, 100000)):
        call, caps = _scripted([(OPT, 1)])
        lp.lists.solve_in_chunks(call, rows, cols, 0)
        call2, caps2 = _scripted([(False, np.array([OPT]), np.array([1]))])
        lp.lists.batch_in_chunks(call2, rows, cols, 0)
        assert caps == caps2 == [lp.simplex.chunk_pivots(rows, cols)]
    assert [lp.simplex.chunk_pivots(*s) for s in ((3, 5), (2000, 3000), (100000, 100000))] == [65536, 11453, 1024]


# ------------------------------------------------------------------ the loop by caps granted
def _answers(*rows, stop=()):
    """Per call (stop, statuses, pivots) from rows of (statuses, pivots)."""
    return [(q in stop, np.array(st, dtype=np.int32), np.array(npv, dtype=np.int64)) for q, (st, npv) in enumerate(rows)]


def test_batch_in_chunks_caps_by_the_caps_granted():
    script = _answers(([MAXP, MAXP], [1, 4]), ([MAXP, OPT], [0, 2]), ([MAXP, OPT], [2, 0]), ([OPT, OPT], [9, 9]))
    kept = [(a.copy(), b.copy()) for _, a, b in script]
    call, caps = _scripted(script)
    st, total = lp.lists.batch_in_chunks(call, 3, 5, 10, chunk=4)
    assert caps == [4, 4, 2]                                  # whatever the members report
    assert st.tolist() == [MAXP, OPT] and total.tolist() == [3, 6] and total.shape == (2,) and total.dtype == np.int64
    for (_, a, b), (a0, b0) in zip(script, kept):             # what the call handed out is as it was
        assert np.array_equal(a, a0) and np.array_equal(b, b0)
    assert total is not script[0][2]


def test_batch_in_chunks_ends_when_no_member_is_at_the_cap():
    call, caps = _scripted(_answers(([MAXP, OPT, UNB], [4, 1, 2]), ([INF, OPT, UNB], [3, 0, 0]), ([OPT] * 3, [9] * 3)))
    st, total = lp.lists.batch_in_chunks(call, 3, 5, 0, chunk=4)
    assert caps == [4, 4] and st.tolist() == [INF, OPT, UNB] and total.tolist() == [7, 1, 2]


def test_batch_in_chunks_sums_pairs():
    script = _answers(([MAXP, OPT], [[4, 0], [2, 1]]), ([OPT, OPT], [[1, 3], [0, 0]]))
    first = script[0][2].copy()
    call, caps = _scripted(script)
    st, total = lp.lists.batch_in_chunks(call, 3, 5, 0, chunk=4)
    assert total.shape == (2, 2) and total.tolist() == [[5, 3], [2, 1]] and st.tolist() == [OPT, OPT]
    assert np.array_equal(script[0][2], first)
    assert [lp.lists.member_pivots(total, q) for q in range(2)] == [(5, 3), (2, 1)]
    assert lp.lists.member_pivots(np.array([7, 8]), 1) == 8 and type(lp.lists.member_pivots(np.array([7, 8]), 1)) is int


def test_batch_in_chunks_stops_at_once_on_the_signal():
    call, caps = _scripted(_answers(([MAXP, MAXP], [4, 4]), ([MAXP, capi.MI_RUNNING], [1, 0]), ([OPT, OPT], [9, 9]), stop=(1,)))
    st, total = lp.lists.batch_in_chunks(call, 3, 5, 100, chunk=4)
    assert caps == [4, 4] and st.tolist() == [MAXP, capi.MI_RUNNING] and total.tolist() == [5, 4]


def test_only_the_exact_adapter_passes_a_cancelled_call_on():
    class Batch:
        n_lps, rows, cols = 2, 3, 5

        def __init__(self):
            self.caps = []

        def solve(self, is_max, max_pivots=0, **kw):
            self.caps.append(max_pivots)
            st, npv = np.array([MAXP, MAXP], dtype=np.int32), np.array([1, 1], dtype=np.int64)
            return (CANC, st, npv) if not kw else (st, npv)  # (the double batch has no call status to look at)
    xb = Batch()
    st, total = lp.exact.batch_in_chunks(xb, None, True, 10, 4)
    assert xb.caps == [4] and total.tolist() == [1, 1]
    mb = Batch()
    mb.rows = mb.cols = 100000                                # (chunk_pivots: 1024)
    st, total = lp.batch_lps.solve_batches(mb, None, True, max_pivots=2000)
    assert mb.caps == [1024, 976] and total.tolist() == [2, 2]


# ------------------------------------------------------------------ the grouping helpers
Tab = namedtuple("Tab", "matrix is_max")


def test_file_by_shape_keys_and_order():
    groups, groups2 = {}, {}
    a, b, c = Tab(np.zeros((3, 5)), True), Tab(np.zeros((3, 5)), False), Tab(np.zeros((3, 7)), False)
    for k, tabs in enumerate([a, [c, a], b, a, [c, b], [c, a], Tab(np.zeros((2, 5)), True)]):
        lp.lists.file_by_shape(groups, groups2, k, tabs)
    assert {key: [m[0] for m in v] for key, v in groups.items()} == \
        {((3, 5), True): [0, 3], ((3, 5), False): [2], ((2, 5), True): [6]}
    assert {key: [m[0] for m in v] for key, v in groups2.items()} == \
        {((3, 7), (3, 5), True): [1, 5], ((3, 7), (3, 5), False): [4]}
    assert groups[((3, 5), True)][1] == (3, a) and groups2[((3, 7), (3, 5), True)][0][1:] == (c, a)
    assert lp.lists.pop_singletons(groups) == [2, 6] and list(groups) == [((3, 5), True)]
    assert lp.lists.pop_singletons(groups2) == [4] and lp.lists.pop_singletons(groups2) == []


def test_group_by_rows_keys_order_and_singletons():
    Low = namedtuple("Low", "name is_max")
    host = {5: "float"}
    lowered = [(0, np.zeros((3, 3)), 0, 1, Low("a", True)), (1, np.zeros((3, 3)), np.int64(0), np.int64(1), Low("b", True)),
               (2, np.zeros((3, 3)), 1, 1, Low("c", True)), (3, np.zeros((3, 3)), 0, 1, Low("d", False)),
               (4, np.zeros((3, 4)), 0, 1, Low("e", True)), (6, np.zeros((3, 3)), 0, 1, Low("f", True))]
    groups = lp.lists.group_by_rows(lowered, host)
    assert list(groups) == [(2, 2, 0, 1, True)] and all(type(x) in (int, bool) for x in list(groups)[0])
    assert [(k, low.name) for k, low in groups[(2, 2, 0, 1, True)]] == [(0, "a"), (1, "b"), (6, "f")]
    assert host == {5: "float", 2: "alone", 3: "alone", 4: "alone"}


def test_row_counts_and_reasons_have_one_home():
    sense = np.array([[0, 1, 2, 0], [1, 1, 0, 2]], dtype=np.int32)
    flip = np.array([[True, True, True, False], [False, True, False, False]])
    n_eq, n_art = lp.lists.row_counts(flip, sense)
    # member 0: `<=` flipped -> `>=` (artificial), `>=` flipped -> `<=`, `=`, `<=`; member 1: `>=`, `>=` flipped, `<=`, `=`
    assert (n_eq.tolist(), n_art.tolist()) == ([1, 1], [2, 2])
    L = np.zeros((2, 5, 3))
    L[:, :4, -1] = np.where(flip, -1.0, 1.0)
    assert [x.tolist() for x in lp.batch_lps.row_counts(L, sense)] == [[1, 1], [2, 2], [3, 1]]
    assert [x.tolist() for x in lp.exact_lps.row_counts(L.astype(np.int64), sense)] == [[1, 1], [2, 2]]
    assert lp.batch_lps.SENSES is lp.exact_lps.SENSES is lp.lists.SENSES
    p = _le(0)
    assert lp.lists.rows_reason(p) is None and lp.batch_lps.host_reason(p) is None and lp.exact_lps.host_reason(p) is None
    assert lp.lists.rows_reason(_unbounded()) == "no constraints"
    odd = lp.Problem(type="max", vars=["x"], objective_func=[("x", 1)], constraints=[("<", [("x", 1)], 1)])
    assert lp.lists.rows_reason(odd) == lp.batch_lps.host_reason(odd) == lp.exact_lps.host_reason(odd) == "constraint"
    assert lp.batch_lps.host_reason(_integer(0)) == lp.exact_lps.host_reason(_integer(0)) == "integer variables"
    assert lp.batch_lps.host_reason(_float(0)) is None and lp.exact_lps.host_reason(_float(0)) == "float"


def test_placement_and_the_tail():
    results = [None] * 5
    lp.lists.place(results, [3, 1], ["c", "a"])
    tried = []

    def solve(k):
        tried.append(k)
        if k == 2:
            raise lp.InfeasibleProblemError()
        if k == 0:
            raise lp.UnboundedProblemError()
        return "s%d" % k
    lp.lists.one_by_one(results, [4, 2, 0], solve)
    assert tried == [4, 2, 0] and results[1::2] == ["a", "c"] and results[4] == "s4"
    assert isinstance(results[0], lp.UnboundedProblemError) and isinstance(results[2], lp.InfeasibleProblemError)
    assert lp.lists.finish(results, False) is results
    with pytest.raises(lp.UnboundedProblemError):             # the lowest index, not the first attempted
        lp.lists.finish(results, True)
    with pytest.raises(KeyError):                             # only the reference's conditions take a slot
        lp.lists.one_by_one(results, [1], {}.__getitem__)


# ------------------------------------------------------------------ routing: a mixed list through the five routes
def _problem(k, rows, kind="max", integer=(), c=1):
    """max / min c x + 2 y over x, y >= 0; the first row's right-hand side, 100 + k, tells the member's index."""
    cons = [("<=", [("x", 1), ("y", 1)], 100 + k)] + rows
    return lp.Problem(type=kind, vars=["x", "y"], objective_var="w", objective_func=[("x", c), ("y", 2)],
                      constraints=cons, integer_vars=list(integer))


def _le(k, m=2, kind="max"):
    return _problem(k, [("<=", [("x", 1 + i), ("y", 1)], 7 + i) for i in range(m - 1)], kind)


def _ge(k):
    return _problem(k, [(">=", [("x", 1)], 1)])              # an artificial row: two phases


def _negated(k):
    return _problem(k, [(">=", [("x", 1), ("y", -1)], -5)])  # negated into a `<=` row: single phase, no unit basis


def _integer(k):
    return _problem(k, [("<=", [("x", 2), ("y", 1)], 7)], integer=["x"])


def _float(k):
    return _problem(k, [("<=", [("x", 2), ("y", 1)], 7)], c=0.5)


def _unbounded():
    return lp.Problem(type="max", vars=["x"], objective_var="w", objective_func=[("x", 1)])


def _mixed():
    return [_le(0), _ge(1), _integer(2), _le(3), _le(4, m=3), _ge(5), _negated(6), _le(7), _ge(8), _unbounded(),
            _float(10), _le(11, kind="min"), _le(12, m=4), _le(13, m=4)]


FINAL = {1: INF, 7: UNB}        # the scripted end of members 1 and 7 wherever a batch solves them
SLOW = 3                        # at MI_MAX_PIVOTS after its batch's first call


class Script:
    """What the stand-ins of one run are told and what they saw."""

    def __init__(self, problems, final=FINAL, declined_rows=None, overflow=()):
        self.problems, self.final, self.declined_rows, self.overflow = problems, final, declined_rows, overflow
        self.log, self.caps, self.made = [], [], []

    def solver(self, problem, **kw):
        """mi355x_simplex_solver / solve_single: declines an integer problem, as they do."""
        k = next(k for k, p in enumerate(self.problems) if p is problem)
        self.log.append(("alone", k))
        if problem.integer_vars:
            raise lp.UnsupportedConstraintError(("integer",) + tuple(problem.integer_vars), "mi355x-simplex")
        return ("alone", k)

    def create(self, cls, what, tags, rows, cols, decline=None):
        """A batch of members `tags`; the shapes of declined_rows rows raise the route's decline."""
        self.log.append((what, list(tags)))
        if rows == self.declined_rows:
            raise decline
        self.made.append(cls(self, list(tags), rows, cols))
        return self.made[-1]


class Fake:
    """A batch: statuses and pivots from the script (every call: 2 pivots per member, or (2, 1)), tableaux of zeros."""

    def __init__(self, script, tags, rows, cols):
        self.s, self.tags, self.n_lps, self.rows, self.cols, self.calls, self.closed = script, tags, len(tags), rows, cols, 0, 0

    def _answer(self, cap, pair, hide=()):
        self.calls += 1
        self.s.caps.append((self.rows, self.cols, cap))
        st = [MAXP if k == SLOW and self.calls == 1 else capi.MI_EXACT_OVERFLOW if k in self.s.overflow else
              self.s.final.get(k, OPT) for k in self.tags]
        st = [OPT if x in hide else x for x in st]
        return np.array(st, dtype=np.int32), np.array([[2, 1] if pair else 2] * self.n_lps, dtype=np.int64)

    def download(self, q):
        return np.zeros((self.rows, self.cols), dtype=self.dtype), np.arange(self.rows - 1, dtype=np.int64)

    def close(self):
        self.closed += 1


class FakeMB(Fake):
    """MultiDeviceBatch: a phase ends optimal for a member without a feasible point; the hand-over finds that out."""
    dtype = np.float64

    def solve(self, is_max=True, fp_tolerance=1024, max_pivots=0):
        return self._answer(max_pivots, False, hide=(INF,))

    def two_phase_handover(self, main, fp_tolerance=1024, phase1_status=None):
        assert phase1_status.tolist() == [OPT] * self.n_lps and main.tags == self.tags
        self.s.log.append(("handover", self.tags))
        return (np.array([self.s.final.get(k, capi.MI_OK) for k in self.tags], dtype=np.int32),
                np.ones(self.n_lps, dtype=np.int64))


class FakeSB(Fake):
    dtype = np.float32

    def solve(self, is_max, fp_tolerance=1024, max_pivots=0):
        return self._answer(max_pivots, False)

    def solve_two_phase(self, main, main_is_max, fp_tolerance=1024, max_pivots=0):
        assert main.tags == self.tags
        return self._answer(max_pivots, True)


class FakeXB(Fake):
    def solve(self, is_max, max_pivots=0):
        return (capi.MI_OK,) + self._answer(max_pivots, False)

    def solve_two_phase(self, main, main_is_max, max_pivots=0):
        assert main.tags == self.tags
        return (capi.MI_OK,) + self._answer(max_pivots, True)


def _tags(matrices):
    return [int(M[0][-1]) - 100 for M in matrices]


def _no_device(monkeypatch, cls):
    monkeypatch.setattr(cls, "_h", property(lambda self: pytest.fail("a device handle was asked for")))


def _stub_double(monkeypatch, s):
    def from_arrays(cls, matrices, bases, n_devices, device_ids=None):
        assert bases.shape == (len(matrices), matrices.shape[1] - 1)
        return s.create(FakeMB, "batch", _tags(matrices), *matrices.shape[1:])

    def from_lps(cls, lps, sense, n_devices, device_ids=None):
        n_eq, n_art, _ = (int(x) for x in lp.batch_lps.row_counts(lps[0], sense[0]))
        rows, cols = lps.shape[1], lps.shape[2] - 1 + sense.shape[1] - n_eq + 1
        main = s.create(FakeMB, "rows", _tags(lps), rows, cols)
        return main, (FakeMB(s, main.tags, rows, cols + n_art) if n_art else None)
    monkeypatch.setattr(lp.batch.MultiDeviceBatch, "from_arrays", classmethod(from_arrays))
    monkeypatch.setattr(lp.batch.MultiDeviceBatch, "from_lps", classmethod(from_lps))
    monkeypatch.setattr(lp.simplex, "mi355x_simplex_solver", s.solver)
    _no_device(monkeypatch, lp.simplex.Tableau)


def _stub_exact(monkeypatch, s):
    def xbatch(tabs, device=0, min_bits=0, pivot_rule="dantzig"):
        rows, cols = tabs[0].matrix.shape
        return s.create(FakeXB, "batch", _tags(t.matrix for t in tabs), rows, cols,
                        lp.exact._declined(("batch", "shape", rows, cols)))

    def create_lps(num, den, sense, device=0, min_bits=0, pivot_rule="dantzig"):
        n_eq, n_art = (int(x) for x in lp.exact_lps.row_counts(num[0], sense[0]))
        rows, cols = num.shape[1], num.shape[2] - 1 + sense.shape[1] - n_eq + 1
        assert (den == 1).all()
        main = s.create(FakeXB, "rows", _tags(num), rows, cols, lp.exact._declined(("batch", "shape", rows, cols + n_art)))
        return main, (FakeXB(s, main.tags, rows, cols + n_art) if n_art else None)
    monkeypatch.setattr(lp.exact, "XBatch", xbatch)
    monkeypatch.setattr(lp.exact_lps, "create_lps", create_lps)
    monkeypatch.setattr(lp.simplex, "mi355x_simplex_solver", s.solver)
    _no_device(monkeypatch, lp.exact.ExactTableau)


def _stub_single(monkeypatch, s):
    def from_arrays(cls, matrices, basis, device=0):
        assert matrices.dtype == np.float32 and basis.shape == (len(matrices), matrices.shape[1] - 1)
        declined = capi.Mi355xError.__new__(capi.Mi355xError)          # (its __init__ asks the library for a message)
        declined.code = capi.MI_UNSUPPORTED
        return s.create(FakeSB, "batch", _tags(matrices), *matrices.shape[1:], declined)
    monkeypatch.setattr(lp.single.SingleBatch, "from_arrays", classmethod(from_arrays))
    monkeypatch.setattr(lp.single, "solve_single", s.solver)
    _no_device(monkeypatch, lp.single.SingleTableau)


A, B, D = [0, 3, 7, 10], [1, 5, 8], [12, 13]          # 3 x 5 max; two-phase; 5 x 7 max (4 and 11 are alone in their groups)
ROUTES = {
    # members 2 (integer) and 6 (no unit basis) go alone as the list is read; a group of one when it is reached
    "default": (dict(), _stub_double,
                [("alone", 2), ("alone", 6), ("batch", A), ("alone", 4), ("alone", 11), ("batch", D), ("batch", B),
                 ("batch", B), ("handover", B)]),
    # the groups first, then what group_lowered_rows leaves to the default route, in list order (9: build-tableau's own
    # condition, no call)
    "from_rows": (dict(from_rows=True), _stub_double,
                  [("rows", A), ("rows", B), ("handover", B), ("rows", D), ("alone", 2), ("alone", 4), ("alone", 6),
                   ("alone", 11)]),
    # 2, 10 (a float) and the groups of one first, in list order; 6 is a member of its shape's group; 5 x 7 is declined
    "exact": (dict(exact=True), _stub_exact,
              [("alone", 2), ("alone", 4), ("alone", 10), ("alone", 11), ("batch", [0, 3, 6, 7]), ("batch", D), ("alone", 12),
               ("alone", 13), ("batch", B), ("batch", B)]),
    # the groups of rows first; the rest -- and the declined group -- is the exact route's list
    "device_build": (dict(exact=True, device_build=True), _stub_exact,
                     [("rows", [0, 3, 6, 7]), ("rows", B), ("rows", D), ("alone", 2), ("alone", 4), ("alone", 10),
                      ("alone", 11), ("batch", D), ("alone", 12), ("alone", 13)]),
    # 2 first, then group by group: no unit-basis rule, a float is a member like any other
    "single": (dict(precision="single"), _stub_single,
               [("alone", 2), ("batch", [0, 3, 6, 7, 10]), ("alone", 4), ("alone", 11), ("batch", D), ("alone", 12),
                ("alone", 13), ("batch", B), ("batch", B)]),
}
DECLINES = {"default": None, "from_rows": None, "exact": 5, "device_build": 5, "single": 5}
TABLEAU = {"default": "Tableau", "from_rows": "Tableau", "exact": "ExactTableau", "device_build": "ExactTableau",
           "single": "SingleTableau"}


@pytest.fixture(params=list(ROUTES))
def route(request, monkeypatch):
    kw, stub, log = ROUTES[request.param]
    s = Script(_mixed(), declined_rows=DECLINES[request.param])
    stub(monkeypatch, s)
    return request.param, kw, s, log


def test_every_route_sends_each_member_where_it_belongs(route):
    name, kw, s, log = route
    ps = s.problems
    out = lp.solve_problems(ps, errorp=False, **kw)
    if DECLINES[name] is None:                                # (the double batch takes the 5 x 7 members)
        log = [e for e in log if e[0] != "alone" or e[1] not in D]
    assert s.log == log
    in_batches = sorted(k for what, ks in log if what != "alone" and what != "handover" for k in ks
                        if DECLINES[name] is None or k not in D)
    one_by_one = [k for what, k in log if what == "alone"]
    assert sorted(set(in_batches) | set(one_by_one) | {9}) == list(range(len(ps))) and not set(in_batches) & set(one_by_one)
    # every result in its own slot
    for k in one_by_one:
        if k != 2:
            assert out[k] == ("alone", k)
    assert isinstance(out[2], lp.UnsupportedConstraintError) and out[2].args == (("integer", "x"), "mi355x-simplex")
    assert type(out[9]) is lp.UnboundedProblemError          # (build-tableau's own condition: no solver was asked)
    assert type(out[1]) is lp.InfeasibleProblemError and type(out[7]) is lp.UnboundedProblemError
    two_phase = (3, 2) if name in ("default", "from_rows") else (2, 1)     # (2 + the hand-over's 1, 2) or one call's (2, 1)
    for k in set(in_batches) - {1, 7}:
        t = out[k]
        assert type(t).__name__ == TABLEAU[name] and t.problem is ps[k], k
        assert t.n_pivots == (two_phase if k in B else 4 if k in A + [6] else 2), k     # (member 3 took its batch two calls)
        assert type(t.n_pivots) is (tuple if k in B else int)
        if k in B:
            assert [type(x) for x in t.n_pivots] == [int, int]
    # every call got chunk_pivots of its (first) batch's shape
    assert s.caps and all(cap == lp.simplex.chunk_pivots(rows, cols) == 65536 for rows, cols, cap in s.caps)
    if name == "single":                                      # (the route closes what it made)
        assert [b.closed for b in s.made] == [1] * len(s.made)


def test_errorp_raises_the_lowest_index_after_every_member_was_attempted(route):
    name, kw, s, log = route
    lp.solve_problems(s.problems, errorp=False, **kw)
    quiet = list(s.log)
    del s.log[:]
    with pytest.raises(lp.InfeasibleProblemError):           # member 1's, though 2's (and elsewhere 7's) came first
        lp.solve_problems(s.problems, errorp=True, **kw)
    assert s.log == quiet


def test_max_pivots_reaches_every_batch_call(route):
    name, kw, s, log = route
    out = lp.solve_problems(s.problems, errorp=False, max_pivots=3, **kw)
    assert s.caps and all(cap == 3 for _, _, cap in s.caps)
    # one call uses the caps up: member 3 is left at MI_MAX_PIVOTS
    assert type(out[3]) is lp.SolverError and out[3].args == ("pivot cap reached",)
    assert out[0].n_pivots == 2


def test_device_build_hands_a_member_past_128_bits_to_the_host_built_route(monkeypatch):
    s = Script(_mixed(), overflow=(3,), declined_rows=5)
    _stub_exact(monkeypatch, s)
    out = lp.solve_problems(s.problems, exact=True, device_build=True, errorp=False)
    assert s.log[:3] == [("rows", [0, 3, 6, 7]), ("rows", B), ("rows", D)]
    assert s.log[3:] == [("alone", k) for k in (2, 3, 4, 10, 11)] + [("batch", D), ("alone", 12), ("alone", 13)]
    assert out[3] == ("alone", 3) and out[0].n_pivots == 4 and out[0].problem is s.problems[0]
