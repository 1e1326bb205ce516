"""The pivot rules of the exact solves, without a GPU: the test-side restatement (tests/pivot_rule_cases.py)
on the inputs the GPU tests run -- what each rule does on the textbook cycling LPs, that the inputs tell the
rules (and a wrong tie key) apart, the argument errors of the public functions, and the new symbols in the
header, in capi.py and in the glue.  Every solve carries a finite cap."""
import os
import re
from fractions import Fraction

import pytest

import oracle.rational_ref as rr
from tests import exact_cases as ec
from tests import pivot_rule_cases as pc
from tests.helpers import ROOT, lp_amd

lp = lp_amd()


@pytest.mark.parametrize("name", sorted(pc.CYCLING))
def test_the_default_rule_cycles_and_the_other_two_end(name):
    make, want, optimum = pc.CYCLING[name]
    tabs = rr.build_tableau(ec.to_dict(make(lp)))
    assert not isinstance(tabs, tuple)
    st, trace, _, _ = pc.solve_tabs(tabs, "dantzig", 60)
    assert st == "max_pivots" and trace == pc.PERIOD * 10
    # the Fraction oracle itself repeats the period
    t = rr.build_tableau(ec.to_dict(make(lp)))
    seen = []
    for _ in range(12):
        e = rr.price(t)
        seen.append((e, rr.ratio(t, e)))
        rr.pivot(t, *seen[-1])
    assert seen == pc.PERIOD * 2
    for rule in ("bland", "dantzig-bland"):
        st, trace, m, stats = pc.solve_tabs(tabs, rule, 200)
        assert st == "optimal" and trace == want and not stats["inexact"]
        assert m.matrix()[-1][-1] == optimum


def test_model_and_vecmodel_agree_under_every_rule():
    T, b = pc.slack(**pc.WIDE_SLACK)
    for rule in pc.RULES + ("row-key",):
        st, trace, m = pc.solve_state(T, b, rule, 3000)
        slow = pc.MODELS[rule].from_state(T.tolist(), 1, b.tolist(), T.shape[1] - 1)
        strace = []
        assert slow.solve(True, strace, 3000) == st and strace == trace
        assert slow.T == m.T.tolist() and slow.D == m.D and slow.basis == m.basis


def test_the_wide_slack_shape_tells_the_rules_and_the_tie_key_apart():
    T, b = pc.slack(**pc.WIDE_SLACK)
    assert T.shape == (41, 341)
    got = {rule: pc.solve_state(T, b, rule, 3000) for rule in pc.RULES + ("row-key",)}
    assert all(st == "optimal" for st, _, _ in got.values())
    traces = [tuple(tr) for _, tr, _ in got.values()]
    assert len(set(traces)) == 4                                      # pairwise different
    assert [len(got[r][1]) for r in pc.RULES] == [44, 106, 107]
    assert pc.degenerate_count(T, b, got["dantzig"][1]) == 43
    for _, _, m in got.values():
        assert Fraction(int(m.T[-1, -1]), m.D) == Fraction(1, 2) and not m.stats["inexact"] and m.stats["max_bits"] <= 64


def test_the_tall_slack_shape_tells_the_tie_key_apart():
    T, b = pc.slack(**pc.TALL_SLACK)
    assert T.shape == (301, 341)
    bland, keyed, dantzig = (pc.solve_state(T, b, r, 3000) for r in ("bland", "row-key", "dantzig"))
    assert bland[0] == keyed[0] == dantzig[0] == "optimal"
    assert bland[1] != keyed[1] and bland[1] != dantzig[1]
    assert bland[2].stats["max_bits"] <= 64


def test_the_two_phase_case_tells_the_rules_apart():
    tabs = rr.build_tableau(ec.to_dict(ec.mixed_problem(lp, 6, 3, 2, 1, seed=7)))
    assert isinstance(tabs, tuple)
    traces = []
    for rule in pc.RULES:
        st, trace, m, stats = pc.solve_tabs(tabs, rule, 200)
        assert st == "optimal" and stats["driveouts"] == 2 and not stats["inexact"]
        assert m.matrix()[-1][-1] == Fraction(158, 9)
        traces.append(tuple(trace))
    assert len(set(traces)) == 3
    # rule 0 through the model is the Fraction oracle's trace
    assert list(traces[0]) == ec.oracle_outcome(tabs)[1]


@pytest.mark.parametrize("seed", [24, 26])
def test_two_phase_cases_where_a_flag_kept_over_the_hand_over_would_show(seed):
    """Under rule 2 phase 1 ends on a degenerate pivot, and Bland's choice on the handed-over tableau is not the
    default rule's: a main tableau that inherited the flag would start phase 2 with another pivot."""
    tabs = rr.build_tableau(ec.to_dict(ec.mixed_problem(lp, 6, 3, 2, 1, seed=seed)))
    keep = {}
    st, trace, mm, stats = pc.solve_tabs(tabs, "dantzig-bland", 200, keep=keep)
    assert st == "optimal" and stats["driveouts"] == 2 and len(trace) > keep["n1"]
    a = pc.DantzigBlandModel(tabs[0].matrix, tabs[0].basis, tabs[0].var_count)
    for e, r in trace[:keep["n1"]]:
        last = a.T[r][a.nv] == 0
        a.pivot(e, r)
    assert last
    T, D, basis = pc.handover_start(tabs, "dantzig-bland")
    stale = pc.BlandModel.from_state(T, D, basis, mm.nv)
    e = stale.price(True)
    assert (e, stale.ratio(e)) != trace[keep["n1"]]


def test_the_restart_case_overflows_64_bits_on_a_degenerate_pivot():
    T, b = pc.restart_state()
    st, trace, m = pc.solve_state(T, b, "dantzig-bland", pc.RESTART_CAP)
    deg = pc.degenerate_flags(T, b, trace)
    stage, at = m.stats["over64"]
    assert st == "max_pivots" and 64 < m.stats["max_bits"] <= 128 and not m.stats["inexact"]
    assert at >= 1 and deg[at - 1] and deg[at]            # the flag stands when the replay starts; cleared, or the
    first = pc.BlandVec.from_state(T, 1, b, T.shape[1] - 1)          # first pivot would be Bland's, another one
    e = first.price(True)
    assert (e, first.ratio(e)) != trace[0]
    assert trace != pc.solve_state(T, b, "dantzig", pc.RESTART_CAP)[1]


# ---- the public functions' argument errors (raised before anything touches a device) -----------------------
def _float_beale():
    p = ec.beale(lp)
    return lp.Problem(type=p.type, vars=p.vars, objective_var=p.objective_var,
                      objective_func=[(v, float(c)) for v, c in p.objective_func],
                      constraints=[(op, [(v, float(c)) for v, c in e], float(rhs)) for op, e, rhs in p.constraints])


def test_argument_errors_of_the_public_functions():
    p = ec.beale(lp)
    with pytest.raises(ValueError, match="pivot_rule"):
        lp.solve_problem(p, exact=True, pivot_rule="steepest", max_pivots=200)
    with pytest.raises(ValueError, match="exact=True"):
        lp.solve_problem(p, pivot_rule="bland", max_pivots=200)
    with pytest.raises(ValueError, match="pivot_rule"):
        lp.solve_problems([p, p], exact=True, pivot_rule=1, max_pivots=200)
    with pytest.raises(ValueError, match="exact=True"):
        lp.solve_problems([p, p], pivot_rule="dantzig-bland", max_pivots=200)
    with pytest.raises(lp.UnsupportedConstraintError) as e:
        lp.solve_problem(_float_beale(), exact=True, pivot_rule="bland", max_pivots=200)
    assert tuple(e.value.constraint) == ("exact", "pivot-rule", "bland")
    with pytest.raises(ValueError):
        lp.exact.XBatch.from_states(None, None, None, pivot_rule="nope")
    with pytest.raises(ValueError):
        lp.exact.ExactTableau(p, p, [[Fraction(0)]], [], 0, 0, {}, pivot_rule="nope")
    xbb = __import__("importlib").import_module("linear-programming_amd.exact_bb")
    with pytest.raises(ValueError):
        xbb.DeviceRounds(p, pivot_rule="nope")
    assert lp.exact.pivot_rule_code("dantzig-bland") == lp.capi.MI_RULE_DANTZIG_BLAND == 2
    assert lp.exact.ExactTableau(p, p, [[Fraction(0)]], [], 0, 0, {}).pivot_rule == "dantzig"


def test_the_new_symbols_in_the_header_the_bindings_and_the_glue():
    header = open(os.path.join(ROOT, "include", "mi355x_simplex.h")).read()
    assert re.search(r"enum\s*\{\s*MI_RULE_DANTZIG = 0, MI_RULE_BLAND = 1, MI_RULE_DANTZIG_BLAND = 2\s*\}", header)
    for name, arg in (("mi355x_xtab_set_pivot_rule", "mi355x_xtab *t"), ("mi355x_xbatch_set_pivot_rule", "mi355x_xbatch *b")):
        at = header.index("int  %s(%s, int rule);" % (name, arg))
        comment = header[header.rindex("/*", 0, at):at]
        assert "find-entering-column" in comment and "find-pivoting-row" in comment     # what the choice replaces
        assert lp.capi.SIGNATURES[name][1] == [lp.capi.ctypes.c_void_p, lp.capi.ctypes.c_int]
        assert hasattr(lp.capi.lib(), name)
        assert getattr(lp.capi.lib(), name)(None, 0) == lp.capi.MI_BAD_ARG
    assert lp.capi.lib().mi355x_abi_version() == 1
    glue = open(os.path.join(ROOT, "linear-programming_amd", "lisp", "mi355x-simplex.lisp")).read()
    assert '(cffi:defcfun ("mi355x_xtab_set_pivot_rule" %xtab-set-pivot-rule) :int (tab :pointer) (rule :int))' in glue
    assert '(cffi:defcfun ("mi355x_xbatch_set_pivot_rule" %xbatch-set-pivot-rule) :int (batch :pointer) (rule :int))' in glue
    assert glue.count("(pivot-rule :dantzig)") == 2
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert ":pivot-rule" in open(os.path.join(ROOT, doc)).read(), doc
