"""build-tableau (src/simplex.lisp:142-328) on the host, written once for every precision.

Two stages.  ``lower`` is the part that needs the problem's names (:189-241, :270-283): var-mappings, the bound
rows put in front of the constraints, and per constraint one row in column space -- the structural
coefficients and the right-hand side less the offsets -- then the objective row with its signs and constant.
``assemble`` is the rest (:214-221, :243-328): the dense matrix and basis, the flip of a row with a negative
right-hand side, slack columns, and the artificial twin with its objective row.  ``bounds_only`` is the branch
for a problem without constraints (:153-186), and ``build`` composes the three.

The device-built batches stop after ``lower`` (batch_lps.lower_problem_rows, exact_lps.lower_problem) and do
``assemble``'s work in kernels; simplex.build_tableau and single.build_tableau_single run both stages.  So
what a device-built batch starts from and what build_tableau produces come from the same statements.

A ``NumberSystem`` says what a number is.  The bodies below use plain Python operators on what ``read``
returns: Python floats for DOUBLE, ints and Fractions for EXACT, and for single.SINGLE a value class whose
operators are Lisp's int / single-float contagion.
"""
from fractions import Fraction

import numpy as np

from .conditions import ParsingError, UnboundedProblemError
from .problem import Problem


def _same(x):
    return x


class NumberSystem:
    """read(x): a number of the problem as the build computes with it; zeros(shape): an empty matrix;
    matrix(M) / mapping(d): a finished matrix / var-mapping as it is handed out (the identity unless the
    build computes with other objects than the ones it hands out).  For the read-back
    (simplex.tableau_variable): value(x) is an entry as it is returned, offset(x) a mapping's offset as it is
    added to one."""

    def __init__(self, read, zeros, value, offset=_same, matrix=_same, mapping=_same):
        self.read, self.zeros, self.value, self.offset = read, zeros, value, offset
        self.matrix, self.mapping = matrix, mapping
        self.zero, self.one = read(0), read(1)


def _object_zeros(shape):
    return np.full(shape, 0, dtype=object)


def _rational(x):
    return x if type(x) is int or type(x) is Fraction else Fraction(x)


def _fraction(x):
    return x if type(x) is Fraction else Fraction(x)


DOUBLE = NumberSystem(float, np.zeros, float)
#: rationals the way Lisp holds them: an integer stays a Python int (the same exact arithmetic at a fraction of
#: the cost), anything else is a Fraction; what is handed out is Fractions only -- ExactTableau makes every
#: entry of its matrix one, mapping does so for the offsets
EXACT = NumberSystem(_rational, _object_zeros, Fraction,
                     mapping=lambda d: {var: mp[:2] + tuple(_fraction(x) for x in mp[2:]) for var, mp in d.items()})

FLIPPED = {"<=": ">=", ">=": "<=", "=": "="}


def lower(problem, ns, instance_problem=None, stored=None, room=False):
    """Steps :189-241 and :270-283 -> (L, ncv, constraints, mapping): L (m + 1) x (ncv + 1) in the number
    system's matrix type, constraints the m (op, expr, rhs) its rows were made from (bound rows first), mapping
    the var-mapping with its offsets as read.  A later term of a variable in one expression replaces the
    coefficient; its offset product is still subtracted.  Raises ParsingError for an unknown operator once
    that row's terms are done.  stored(x), when given, sees every coefficient as it is stored and every
    finished right-hand side and the objective's constant (exact_lps: the 64-bit check).  room=True puts one zero
    column per slack variable in front of L's last, so that assemble can finish L itself (in_place)."""
    read = ns.read
    constraints = [(op, list(expr), rhs) for op, expr, rhs in (instance_problem or problem).constraints]
    bounds = dict(problem.var_bounds)
    mappings, column = {}, 0
    for var in problem.vars:                                              # :189-212
        if var not in bounds:
            mappings[var] = ("positive", column, ns.zero)
        else:
            lb, ub = bounds[var]
            if lb is not None and ub is not None:
                if 0 <= ub:
                    constraints.insert(0, ("<=", [(var, 1)], ub))
                else:
                    constraints.insert(0, (">=", [(var, 1)], -ub))
                mappings[var] = ("positive", column, read(lb))
            elif lb is not None:
                mappings[var] = ("positive", column, read(lb))
            elif ub is not None:
                mappings[var] = ("negative", column, read(ub))
            else:
                mappings[var] = ("signed", column)
                column += 1
        column += 1
    ncv, m = column, len(constraints)
    last = ncv + sum(1 for c in constraints if c[0] != "=") if room else ncv
    L = ns.zeros((m + 1, last + 1))
    for (op, expr, rhs), out in zip(constraints, L):                      # :223-241
        acc = read(rhs)
        for var, coef in expr:
            mp, c = mappings[var], read(coef)
            if mp[0] == "positive":
                out[mp[1]] = a = c
                acc = acc - c * mp[2]
            elif mp[0] == "negative":
                out[mp[1]] = a = -c
                acc = acc - c * mp[2]
            else:
                out[mp[1]] = a = c
                out[mp[1] + 1] = -c
            if stored is not None:
                stored(a)
        out[last] = acc
        if stored is not None:
            stored(acc)
        if op not in FLIPPED:
            raise ParsingError("%r is not a valid constraint equation" % ((op, expr, rhs),))
    out, acc = L[m], ns.zero
    for var, coef in problem.objective_func:                              # :270-283
        mp, c = mappings[var], read(coef)
        if mp[0] == "positive":
            out[mp[1]] = a = -c
            acc = acc + c * mp[2]
        elif mp[0] == "negative":
            out[mp[1]] = a = c
            acc = acc + c * mp[2]
        else:
            out[mp[1]] = a = -c
            out[mp[1] + 1] = c
        if stored is not None:
            stored(a)
    out[last] = acc
    if stored is not None:
        stored(acc)
    return L, ncv, constraints, mappings


def assemble(L, ncv, constraints, ns, in_place=False, general=False):
    """Steps :214-221 and :243-328 on lower's rows -> (main matrix, main basis, artificial matrix, artificial
    basis), the last two None when no row needs an artificial variable or with general=True (the general form:
    the basis entry of such a row is the number of columns).  in_place: L was lowered with room=True and
    becomes the main matrix."""
    ops = [c[0] for c in constraints]
    m = len(ops)
    if in_place:
        M, num_cols = L, L.shape[1]
    else:
        num_cols = ncv + sum(1 for op in ops if op != "=") + 1
        M = ns.zeros((m + 1, num_cols))
        M[:, :ncv], M[:, -1] = L[:, :ncv], L[:, -1]
    basis = np.zeros(m, dtype=np.int64)
    art_rows = []
    slack = ncv
    for row, op in enumerate(ops):
        if M[row, -1] < 0:                                                # :243-252: the whole row, zeros included
            M[row, :] = -M[row, :]
            op = FLIPPED[op]
        if op == "<=":                                                    # :254-265
            M[row, slack] = ns.one
            basis[row] = slack
        else:
            art_rows.insert(0, row)
            basis[row] = num_cols
            if op == ">=":
                M[row, slack] = -ns.one
        slack += op != "="
    if not art_rows or general:
        return M, basis, None, None
    nac = num_cols + len(art_rows)                                        # :292-325
    A = ns.zeros((m + 1, nac))
    A[:m, :num_cols - 1], A[:m, -1] = M[:m, :num_cols - 1], M[:m, -1]
    objective = A[m]
    for row in reversed(art_rows):                                        # increasing rows, from zero: the order
        objective += A[row]                                               # of the reference's sum, column by column
    abasis = basis.copy()
    for i, row in enumerate(art_rows):                                    # (after the sum: it leaves their columns 0)
        abasis[row] = num_cols - 1 + i
        A[row, num_cols - 1 + i] = ns.one
    return M, basis, A, abasis


def bounds_only(problem, ns):
    """The problem without constraints (:153-186): every variable at the bound its objective coefficient pulls
    it to -> (matrix, basis, mapping); unbounded-problem-error at the first variable without that bound."""
    pvars = list(problem.vars)
    n = len(pvars)
    bounds = dict(problem.var_bounds)
    objd = dict(problem.objective_func)
    is_max = problem.type == "max"
    M = ns.zeros((n + 1, n + 1))
    mappings = {}
    objective_value = ns.zero
    for i, var in enumerate(pvars):
        coef = objd[var]
        lb, ub = bounds.get(var, (None, None))
        M[i, i] = ns.one
        bound = ub if (0 <= coef) == is_max else lb
        if bound is None:
            raise UnboundedProblemError()
        mappings[var] = ("positive", i, ns.read(bound))
        objective_value = objective_value + ns.read(coef) * mappings[var][2]
    M[n, n] = objective_value
    return M, np.arange(n, dtype=np.int64), mappings


def build(problem, instance_problem, ns, make, general=False):
    """build-tableau: make(instance problem, matrix, basis, var-mapping) -> a tableau; returns one, or
    [artificial, main] when the trivial basis is infeasible.  general=True: the main tableau of the general
    form only, also for a problem without constraints."""
    if not instance_problem.constraints and not general:
        M, basis, mapping = bounds_only(problem, ns)
        return make(problem, ns.matrix(M), basis, ns.mapping(mapping))
    L, ncv, constraints, mapping = lower(problem, ns, instance_problem, room=True)
    M, basis, A, abasis = assemble(L, ncv, constraints, ns, True, general)
    mapping = ns.mapping(mapping)
    main = make(instance_problem, ns.matrix(M), basis, mapping)
    if A is None:
        return main
    art_problem = Problem(type="min", vars=list(problem.vars))            # artificial problem
    return [make(art_problem, ns.matrix(A), abasis, mapping), main]
