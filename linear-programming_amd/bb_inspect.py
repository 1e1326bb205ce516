"""Inspection and control of a running branch-and-bound job (native.BranchAndBound) from outside
the glue's call sequence: mi355x_simplex_solver_bb_cancel (any thread), _bb_stats and _bb_trace.
native.py keeps to the calls the Lisp glue's native route makes; these are what tests and tools use
on top of them."""
import ctypes

import numpy as np

from . import capi


def cancel(bb):
    capi.check(capi.lib().mi355x_simplex_solver_bb_cancel(bb._h), "mi355x_simplex_solver_bb_cancel")


def stats(bb):
    a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    capi.check(capi.lib().mi355x_simplex_solver_bb_stats(bb._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
               "mi355x_simplex_solver_bb_stats")
    return {"processed": a.value, "solved": b.value, "max_depth": c.value}


def trace(bb):
    """[(parent, var name or None, sense, bound, outcome, objective)] of the processed nodes."""
    L, n = capi.lib(), ctypes.c_int64(0)
    capi.check(L.mi355x_simplex_solver_bb_trace(bb._h, None, None, None, None, None, None, 0, ctypes.byref(n)),
               "mi355x_simplex_solver_bb_trace")
    k = n.value
    par, var = np.empty(k, np.int64), np.empty(k, np.int64)
    sen, out = np.empty(k, np.int32), np.empty(k, np.int32)
    bnd, obj = np.empty(k), np.empty(k)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    capi.check(L.mi355x_simplex_solver_bb_trace(bb._h, ptr(par), ptr(var), ptr(sen), ptr(bnd), ptr(out), ptr(obj),
                                                k, ctypes.byref(n)), "mi355x_simplex_solver_bb_trace")
    names = bb.nproblem.problem.vars
    return [(int(par[i]), None if var[i] < 0 else names[var[i]], int(sen[i]), float(bnd[i]), int(out[i]),
             float(obj[i])) for i in range(k)]
