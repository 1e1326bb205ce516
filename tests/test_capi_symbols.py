"""CPU-side checks of the drop-in boundary: libmi355x_simplex.so builds for gfx950, loads, and
exports every symbol include/mi355x_simplex.h declares; nothing computes without a GPU and
nothing falls back to the CPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import ROOT, lp_amd

lp = lp_amd()
HEADER = os.path.join(ROOT, "include", "mi355x_simplex.h")
TUNE_HEADER = os.path.join(ROOT, "include", "mi355x_simplex_tune.h")


def declared_functions(header=HEADER, test_hooks=False):
    """Functions a header declares; the `#ifdef MI355X_TEST_HOOKS` section (fault injection, the
    test build of the library only) is left out unless test_hooks."""
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not test_hooks:
        src = re.sub(r"#ifdef MI355X_TEST_HOOKS.*?#endif", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mi355x_[a-z0-9_]+)\s*\(", src)))


def test_library_is_built_and_loads():
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.exists(lp.capi.LIB_PATH)
    L = lp.capi.lib()
    assert L.mi355x_abi_version() == 1
    assert L.mi355x_epsilon() == 2.0 ** -53 * (1 + 2.0 ** -52)
    assert L.mi355x_update_kernel_name().decode() == "k_update"


def test_every_declared_symbol_is_exported_and_bound():
    names = declared_functions()
    assert len(names) >= 25
    L = ctypes.CDLL(lp.capi.LIB_PATH)
    for name in names:
        assert hasattr(L, name), "%s declared in the header but not exported" % name
    assert sorted(lp.capi.SIGNATURES) == names, "capi.py and the header disagree"


def test_tuning_hooks_are_declared_exported_and_bound():
    """include/mi355x_simplex_tune.h is the one place the non-boundary hooks are declared; the
    library exports exactly the union of the two headers (nothing undeclared)."""
    names = declared_functions(TUNE_HEADER)
    assert len(names) >= 15 and not set(names) & set(declared_functions())
    L = ctypes.CDLL(lp.capi.LIB_PATH)
    for name in names:
        assert hasattr(L, name), "%s declared in the tuning header but not exported" % name
    assert sorted(lp.capi._EXTRA) == names, "capi.py and the tuning header disagree"
    out = subprocess.check_output(["nm", "-D", "--defined-only", lp.capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and "mi355x_" in l}
    assert exported == set(names) | set(declared_functions()), \
        "undeclared exports: %s" % sorted(exported - set(names) - set(declared_functions()))


def test_fault_injection_hooks_exist_in_the_test_build_only():
    """The fault-injection hooks are compiled in with -DMI355X_TEST_HOOKS only: the product library
    exports none of them, the test build (same sources) exports exactly the product's symbols plus
    the hooks, and capi.py binds them only on the test build."""
    hooks = set(declared_functions(TUNE_HEADER, test_hooks=True)) - set(declared_functions(TUNE_HEADER))
    assert hooks == set(lp.capi._TEST_HOOKS) and len(hooks) >= 2

    def exports(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {l.split()[-1] for l in out.splitlines() if " T " in l and "mi355x_" in l}
    assert os.path.exists(lp.capi.TEST_LIB_PATH)
    product, test = exports(lp.capi.LIB_PATH), exports(lp.capi.TEST_LIB_PATH)
    assert not hooks & product
    assert test == product | hooks
    with lp.capi.test_build() as L:
        assert L is not None and L.mi355x_tune_set_la_fault(0) == 0
    assert not hasattr(lp.capi.lib(), "_never") and lp.capi.lib() is not L


def test_exports_are_plain_c_symbols():
    out = subprocess.check_output(["nm", "-D", "--defined-only", lp.capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in declared_functions():
        assert name in exported


def test_code_object_targets_gfx950():
    blob = open(lp.capi.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"k_update" in blob and b"k_select" in blob


def test_library_does_not_link_the_oracle_or_torch():
    out = subprocess.check_output(["ldd", lp.capi.LIB_PATH], text=True)
    assert "liboracle" not in out and "torch" not in out
    assert "libamdhip64" in out


@pytest.mark.skipif(lp.capi.device_count() > 0, reason="a GPU is present")
def test_no_device_means_loud_failure_not_fallback():
    assert lp.capi.device_count() == 0
    M = np.zeros((3, 4))
    h = ctypes.c_void_p()
    rc = lp.capi.lib().mi355x_tab_create(ctypes.byref(h), 3, 4, M.ctypes.data_as(ctypes.c_void_p),
                                         None, 0)
    assert rc == lp.capi.MI_NO_DEVICE and not h.value
    assert b"no HIP device" in lp.capi.lib().mi355x_last_error()
    t = lp.Tableau(None, lp.Problem(), M, np.zeros(2, dtype=np.int64), 3, 2, {})
    with pytest.raises(lp.capi.Mi355xError):
        lp.n_solve_tableau(t)
    with pytest.raises(lp.capi.Mi355xError):
        lp.find_entering_column(t)


def test_argument_validation_without_device():
    L = lp.capi.lib()
    assert L.mi355x_tab_pivot(None, 0, 0) == lp.capi.MI_BAD_ARG
    assert L.mi355x_tab_solve(None, 1, 1024.0, 0, None) == lp.capi.MI_BAD_ARG
    assert L.mi355x_tab_download(None, None, None, None, None) == lp.capi.MI_BAD_ARG
    h = ctypes.c_void_p()
    assert L.mi355x_tab_create(ctypes.byref(h), 3, 4, None, None, 0) == lp.capi.MI_BAD_ARG
    assert L.mi355x_tab_create_synthetic(ctypes.byref(h), 0, 4, 1, 0, -1, 0) == lp.capi.MI_BAD_ARG
    L.mi355x_tab_destroy(None)                       # no-op


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "linear-programming_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".inc", ".cpp", ".lisp", ".asd")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "liboracle" not in text and "simplex_oracle" not in text, f


def test_header_is_plain_c_and_a_c_program_links(tmp_path):
    """gcc -std=c11 -Wall -Werror on a C client of the header, linked against the library."""
    exe = str(tmp_path / "c_abi_check")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_check.c"), "-o", exe,
                           "-L", os.path.dirname(lp.capi.LIB_PATH), "-lmi355x_simplex",
                           "-Wl,-rpath," + os.path.dirname(lp.capi.LIB_PATH)])
    out = subprocess.check_output([exe], text=True)
    assert "c abi ok" in out


def test_lisp_glue_is_well_formed_and_binds_only_declared_entry_points():
    """The CFFI glue cannot be executed here (no Common Lisp in the image): at least its forms
    are balanced, every foreign function it binds is declared in the public header with the same
    number of arguments, and every status constant it names has the header's value."""
    import re
    src = open(os.path.join(ROOT, "linear-programming_amd", "lisp", "mi355x-simplex.lisp")).read()
    depth, i, in_str, in_comment = 0, 0, False, False
    while i < len(src):
        c = src[i]
        if in_comment:
            in_comment = c != "\n"
        elif in_str:
            if c == "\\":
                i += 1
            elif c == '"':
                in_str = False
        elif c == ";":
            in_comment = True
        elif c == '"':
            in_str = True
        elif c == "#" and src[i + 1] == "\\":
            i += 2
        elif c == "(":
            depth += 1
        elif c == ")":
            depth -= 1
            assert depth >= 0, "unbalanced ')' at offset %d" % i
        i += 1
    assert depth == 0 and not in_str
    header = open(os.path.join(ROOT, "include", "mi355x_simplex.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    bound = list(re.finditer(r'\(cffi:defcfun \("(mi355x_\w+)" %?[\w-]+\)\s+\S+?((?:\s*\([\w-]+ [^()]+\))*)\)', src))
    assert len(bound) == src.count("cffi:defcfun") >= 11          # (every binding is looked at)
    for m in bound:
        name, args = m.group(1), re.findall(r"\([\w-]+ [^()]+\)", m.group(2))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, flat, flags=re.S)
        assert decl, "%s is bound by the glue but not declared in mi355x_simplex.h" % name
        params = [p for p in decl.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), "%s: the glue passes %d arguments, the header declares %d" % (name, len(args), len(params))
    for m in re.finditer(r"\(defconstant \+mi-([\w-]+)\+ (-?\d+)\)", src):
        macro = "MI_" + m.group(1).upper().replace("-", "_")
        decl = re.search(r"#define\s+%s\s+(-?\d+)" % macro, header)
        assert decl and int(decl.group(1)) == int(m.group(2)), "%s = %s in the glue" % (macro, m.group(2))


def _glue_source():
    return open(os.path.join(ROOT, "linear-programming_amd", "lisp", "mi355x-simplex.lisp")).read()


def test_lisp_glue_binds_the_native_route_and_has_a_method_on_every_generic():
    """SURVEY section 8 f-2 / f-3 from the reference's host language: the glue binds the whole
    problem -> solution path (mi355x_problem_*, the resumable solver job, mi355x_solution_*), has one
    method per solution-* generic of src/solver.lisp:59-80 on its own solution class, signals the
    reference's errors in the read-back (src/simplex.lisp:85-86, 117-118), and every foreign
    function it CALLS is one it binds."""
    src = _glue_source()
    code = re.sub(r";[^\n]*", "", src)
    bound_c = set(re.findall(r'\(cffi:defcfun \("(mi355x_\w+)"', src))
    for name in ("mi355x_problem_create", "mi355x_problem_set_objective", "mi355x_problem_set_bounds",
                 "mi355x_problem_set_integer", "mi355x_problem_add_constraint", "mi355x_problem_destroy",
                 "mi355x_simplex_solver", "mi355x_simplex_solver_begin", "mi355x_simplex_solver_step",
                 "mi355x_simplex_solver_finish", "mi355x_simplex_solver_abandon", "mi355x_var_mapping",
                 "mi355x_solution_objective_value", "mi355x_solution_variable", "mi355x_solution_reduced_cost",
                 "mi355x_solution_pivots", "mi355x_solution_destroy", "mi355x_two_phase_handover"):
        assert name in bound_c, "%s is not bound by the glue" % name
    # every %foreign-function the glue calls is bound, and every binding (but the documented one-shot
    # conveniences) is used
    bound_lisp = set(re.findall(r'\(cffi:defcfun \("mi355x_\w+" (%?[\w-]+)\)', src))
    body = re.sub(r'\(cffi:defcfun \("mi355x_\w+" %?[\w-]+\)', "", code)
    called = set(re.findall(r"\((%[\w-]+)[\s)]", body))
    assert called <= bound_lisp, "called but never bound: %s" % sorted(called - bound_lisp)
    unused = {n for n in bound_lisp if n.startswith("%")} - called
    assert unused <= {"%simplex-solver", "%solve-two-phase", "%multibatch-solve-two-phase"}, "bound but never called: %s" % sorted(unused)
    # the four generics of src/solver.lisp:59-80, imported from the reference's package and specialised
    assert "(:import-from :linear-programming/solver" in src
    for generic, params in (("solution-problem", r"\(\(solution mi355x-solution\)\)"),
                            ("solution-objective-value", r"\(\(solution mi355x-solution\)\)"),
                            ("solution-variable", r"\(\(solution mi355x-solution\) variable\)"),
                            ("solution-reduced-cost", r"\(\(solution mi355x-solution\) variable\)")):
        assert re.search(r"#:%s\b" % generic, src), "%s is not imported" % generic
        assert re.search(r"\(defmethod %s %s" % (generic, params), src), "no method on %s" % generic
    assert "(defclass mi355x-solution" in src and "sb-ext:finalize" in src and "(defun free-solution" in src
    # the reference's error texts of the read-back
    assert '"~S is not a variable in the tableau"' in src and '"~S has no lower bound"' in src
    # the solver takes the native route by default and keeps the build-tableau route
    solver = src[src.index("(defun mi355x-simplex-solver"):src.index(";;; ------------------------------------------------------------------ many problems at once")]
    assert "(native :auto)" in solver and "(solve-natively problem" in solver and "(build-tableau problem problem" in solver
    assert solver.index("(solve-natively problem") < solver.index("(build-tableau problem problem")
    # never an unbounded foreign solve: every solve entry point is called with a cap through solve-in-chunks
    for fn in ("%tab-solve", "%colpart-solve", "%solver-step"):
        for m in re.finditer(r"\(%s " % re.escape(fn), body):
            ctx = body[max(0, m.start() - 120):m.start()]
            assert "(lambda (cap)" in ctx, "%s is called outside solve-in-chunks" % fn


def test_python_mirror_replays_the_glue_call_for_call():
    """The C entry points the glue's native route calls are exactly those NativeProblem (marshal) +
    NativeProblem.solve_in_chunks (begin / step / finish / abandon) + NativeSolution (read-back) call:
    the GPU tests of the native route (tests/test_gpu_native_route.py) exercise the glue's sequence."""
    src = _glue_source()
    native = src[src.index(";;; ------------------------------------------------------------------ the native route"):
                 src.index("(defun solve-two-phase-in-chunks")]
    lisp_to_c = dict((l, c) for c, l in re.findall(r'\(cffi:defcfun \("(mi355x_\w+)" (%[\w-]+)\)', src))
    glue_calls = {lisp_to_c[n] for n in set(re.findall(r"\((%[\w-]+)[\s)]", re.sub(r";[^\n]*", "", native)))}
    py = open(os.path.join(ROOT, "linear-programming_amd", "native.py")).read()
    py_calls = set(re.findall(r"\b(mi355x_(?:problem|simplex_solver|solution|var_mapping)\w*)\(", py))
    py_calls -= {"mi355x_problem_read_mps", "mi355x_problem_read_mps_ex", "mi355x_problem_to_json", "mi355x_simplex_solver"}   # (the MPS reader, the one-shot form)
    assert glue_calls == py_calls, (sorted(glue_calls - py_calls), sorted(py_calls - glue_calls))


# ---- static guards of the glue (round-5 review, item 5): it cannot be executed here, so everything that CAN be
# checked without a Lisp reader is a test -- argument and return TYPES of every binding, every imported symbol
# against the reference's export lists, every keyword of the solver's lambda list against INTEGRATION.md
_CFFI_OF_C = {"int": ":int", "int64_t": ":int64", "double": ":double", "void": ":void", "unsigned": ":uint",
              "unsigned int": ":uint", "uint64_t": ":uint64", "int32_t": ":int32"}


def _c_params(decl_args):
    """Parameter type strings of a C declaration's argument list (names and comments stripped)."""
    out = []
    for a in decl_args.split(","):
        a = " ".join(a.split())
        if not a or a == "void":
            continue
        if "*" in a:
            out.append("pointer")
            continue
        toks = [t for t in a.split(" ") if t not in ("const",)]
        # the last token is the parameter's name unless the declaration is anonymous
        typ = " ".join(toks[:-1]) if len(toks) > 1 else toks[0]
        out.append(typ)
    return out


def test_lisp_glue_binding_types_match_the_header():
    """Every (cffi:defcfun ...) passes arguments of the header's TYPES and takes the header's return type:
    int <-> :int, int64_t <-> :int64, double <-> :double, any pointer <-> :pointer (const char * may be :string).
    An :int where the header says int64_t would corrupt the call on the first pivot count above 2^31, or
    silently pass garbage in the upper half of a register -- nothing a Lisp compiler can notice."""
    src = _glue_source()
    header = open(os.path.join(ROOT, "include", "mi355x_simplex.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    bound = list(re.finditer(r'\(cffi:defcfun \("(mi355x_\w+)" %?[\w-]+\)\s+(\S+?)((?:\s*\([\w-]+ [^()]+\))*)\)', src))
    assert len(bound) == src.count("cffi:defcfun") >= 11
    checked = 0
    for m in bound:
        name, ret = m.group(1), m.group(2)
        args = [a.split()[-1].rstrip(")") for a in re.findall(r"\([\w-]+ [^()]+\)", m.group(3))]
        decl = re.search(r"([\w\s\*]+?)\b%s\s*\(([^;]*?)\)\s*;" % name, flat, flags=re.S)
        assert decl, name
        c_ret = " ".join(decl.group(1).replace("extern", "").split())
        if "*" in c_ret:
            assert ret in (":pointer", ":string"), "%s returns %s, the glue says %s" % (name, c_ret, ret)
        else:
            assert _CFFI_OF_C.get(c_ret) == ret, "%s returns %s, the glue says %s" % (name, c_ret, ret)
        params = _c_params(decl.group(2))
        assert len(params) == len(args), name
        for k, (c_t, l_t) in enumerate(zip(params, args)):
            want = ":pointer" if c_t == "pointer" else _CFFI_OF_C.get(c_t)
            assert want is not None, "%s: unknown C type %r" % (name, c_t)
            assert l_t == want or (want == ":pointer" and l_t == ":string"), \
                "%s: argument %d is %s in the header, %s in the glue" % (name, k + 1, c_t, l_t)
            checked += 1
    assert checked > 150


def test_lisp_glue_imports_only_what_the_reference_exports():
    """Every symbol of every (:import-from pkg ...) is in the :export list of the reference file that defines
    pkg (src/simplex.lisp:14-35, src/problem.lisp:15-40, src/solver.lisp:20-30, src/conditions.lisp:3-11) --
    from the committed fixture (`python tools/gen_reference_exports.py REFERENCE_TREE` writes it)."""
    import json
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_exports.json")))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_reference_exports
    # (the fixture as the tool writes it: one package per file the tool reads, sorted unique symbols)
    assert sorted(v["file"] for v in fix.values()) == sorted("src/%s.lisp" % f for f in gen_reference_exports.FILES)
    assert all(v["exports"] == sorted(set(v["exports"])) for v in fix.values())
    src = re.sub(r";[^\n]*", "", _glue_source())
    imports = re.findall(r"\(:import-from :([\w/.-]+)((?:\s+#:[^\s()]+)+)\)", src)
    assert len(imports) >= 4
    n = 0
    for pkg, syms in imports:
        assert pkg in fix, "the glue imports from %s, which is not a reference package of the path" % pkg
        for s in syms.split():
            s = s[2:].lower()
            assert s in fix[pkg]["exports"], "%s is not exported by %s (%s)" % (s, pkg, fix[pkg]["file"])
            n += 1
    assert n >= 20
    # and what the glue uses package-qualified
    for pkg, sym in set(re.findall(r"\b(linear-programming/[\w-]+):([\w*+<>=-]+)", src)):
        assert sym.lower() in fix[pkg]["exports"], "%s:%s" % (pkg, sym)


def test_solver_keywords_are_documented_in_integration_md():
    """Every keyword of mi355x-simplex-solver's and mi355x-solve-problems' lambda lists appears in
    INTEGRATION.md (the maintainer's side of the boundary) and in the function's own docstring."""
    src = _glue_source()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in ("mi355x-simplex-solver", "mi355x-solve-problems"):
        m = re.search(r"\(defun %s \(problems? &rest args\s+&key(.*?)&allow-other-keys\)\s+\"(.*?)\"" % fn, src, flags=re.S)
        assert m, fn
        keys = re.findall(r"\(?([a-z][\w-]*)", re.sub(r"\([\w-]+ [^()]*\)", lambda mm: "(" + mm.group(0)[1:].split()[0] + ")", m.group(1)))
        keys = [k for k in keys if k not in ("t", "nil")]
        assert len(keys) >= 6, keys
        for k in keys:
            assert ":" + k in m.group(2) or k.upper() in m.group(2), "%s: :%s is not in the docstring" % (fn, k)
            assert ":" + k in doc, "%s: :%s is not documented in INTEGRATION.md" % (fn, k)
