"""IGXSolveNonlinear in the C ABI (include/petiga_amd.h) and its Python view, and the restatement of its loop (tests/newton_ref.py) on
the CPU: the call is declared, exported and bound; the two structs have the size a C compiler gives them; every refusal that is decided
before any HIP call, by code and word; exact Newton on the CPU oracle's Bratu (quadratic convergence); constant against Eisenstat-Walker
forcing; the two line searches on arctan; and the inputs of the line-search tests of tests/test_gpu_newton.py, found here on the oracle
and committed as constants (LS_CONVERGES, LS_DIVERGES)."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import krylov_ref as K
import newton_ref as N
from common import make_pair

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
HEADER = os.path.join(INCLUDE, "petiga_amd.h")

# the Dirichlet values of "bratu-p3" in tests/test_gpu_matrix_action.py (a GPU module: restated, and held equal below)
BRATU_BCS = [(d, s, 0, 0.1 * d * s) for d in range(3) for s in range(2)]
BRATU_P3 = dict(p=3, N=(4, 4, 4))
EXACT_NEWTON_ITERATIONS = 3      # recorded: Bratu 3.5 on bratu-p3 from x0 = 0 with the direct solve reaches 1e-12 |F_0| in 3 steps

# ---- the inputs of the GPU line-search tests, found on the oracle with the direct solve (test_line_search_inputs_* hold them)
# (i) backtracks and still converges: the first step from the constant guess overshoots (|F| 1.7e2 -> 7.0e5 at lambda = 1, 5.5e2 at 1/2,
#     1.3e2 at 1/4), every later step is a full one.  The small discretisation keeps the inner solves short (the Jacobian at the guess is
#     indefinite: 3.5 e^4 is above the Laplacian's lowest eigenvalue) and the margins of every acceptance test wide.
LS_CONVERGES = dict(p=2, N=(3, 3, 3), lam=3.5, guess=4.0, max_backtracks=8, maxit=20, rtol=1e-10, lambdas=[0.25, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
#     As an IFunction with a = LS_IFUNCTION_A and W = -a x0 (a backward-Euler step from the guess) the same input backtracks the same way.
LS_IFUNCTION_A = 2.0
# (ii) beyond the fold (no solution): the iteration settles at a positive minimum of |F| and the halvings run out in the sixth step
LS_DIVERGES = dict(p=3, N=(4, 4, 4), lam=10.0, guess=0.0, max_backtracks=8, maxit=20, rtol=1e-10, iterations=5, backtracks=25)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_declared_exported_and_bound():
    import petiga_amd as P
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", _header())}
    assert "IGXSolveNonlinear" in decl, "not declared in include/petiga_amd.h"
    args = [a.strip() for a in decl["IGXSolveNonlinear"].split(",") if a.strip()]
    assert len(args) == 6
    f = P.lib().IGXSolveNonlinear                      # AttributeError: the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == 6
    assert callable(P.IGX.solve_nonlinear)
    text = _header()
    for word, value in (("IGX_NEWTON_CONVERGED_FNORM_ABS", N.CONVERGED_FNORM_ABS), ("IGX_NEWTON_CONVERGED_FNORM_RELATIVE", N.CONVERGED_FNORM_RELATIVE),
                        ("IGX_NEWTON_CONVERGED_SNORM_RELATIVE", N.CONVERGED_SNORM_RELATIVE), ("IGX_NEWTON_DIVERGED_LINEAR_SOLVE", N.DIVERGED_LINEAR_SOLVE),
                        ("IGX_NEWTON_DIVERGED_FNORM_NAN", N.DIVERGED_FNORM_NAN), ("IGX_NEWTON_DIVERGED_MAX_IT", N.DIVERGED_MAX_IT),
                        ("IGX_NEWTON_DIVERGED_LINE_SEARCH", N.DIVERGED_LINE_SEARCH), ("IGX_LINESEARCH_BASIC", 0), ("IGX_LINESEARCH_BT", 1),
                        ("IGX_FORCING_CONSTANT", 0), ("IGX_FORCING_EW2", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (word, value), text), word
    assert P.NEWTON_LINESEARCHES == dict(basic=0, bt=1) and P.NEWTON_FORCINGS == dict(constant=0, ew2=1)
    assert set(P.NEWTON_REASONS) >= {2, 3, 4, -3, -4, -5, -6}


def test_struct_sizes_are_the_c_compilers(tmp_path):
    import petiga_amd as P
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "petiga_amd.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(IGXNewtonSpec), sizeof(IGXNewtonInfo)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", INCLUDE, "-o", str(exe), str(src)])
    spec, info = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert (spec, info) == (C.sizeof(P.IGXNewtonSpec), C.sizeof(P.IGXNewtonInfo))
    # the members in the header's order
    for name in ("IGXNewtonSpec", "IGXNewtonInfo"):
        m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header())
        names = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert names == [f[0] for f in getattr(P, name)._fields_], name


def _box(setup=True):
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i, Nel in enumerate((4, 3, 3)):
        g.axis_uniform(i, 2, Nel)
    if setup:
        g.setup()
    return g


def _rc(g, **kw):
    """IGXSolveNonlinear with a null x: every refusal tested here is decided before x is looked at"""
    import petiga_amd as P
    d = dict(op=1, a=0.0, t=0.0, W=None, method=1, pc=0, lin_rtol=1e-5, lin_atol=0.0, lin_maxit=100, forcing=0, rtol=1e-8, atol=0.0, stol=0.0, maxit=10,
             linesearch=0, max_backtracks=5)
    d.update(kw)
    spec = P.IGXNewtonSpec(*[d[f[0]] for f in P.IGXNewtonSpec._fields_])
    info = P.IGXNewtonInfo()
    rc = P.lib().IGXSolveNonlinear(g.h, C.byref(spec), None, C.byref(info), None, None)
    return rc, P.lib().IGXGetLastError().decode()


def test_refusals_decided_before_any_hip_call():
    import petiga_amd as P
    g = _box()
    g.set_form("bratu", (3.5,))
    nan = float("nan")
    for kw in (dict(op=0), dict(op=3), dict(op=-1), dict(method=2), dict(method=-1), dict(pc=4), dict(pc=-1), dict(linesearch=2), dict(linesearch=-1), dict(forcing=2),
               dict(forcing=-1), dict(rtol=-1e-8), dict(atol=-1.0), dict(stol=-1.0), dict(lin_rtol=-1e-3), dict(lin_atol=-1.0), dict(rtol=nan), dict(atol=nan),
               dict(stol=nan), dict(lin_rtol=nan), dict(lin_atol=nan), dict(maxit=-1), dict(lin_maxit=-1), dict(max_backtracks=-1)):
        rc, why = _rc(g, **kw)
        assert rc == 63 and "IGXSolveNonlinear" in why, (kw, rc, why)
    rc, why = _rc(g, op=0)
    assert "IGX_OP_MATRIX" in why
    for key, word in (("method", "method"), ("pc", "preconditioner"), ("linesearch", "line search"), ("forcing", "forcing"), ("max_backtracks", "max_backtracks")):
        assert word in _rc(g, **{key: -1})[1], key
    assert "tolerance" in _rc(g, stol=nan)[1] and "maxit" in _rc(g, lin_maxit=-1)[1]
    rc, why = _rc(g)
    assert rc == 62 and "null" in why, (rc, why)                  # in range: now x is looked at
    rc, why = _rc(g, op=2)
    assert rc == 62 and "W" in why, (rc, why)                     # the IFunction's W is missing
    assert P.lib().IGXSolveNonlinear(g.h, None, None, None, None, None) == 62
    rc, why = _rc(g, pc=3)
    assert rc == 58 and "IGXFastDiagSetUp" in why, (rc, why)

    rc, why = _rc(_box(setup=False))                              # before IGXSetUp
    assert rc == 58 and "IGXSetUp" in why, (rc, why)

    rc, why = _rc(_box())                                         # no form set
    assert rc == 73 and "Form" in why, (rc, why)

    g = _box(setup=False)
    g.set_comm(2, 0)
    g.set_processors(1, 2)
    g.setup()
    g.set_form("bratu", (3.5,))
    rc, why = _rc(g)                                              # IGXSolve refuses two ranks too: it arrives under the Newton solve's name
    assert rc == 56 and "Newton solve" in why and "rank" in why, (rc, why)
    with pytest.raises(P.IGXError) as e:
        g.solve_nonlinear(None)
    assert e.value.code == 56 and "Newton solve" in str(e.value)


# ---- the restatement on the CPU oracle
@functools.lru_cache(maxsize=None)
def _bratu_oracle(p, Nel):
    orc, _ = make_pair(3, 1, p, list(Nel), engine=False)
    for bc in BRATU_BCS:
        orc.set_boundary_value(*bc)
    return orc


def _bratu_callables(p, Nel, lam, **kw):
    return N.oracle_callables(_bratu_oracle(p, tuple(Nel)), "orc_form_bratu_function", "orc_form_bratu_jacobian", C.c_double(lam), **kw)


def test_bratu_p3_is_the_case_of_the_action_tests():
    from test_gpu_matrix_action import CASES
    form, dof, p, Nel, kw, geo, bcs, _ = CASES["bratu-p3"]
    assert (form, dof, p, tuple(Nel), kw, geo, bcs) == ("bratu", 1, BRATU_P3["p"], BRATU_P3["N"], {}, None, BRATU_BCS)


@functools.lru_cache(maxsize=None)
def _exact_bratu():
    fun, lin = _bratu_callables(BRATU_P3["p"], BRATU_P3["N"], 3.5)
    n = _bratu_oracle(BRATU_P3["p"], BRATU_P3["N"]).global_size()
    x, info = N.newton(fun, lin, np.zeros(n), rtol=1e-12, maxit=20)
    x.setflags(write=False)
    return x, info


def test_exact_newton_on_the_oracles_bratu_converges_quadratically():
    x, info = _exact_bratu()
    r = info["history"] / info["fnorm0"]
    print("exact Newton, Bratu 3.5 on bratu-p3: %d iterations, |F_k| / |F_0| = %s" % (info["iterations"], r))
    assert info["reason"] == N.CONVERGED_FNORM_RELATIVE and info["iterations"] == EXACT_NEWTON_ITERATIONS
    assert r[-1] <= 1e-12 and info["function_evaluations"] == 1 + info["iterations"] and info["backtracks"] == 0
    # at least quadratic below 1e-2: r_{k+1} <= r_k^2, down to the residual's rounding floor (1e-13 |F_0|: 1e3 u on sums of O(1) terms)
    quadratic = [(a, b) for a, b in zip(r[:-1], r[1:]) if a < 1e-2]
    assert len(quadratic) >= 2 and all(b <= max(a * a, 1e-13) for a, b in quadratic), r
    # the fixed rows hold their Dirichlet values
    J = _bratu_oracle(BRATU_P3["p"], BRATU_P3["N"]).compute_jacobian("orc_form_bratu_jacobian", C.c_double(3.5), x).scipy().tocsr()
    off = abs(J)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    assert fixed.sum() == 7 ** 3 - 5 ** 3 and set(np.round(x[fixed], 12)) <= {0.0, 0.1, 0.2}


def test_constant_and_eisenstat_walker_forcing_reach_the_same_solution():
    want, _ = _exact_bratu()
    n = want.size
    runs = {}
    for forcing, lin_rtol in (("constant", 1e-8), ("ew2", 1e-3)):
        fun, lin = _bratu_callables(BRATU_P3["p"], BRATU_P3["N"], 3.5, iterative="cg")
        x, info = N.newton(fun, lin, np.zeros(n), rtol=1e-10, maxit=30, lin_rtol=lin_rtol, forcing=forcing)
        print("%s: %d iterations, inner %s, eta %s, max|x - exact| / max|x| = %.3e" % (forcing, info["iterations"], info["linear_its"], info["etas"], np.abs(x - want).max() / np.abs(want).max()))
        assert info["reason"] == N.CONVERGED_FNORM_RELATIVE
        # |x - x*| <= |J^-1| |F|: the residual is below 1e-10 |F_0| and cond(J) is O(1e2) on this mesh
        assert np.abs(x - want).max() <= 1e-8 * np.abs(want).max()
        runs[forcing] = info
    assert all(e == 1e-8 for e in runs["constant"]["etas"])
    etas = runs["ew2"]["etas"]
    assert etas[0] == 1e-3 and all(0 < e <= 0.9 for e in etas) and etas[1] == 0.9 * (runs["ew2"]["history"][1] / runs["ew2"]["history"][0]) ** 2
    assert runs["ew2"]["linear_iterations"] < runs["constant"]["linear_iterations"]


def test_forcing_safeguard_and_cap():
    """the two clauses of choice 2 on a scripted sequence of norms: f = 1, 1.5 (eta_1 = 2.025 capped at 0.9), 1e-3 (0.9 eta_1^2 = 0.729 > 0.1 holds eta_2 up)"""
    norms = iter([1.0, 1.5, 1e-3, 1e-9])
    fun = lambda x: np.array([next(norms)])
    seen = []
    lin = lambda x, F, eta: (seen.append(eta) or np.ones(1), 1, K.CONVERGED_RTOL)
    _, info = N.newton(fun, lin, np.zeros(1), rtol=1e-8, stol=0.0, atol=1e-9, maxit=5, lin_rtol=0.5, forcing="ew2")
    assert info["reason"] == N.CONVERGED_FNORM_ABS and info["iterations"] == 3
    assert seen == [0.5, 0.9, 0.9 * (0.9 * 0.9)], seen


def test_line_searches_on_arctan():
    fun = lambda x: np.arctan(x)
    lin = lambda x, F, eta: (F * (1.0 + x * x), 1, K.CONVERGED_RTOL)
    x0 = np.full(5, 3.0)
    with np.errstate(all="ignore"):
        x, info = N.newton(fun, lin, x0, rtol=1e-12, maxit=12, linesearch="basic")
    print("basic: reason %d after %d iterations, |F| %s" % (info["reason"], info["iterations"], info["history"]))
    assert info["reason"] in (N.DIVERGED_FNORM_NAN, N.DIVERGED_MAX_IT) and np.all(np.diff(info["history"]) >= 0) and info["backtracks"] == 0
    x, info = N.newton(fun, lin, x0, rtol=1e-12, maxit=12, linesearch="bt")
    print("bt: reason %d after %d iterations, lambdas %s" % (info["reason"], info["iterations"], info["lambdas"]))
    assert info["reason"] == N.CONVERGED_FNORM_ABS and info["fnorm"] == 0.0 and info["backtracks"] == 2      # (arctan underflows to 0 <= atol = 0: the test of atol comes first)
    assert info["lambdas"] == [[1.0, 0.5, 0.25], [1.0], [1.0], [1.0]]
    assert info["function_evaluations"] == 1 + info["iterations"] + info["backtracks"] and np.abs(x).max() <= 1e-12
    _, info = N.newton(fun, lin, x0, rtol=1e-12, maxit=12, linesearch="bt", max_backtracks=1)
    assert info["reason"] == N.DIVERGED_LINE_SEARCH and info["iterations"] == 0 and info["lambdas"] == [[1.0, 0.5]]
    assert info["function_evaluations"] == 1 + info["iterations"] + info["backtracks"] + 1      # the trial that was not accepted


def _recorded_norms(fun):
    norms = []

    def wrapped(x):
        F = fun(x)
        norms.append(float(np.linalg.norm(F)))
        return F
    return wrapped, norms


def test_line_search_input_that_backtracks_and_converges():
    c = LS_CONVERGES
    n = _bratu_oracle(c["p"], c["N"]).global_size()
    for iterative in (None, "bicgstab"):      # the margins hold with an inner solve to 1e-8 as the GPU test runs it
        fun, lin = _bratu_callables(c["p"], c["N"], c["lam"], iterative=iterative, lin_maxit=200)
        fun, norms = _recorded_norms(fun)
        x, info = N.newton(fun, lin, np.full(n, c["guess"]), rtol=c["rtol"], lin_rtol=1e-8, maxit=c["maxit"], linesearch="bt", max_backtracks=c["max_backtracks"])
        print("direct" if iterative is None else iterative, info["lambdas"], info["linear_its"], ["%.4e" % v for v in norms])
        assert info["reason"] == N.CONVERGED_FNORM_RELATIVE and info["backtracks"] >= 1
        assert [tried[-1] for tried in info["lambdas"]] == c["lambdas"]
        assert max(info["linear_its"]) < 200
        # every acceptance test is decided by a wide margin: no |F_t| within 1e-3 of its threshold
        k, f = 1, norms[0]
        for tried in info["lambdas"]:
            for lam in tried:
                assert abs(norms[k] - (1.0 - 1e-4 * lam) * f) > 1e-3 * f
                k += 1
            f = norms[k - 1]


def test_line_search_input_as_an_ifunction_backtracks_in_its_first_step():
    c, a = LS_CONVERGES, LS_IFUNCTION_A
    orc = _bratu_oracle(c["p"], c["N"])
    x0 = np.full(orc.global_size(), c["guess"])
    for iterative in (None, "bicgstab"):
        fun, lin = N.oracle_callables(orc, "orc_form_bratu_ifunction", "orc_form_bratu_ijacobian", C.c_double(c["lam"]), op="ijacobian", a=a, W=-a * x0, iterative=iterative, lin_maxit=200)
        fun, norms = _recorded_norms(fun)
        x, info = N.newton(fun, lin, x0, rtol=c["rtol"], lin_rtol=1e-8, maxit=c["maxit"], linesearch="bt", max_backtracks=c["max_backtracks"])
        print("direct" if iterative is None else iterative, info["lambdas"], info["linear_its"], ["%.4e" % v for v in norms])
        assert info["reason"] == N.CONVERGED_FNORM_RELATIVE and info["lambdas"][0] == [1.0, 0.5, 0.25] and info["iterations"] >= 3
        assert all(t == [1.0] for t in info["lambdas"][1:]) and max(info["linear_its"]) < 200
        k, f = 1, norms[0]
        for tried in info["lambdas"]:
            for lam in tried:
                assert abs(norms[k] - (1.0 - 1e-4 * lam) * f) > 1e-3 * f
                k += 1
            f = norms[k - 1]


def test_line_search_input_that_diverges():
    c = LS_DIVERGES
    n = _bratu_oracle(c["p"], c["N"]).global_size()
    for iterative in (None, "bicgstab"):
        fun, lin = _bratu_callables(c["p"], c["N"], c["lam"], iterative=iterative, lin_maxit=200)
        fun, norms = _recorded_norms(fun)
        x, info = N.newton(fun, lin, np.full(n, c["guess"]), rtol=c["rtol"], lin_rtol=1e-8, maxit=c["maxit"], linesearch="bt", max_backtracks=c["max_backtracks"])
        print("direct" if iterative is None else iterative, info["lambdas"], info["linear_its"])
        assert info["reason"] == N.DIVERGED_LINE_SEARCH and info["iterations"] == c["iterations"] < c["maxit"] and info["backtracks"] == c["backtracks"]
        assert info["function_evaluations"] == 1 + info["iterations"] + info["backtracks"] + 1
        assert np.array_equal(x, info["iterates"][-1]) and max(info["linear_its"]) < 200
        k, f = 1, norms[0]
        for tried in info["lambdas"]:
            for lam in tried:
                assert abs(norms[k] - (1.0 - 1e-4 * lam) * f) > 1e-6 * f
                k += 1
            f = norms[k - 1]
