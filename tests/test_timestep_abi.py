"""IGXTimeStep in the C ABI (include/petiga_amd.h) and its Python view, and the restatement of its loop (tests/timestep_ref.py) on the CPU:
the call is declared, exported and bound; the structs have the size a C compiler gives them; every refusal that is decided before any HIP
call and needs no vector, by code and word; the radius parametrisation; the backward-Euler identities of the two sweeps.  The restatement
then runs a linear problem, M u' + K u = 0 with the oracle's Mass and Poisson matrices on a p = 2 (3,3,3) box (no Dirichlet face) and a
sparse direct stage solve, against the exact solution of the generalized eigen-decomposition: the schemes' orders, an adaptive run, a
failed stage, the shortened last step and resume; and two steps of the oracle's Bratu IFunction through tests/newton_ref.py."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import newton_ref as N
import timestep_ref as T
from common import greville, make_pair
from test_newton_abi import BRATU_BCS

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
HEADER = os.path.join(INCLUDE, "petiga_amd.h")

NEWTON_OK = dict(reason=N.CONVERGED_FNORM_RELATIVE, iterations=1, linear_iterations=1, function_evaluations=2)
NEWTON_FAILED = dict(reason=N.DIVERGED_MAX_IT, iterations=1, linear_iterations=1, function_evaluations=2)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_declared_exported_and_bound():
    import petiga_amd as P
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", _header())}
    assert "IGXTimeStep" in decl, "not declared in include/petiga_amd.h"
    args = [a.strip() for a in decl["IGXTimeStep"].split(",") if a.strip()]
    assert len(args) == 7
    f = P.lib().IGXTimeStep                      # AttributeError: the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == 7
    assert callable(P.IGX.time_step)
    text = _header()
    for word, value in (("IGX_TS_CONVERGED_TIME", T.CONVERGED_TIME), ("IGX_TS_CONVERGED_STEPS", T.CONVERGED_STEPS), ("IGX_TS_DIVERGED_NONLINEAR_SOLVE", T.DIVERGED_NONLINEAR_SOLVE),
                        ("IGX_TS_DIVERGED_STEP_REJECTED", T.DIVERGED_STEP_REJECTED), ("IGX_TS_DIVERGED_NAN", T.DIVERGED_NAN)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (word, value), text), word
    assert (T.CONVERGED_TIME, T.CONVERGED_STEPS, T.DIVERGED_NONLINEAR_SOLVE, T.DIVERGED_STEP_REJECTED, T.DIVERGED_NAN) == (1, 2, -1, -2, -3)
    assert set(P.TS_REASONS) >= {1, 2, -1, -2, -3}
    # the solver stack below it is what it was
    assert P.SOLVE_METHODS == dict(cg=0, bicgstab=1)
    assert P.TS_LOG_DTYPE.itemsize == C.sizeof(P.IGXTimeStepLog) and list(P.TS_LOG_DTYPE.names) == [f[0] for f in P.IGXTimeStepLog._fields_]
    for name, _ in P.IGXTimeStepLog._fields_:
        assert P.TS_LOG_DTYPE.fields[name][1] == getattr(P.IGXTimeStepLog, name).offset, name


def test_struct_sizes_are_the_c_compilers(tmp_path):
    import petiga_amd as P
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    names = ("IGXTimeStepSpec", "IGXTimeStepLog", "IGXTimeStepInfo", "IGXNewtonSpec", "IGXSolveSpec")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "petiga_amd.h"\n'
                   'int main(void) { printf("%s %%zu\\n", %s, offsetof(IGXTimeStepSpec, newton)); return 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("sizeof(%s)" % n for n in names)))
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[:-1] == [C.sizeof(getattr(P, n)) for n in names]
    assert got[-1] == P.IGXTimeStepSpec.newton.offset
    # the members in the header's order
    for name in names[:3]:
        m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header())
        members = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert members == [f[0] for f in getattr(P, name)._fields_], name


def _box(setup=True):
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i, Nel in enumerate((4, 3, 3)):
        g.axis_uniform(i, 2, Nel)
    if setup:
        g.setup()
    return g


def _rc(g, newton=None, **kw):
    """IGXTimeStep with null U and V: every refusal tested here is decided before they are looked at"""
    import petiga_amd as P
    nd = dict(op=2, a=0.0, t=0.0, W=None, method=1, pc=0, lin_rtol=1e-5, lin_atol=0.0, lin_maxit=100, forcing=0, rtol=1e-8, atol=0.0, stol=0.0, maxit=10,
              linesearch=0, max_backtracks=5)
    nd.update(newton or {})
    d = dict(alpha_m=5.0 / 6.0, alpha_f=2.0 / 3.0, gamma=2.0 / 3.0, t0=0.0, dt=0.1, max_time=1.0, max_steps=3, adapt=0, adapt_rtol=1e-3, adapt_atol=1e-3, dt_min=0.0,
             dt_max=1.0, max_rejections=5, resume=0)
    d.update(kw)
    d["newton"] = P.IGXNewtonSpec(*[nd[f[0]] for f in P.IGXNewtonSpec._fields_])
    spec = P.IGXTimeStepSpec(*[d[f[0]] for f in P.IGXTimeStepSpec._fields_])
    info = P.IGXTimeStepInfo()
    rc = P.lib().IGXTimeStep(g.h, C.byref(spec), None, None, C.byref(info), None, 0)
    return rc, P.lib().IGXGetLastError().decode()


def test_refusals_decided_before_any_hip_call():
    import petiga_amd as P
    g = _box()
    g.set_form("bratu", (3.5,))
    nan, inf = float("nan"), float("inf")
    out_of_range = [(dict(alpha_m=0.0), "alpha_m"), (dict(alpha_m=-1.0), "alpha_m"), (dict(alpha_m=nan), "alpha_m"), (dict(alpha_m=inf), "alpha_m"),
                    (dict(alpha_f=0.0), "alpha_f"), (dict(alpha_f=nan), "alpha_f"), (dict(alpha_f=inf), "alpha_f"),
                    (dict(gamma=0.0), "gamma"), (dict(gamma=-0.5), "gamma"), (dict(gamma=nan), "gamma"), (dict(gamma=inf), "gamma"),
                    (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=nan), "dt"), (dict(t0=2.0), "max_time"), (dict(max_time=-1.0), "max_time"),
                    (dict(max_steps=-1), "max_steps"), (dict(max_rejections=-1), "max_rejections"),
                    (dict(adapt_rtol=-1e-3), "adapt_rtol"), (dict(adapt_rtol=nan), "adapt_rtol"), (dict(adapt_atol=-1e-3), "adapt_atol"), (dict(adapt_atol=nan), "adapt_atol"),
                    (dict(dt_min=-1.0), "dt_min"), (dict(dt_min=nan), "dt_min"), (dict(dt_max=-1.0), "dt_max"), (dict(dt_max=nan), "dt_max"),
                    (dict(dt_min=0.5, dt_max=0.25), "dt_max"), (dict(adapt=1, adapt_rtol=0.0, adapt_atol=0.0), "adapt")]
    for kw, word in out_of_range:
        rc, why = _rc(g, **kw)
        assert rc == 63 and "IGXTimeStep" in why and word in why, (kw, rc, why)
    for op in (0, 1, 3, -1):
        rc, why = _rc(g, newton=dict(op=op))
        assert rc == 63 and "IGXTimeStep" in why and "newton.op" in why, (op, rc, why)
    assert _rc(g, adapt=0, adapt_rtol=0.0, adapt_atol=0.0)[0] == 62      # both tolerances 0 without adapt: in range
    # what IGXSolveNonlinear refuses in the spec it is handed, with its reason under the stepper's name
    for kw, word in ((dict(method=2), "method"), (dict(method=-1), "method"), (dict(pc=4), "preconditioner"), (dict(linesearch=2), "line search"), (dict(forcing=-1), "forcing"),
                     (dict(rtol=-1e-8), "tolerance"), (dict(lin_rtol=nan), "tolerance"), (dict(maxit=-1), "maxit"), (dict(max_backtracks=-1), "max_backtracks")):
        rc, why = _rc(g, newton=kw)
        assert rc == 63 and "IGXTimeStep" in why and "IGXSolveNonlinear" in why and word in why, (kw, rc, why)
    rc, why = _rc(g)
    assert rc == 62 and "null" in why, (rc, why)                  # in range: now U and V are looked at
    assert P.lib().IGXTimeStep(g.h, None, None, None, None, None, 0) == 62
    rc, why = _rc(g, newton=dict(pc=3))
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
    rc, why = _rc(g)
    assert rc == 56 and "time stepper" in why and "rank" in why, (rc, why)
    with pytest.raises(P.IGXError) as e:
        g.time_step(None, None, 0.1)
    assert e.value.code == 56 and "time stepper" in str(e.value)


def test_radius_parametrisation():
    import petiga_amd as P
    for rho, want in ((0.0, (1.5, 1.0, 1.0)), (0.5, (5.0 / 6.0, 2.0 / 3.0, 2.0 / 3.0)), (1.0, (0.5, 0.5, 0.5))):
        got = P.alpha_scheme(rho_inf=rho)
        assert got == T.alphas(rho), (rho, got)
        assert np.allclose(got, want, rtol=4e-16, atol=0.0), (rho, got, want)      # (the three are one or two roundings from the fractions)
        am, af, g = got
        assert g == 0.5 + am - af                                            # second order
        assert am >= af >= 0.5                                               # unconditionally stable
    assert P.alpha_scheme(scheme="backward_euler") == T.BACKWARD_EULER == (1.0, 1.0, 1.0)
    assert P.alpha_scheme(alpha=(0.9, 0.8, 0.7)) == (0.9, 0.8, 0.7)
    assert P.alpha_scheme() == T.alphas(0.5)                                 # the reference demos' radius
    with pytest.raises(ValueError):
        P.alpha_scheme(rho_inf=0.5, scheme="backward_euler")


def test_backward_euler_identities():
    """(1, 1, 1): a = 1/h, W = -U0/h, U1 = x, V1 = (U1 - U0)/h, entry by entry"""
    rng = np.random.default_rng(7)
    U0, V0, x = rng.standard_normal(101), rng.standard_normal(101), rng.standard_normal(101)
    for h in (0.1, 1e-10, 3.0):
        a, W, guess = T.stage(T.BACKWARD_EULER, h, U0, V0)
        assert a == 1.0 / h and np.array_equal(W, -(a * U0)) and np.array_equal(guess, U0)
        # a U0 against U0 / h: the same number up to the rounding of 1 / h (exact for a power of two)
        assert np.allclose(W, -U0 / h, rtol=4e-16, atol=0.0)
        U1, V1 = T.update(T.BACKWARD_EULER, h, x, U0, V0)
        assert np.array_equal(U1, U0 + (x - U0)) and np.allclose(U1, x, rtol=0.0, atol=4e-16 * np.abs(U0).max())
        assert np.array_equal(V1, (1.0 / h) * (U1 - U0)) and np.allclose(V1, (U1 - U0) / h, rtol=4e-16, atol=0.0)
    a, W, _ = T.stage(T.BACKWARD_EULER, 0.25, U0, V0)
    assert a == 4.0 and np.array_equal(W, -U0 / 0.25)                       # a power of two: exact
    U1, V1 = T.update(T.BACKWARD_EULER, 0.25, U0 + 0.5, U0, V0)
    assert np.array_equal(V1, (U1 - U0) / 0.25)


# ---- the restatement on a linear problem with a known solution
@functools.lru_cache(maxsize=None)
def _linear():
    """M, K of the p = 2 (3,3,3) box without Dirichlet faces, u0 smooth, V0 = -M^-1 K u0, and exact(t) from K Phi = M Phi Lambda"""
    import scipy.linalg as sl
    import scipy.sparse.linalg as spla
    orc, _ = make_pair(3, 1, 2, [3, 3, 3], engine=False)
    M = orc.compute_system("orc_form_mass")[0].scipy().tocsc()
    K = orc.compute_system("orc_form_poisson")[0].scipy().tocsc()
    lam, Phi = sl.eigh(K.toarray(), M.toarray())
    g = [greville(orc.axis(i)["U"], 2) for i in range(3)]
    X, Y, Z = np.meshgrid(g[0], g[1], g[2], indexing="ij")
    u0 = (1 + np.cos(np.pi * X) * np.cos(np.pi * Y) + 0.5 * np.cos(np.pi * Z)).transpose(2, 1, 0).ravel()
    c = Phi.T @ (M @ u0)
    V0 = -spla.spsolve(M, K @ u0)
    for a in (u0, V0):
        a.setflags(write=False)
    return M, K, u0, V0, (lambda t: Phi @ (np.exp(-lam * t) * c))


def _linear_newton(fails=lambda a: False, seen=None):
    """the stage solve of M V + K U = 0 at V = a x + W: (a M + K) x = -M W, by a sparse LU kept per shift"""
    import scipy.sparse.linalg as spla
    M, K = _linear()[:2]
    lu = {}

    def newton(a, t, W, x0):
        if seen is not None:
            seen.append((a, t))
        if fails(a):
            return x0.copy(), dict(NEWTON_FAILED)
        if a not in lu:
            lu[a] = spla.splu((a * M + K).tocsc())
        return lu[a].solve(-(M @ W)), dict(NEWTON_OK)
    return newton


# T = 0.1 in 8 and in 16 steps: the ratios the restatement shows there are 4.01 (rho 0.5), 4.01 (rho 1) and 1.96 (backward Euler);
# at 4 against 8 steps they are still 5.4, 5.0 and 1.92 (h lambda_max = 18: the stiff modes are not resolved)
@pytest.mark.parametrize("scheme,lo,hi", [(0.5, 3.5, 4.5), (1.0, 3.5, 4.5), ("backward_euler", 1.7, 2.3)])
def test_order_on_the_linear_problem(scheme, lo, hi):
    M, K, u0, V0, exact = _linear()
    alpha = T.BACKWARD_EULER if scheme == "backward_euler" else T.alphas(scheme)
    errs = []
    for steps in (8, 16):
        U, V, info = T.integrate(_linear_newton(), u0, V0, 0.1 / steps, max_time=0.1, max_steps=1000, alpha=alpha)
        assert info["reason"] == T.CONVERGED_TIME and info["t"] == 0.1 and info["steps"] == steps
        errs.append(np.abs(U - exact(0.1)).max())
        # V is the derivative of the same solution (seen: off by 0.11 of max|V_0| = 51 at 8 steps: the last step is a whole one, not a
        # remainder of rounding size, which would divide rounding noise by h)
        dV = np.abs(V - (exact(0.1 + 1e-6) - exact(0.1 - 1e-6)) / 2e-6).max()
        print("  %d steps: max|V - exact'| = %.3e" % (steps, dV))
        assert dV <= 0.05 * np.abs(V0).max()
    print("%s: max|U - exact| = %.3e, %.3e, ratio %.3f" % (scheme, errs[0], errs[1], errs[0] / errs[1]))
    assert lo < errs[0] / errs[1] < hi


# On this problem u'' only decays and the estimate is h^2 u'' / 2 whatever the step before was, so a step grown by fac = 0.9 / sqrt(wlte)
# lands on wlte = 0.81 and is never rejected: the run from dt0 = 1e-6 grows (by the cap of 10, then with the decay) without a rejection.
# The estimate does reject a first step that is too long for the tolerance, as soon as it exists: dt0 = 5e-3 at tolerances 1e-4 is
# rejected at the second step, cut by fac and grows from there as the solution decays (what is seen is in the test's output).
GROWING = dict(dt=1e-6, max_time=0.3, max_steps=200, adapt=True, adapt_rtol=1e-4, adapt_atol=1e-4, max_rejections=5)
REJECTING = dict(dt=5e-3, max_time=0.3, max_steps=2000, adapt=True, adapt_rtol=1e-4, adapt_atol=1e-4, max_rejections=5)


def test_adaptive_run_grows_and_rejects():
    M, K, u0, V0, exact = _linear()
    U, V, info = T.integrate(_linear_newton(), u0, V0, alpha=T.alphas(0.5), **GROWING)
    log = info["log"]
    dts = [r["dt"] for r in log if r["accepted"]]
    print("growing: %d steps, %d rejections, dt %s" % (info["steps"], info["rejections"], ["%.2e" % d for d in dts]))
    assert info["reason"] == T.CONVERGED_TIME and info["t"] == GROWING["max_time"]
    assert log[0]["wlte"] == -1.0 and log[0]["accepted"] == 1 and dts[1] == dts[0]      # no estimate on the first step: h unchanged
    assert dts[2] == 10.0 * dts[1] and dts[3] == 10.0 * dts[2]                            # growth starts from the second step, at the cap
    assert max(dts) > 1e3 * dts[0]
    assert info["attempts"] == len(log) == info["steps"] + info["rejections"]
    assert all(0.0 <= r["wlte"] <= 1.0 for r in log[1:] if r["accepted"])
    assert np.abs(U - exact(info["t"])).max() <= 1e-2 * np.abs(u0).max()
    # another order of the sum changes wlte by rounding alone
    U2, V2, info2 = T.integrate(_linear_newton(), u0, V0, alpha=T.alphas(0.5), summed=lambda q: np.sum(q[::-1]), **GROWING)
    assert [r["accepted"] for r in info2["log"]] == [r["accepted"] for r in log]
    assert info2["log"][1]["wlte"] != -1.0 and abs(info2["log"][1]["wlte"] - log[1]["wlte"]) <= 125 * 2.0 ** -53 * log[1]["wlte"]      # (the same vectors up to here)

    U, V, info = T.integrate(_linear_newton(), u0, V0, alpha=T.alphas(0.5), **REJECTING)
    log = info["log"]
    rejected = [r for r in log if not r["accepted"]]
    dts = [r["dt"] for r in log if r["accepted"]]
    print("rejecting: %d steps, %d rejections, the first attempts (dt, wlte, accepted) %s, the last dt %.3e"
          % (info["steps"], info["rejections"], [("%.2e" % r["dt"], "%.3g" % r["wlte"], r["accepted"]) for r in log[:4]], dts[-2]))
    assert info["reason"] == T.CONVERGED_TIME and info["t"] == REJECTING["max_time"]
    assert info["rejections"] == len(rejected) >= 1 and all(r["wlte"] > 1.0 for r in rejected) and info["attempts"] == info["steps"] + info["rejections"]
    assert log[1] is rejected[0]
    for a, b in zip(log[:-1], log[1:]):
        if not a["accepted"]:
            assert b["dt"] == T.factor(a["wlte"]) * a["dt"] and b["t"] == a["t"]
    assert dts[-2] > 3 * dts[1]                                                             # the step grows again as u'' decays
    assert np.abs(U - exact(info["t"])).max() <= 1e-4 * np.abs(u0).max()
    # the restatement fed its own wlte takes the same decisions and gives the same bits
    U3, V3, info3 = T.integrate(_linear_newton(), u0, V0, alpha=T.alphas(0.5), device_wlte=[r["wlte"] for r in log], **REJECTING)
    assert np.array_equal(U3, U) and np.array_equal(V3, V) and [r["dt"] for r in info3["log"]] == [r["dt"] for r in log]
    assert all(r["host_wlte"] == r["wlte"] for r in info3["log"])


def test_failed_stage_quarters_the_step():
    M, K, u0, V0, exact = _linear()
    alpha = T.alphas(0.5)
    a_of = lambda h: alpha[0] / (alpha[1] * alpha[2] * h)
    fails = lambda a: a < a_of(0.003)                # every stage with h > 0.003 fails
    U, V, info = T.integrate(_linear_newton(fails), u0, V0, 0.04, max_steps=1, alpha=alpha, adapt=True, max_rejections=5)
    print("failed stage:", [(r["dt"], r["accepted"], r["newton_reason"]) for r in info["log"]])
    assert [r["dt"] for r in info["log"]] == [0.04, 0.01, 0.0025] and [r["accepted"] for r in info["log"]] == [0, 0, 1]
    assert info["rejections"] == 2 and info["steps"] == 1 and info["reason"] == T.CONVERGED_STEPS and info["t"] == 0.0025 and info["dt_next"] == 0.0025
    assert all(r["wlte"] == -1.0 for r in info["log"])
    # without adapt: the failure ends the run with the entry state
    U, V, info = T.integrate(_linear_newton(fails), u0, V0, 0.04, max_steps=1, alpha=alpha)
    assert info["reason"] == T.DIVERGED_NONLINEAR_SOLVE and info["steps"] == 0 and np.array_equal(U, u0) and np.array_equal(V, V0) and info["t"] == 0.0
    # the limits: max_rejections, then dt_min
    U, V, info = T.integrate(_linear_newton(fails), u0, V0, 0.04, max_steps=1, alpha=alpha, adapt=True, max_rejections=1)
    assert info["reason"] == T.DIVERGED_NONLINEAR_SOLVE and info["attempts"] == 2 and info["rejections"] == 2 and np.array_equal(U, u0)
    U, V, info = T.integrate(_linear_newton(fails), u0, V0, 0.04, max_steps=1, alpha=alpha, adapt=True, max_rejections=5, dt_min=0.02)
    assert info["reason"] == T.DIVERGED_NONLINEAR_SOLVE and info["attempts"] == 1 and np.array_equal(U, u0)
    # an estimate that never passes: IGX_TS_DIVERGED_STEP_REJECTED by either limit, with the first (estimate-free) step kept
    tight = dict(alpha=alpha, adapt=True, adapt_rtol=1e-14, adapt_atol=1e-14, max_steps=2)
    U, V, info = T.integrate(_linear_newton(), u0, V0, 0.01, max_rejections=2, **tight)
    assert info["reason"] == T.DIVERGED_STEP_REJECTED and info["steps"] == 1 and info["rejections"] == 3 and info["attempts"] == 4 and info["t"] == 0.01
    U1, V1, one = T.integrate(_linear_newton(), u0, V0, 0.01, max_steps=1, alpha=alpha)
    assert np.array_equal(U, U1) and np.array_equal(V, V1)
    U, V, info = T.integrate(_linear_newton(), u0, V0, 0.01, max_rejections=50, dt_min=2e-4, **tight)
    assert info["reason"] == T.DIVERGED_STEP_REJECTED and info["steps"] == 1 and info["rejections"] == 2 and np.array_equal(U, U1)


def test_last_step_is_shortened_to_max_time():
    M, K, u0, V0, exact = _linear()
    seen = []
    U, V, info = T.integrate(_linear_newton(seen=seen), u0, V0, 0.03, max_time=0.1, max_steps=50, alpha=T.alphas(0.5), dt_min=0.02)
    dts = [r["dt"] for r in info["log"]]
    print("shortened: dt %s, t %.17g, dt_next %.17g" % (dts, info["t"], info["dt_next"]))
    assert info["reason"] == T.CONVERGED_TIME and info["t"] == 0.1 and info["steps"] == 4
    assert dts[:3] == [0.03, 0.03, 0.03] and dts[3] == 0.1 - (0.03 + 0.03 + 0.03) and dts[3] < 0.02      # exempt from dt_min
    assert info["dt_last"] == dts[3] and info["dt_next"] == 0.03                                            # the step proposed before the shortening
    af = T.alphas(0.5)[1]
    assert seen[3][1] == (0.03 + 0.03 + 0.03) + af * dts[3]
    assert np.abs(U - exact(0.1)).max() <= 2e-2      # (seen: 9.9e-3 at h = 0.03)
    # max_steps = 0 and t0 == max_time: nothing is done
    for kw, reason in ((dict(max_steps=0), T.CONVERGED_STEPS), (dict(max_steps=3, t0=0.1, max_time=0.1), T.CONVERGED_TIME)):
        U, V, info = T.integrate(None, u0, V0, 0.03, **kw)
        assert info["reason"] == reason and info["steps"] == 0 and info["attempts"] == 0 and np.array_equal(U, u0) and info["dt_next"] == 0.03


def test_resume_equals_one_long_run():
    M, K, u0, V0, exact = _linear()
    kw = dict(alpha=T.alphas(0.5), adapt=True, adapt_rtol=1e-3, adapt_atol=1e-3, max_rejections=5)
    U6, V6, six = T.integrate(_linear_newton(), u0, V0, 1e-4, max_steps=6, **kw)
    Ua, Va, a = T.integrate(_linear_newton(), u0, V0, 1e-4, max_steps=3, **kw)
    Ub, Vb, b = T.integrate(_linear_newton(), Ua, Va, a["dt_next"], max_steps=3, t0=a["t"], prev=a["prev"], **kw)
    print("resume: dt of six %s; of 3 + 3 %s" % ([r["dt"] for r in six["log"]], [r["dt"] for r in a["log"] + b["log"]]))
    assert six["steps"] == 6 and a["steps"] == b["steps"] == 3
    assert np.array_equal(U6, Ub) and np.array_equal(V6, Vb) and b["t"] == six["t"] and b["dt_next"] == six["dt_next"]
    strip = lambda log: [tuple(sorted(r.items())) for r in log]
    assert strip(a["log"] + b["log"]) == strip(six["log"])
    assert b["log"][0]["wlte"] >= 0.0                       # the estimate is available at once
    # without the kept U_{n-1} the second call starts estimate-free and takes other steps
    Uc, Vc, c = T.integrate(_linear_newton(), Ua, Va, a["dt_next"], max_steps=3, t0=a["t"], **kw)
    assert c["log"][0]["wlte"] == -1.0 and not np.array_equal(Uc, U6)


# ---- Bratu as an IFunction on the oracle, through tests/newton_ref.py
def test_bratu_ifunction_two_steps_on_the_oracle():
    orc, _ = make_pair(3, 1, 2, [3, 3, 3], engine=False)
    for bc in BRATU_BCS:
        orc.set_boundary_value(*bc)
    lam = C.c_double(3.5)
    n = orc.global_size()
    # U_0: the Dirichlet values on the faces (taken from a converged steady state), a bump inside; V_0 = 0 on the fixed rows
    fun, lin = N.oracle_callables(orc, "orc_form_bratu_function", "orc_form_bratu_jacobian", lam)
    steady, sinfo = N.newton(fun, lin, np.zeros(n), rtol=1e-12, maxit=20)
    assert sinfo["reason"] == N.CONVERGED_FNORM_RELATIVE
    J = orc.compute_jacobian("orc_form_bratu_jacobian", lam, steady).scipy().tocsr()
    off = abs(J)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    U0 = np.where(fixed, steady, steady + 0.2)
    V0 = np.zeros(n)
    h = 0.01
    newton = T.oracle_callables(orc, "orc_form_bratu_ifunction", "orc_form_bratu_ijacobian", lam, rtol=1e-12, maxit=20)
    for alpha in (T.alphas(0.5), T.BACKWARD_EULER):
        U, V, info = T.integrate(newton, U0, V0, h, max_steps=2, alpha=alpha)
        print("Bratu IFunction, alpha %s: %d steps, newton %d iterations, |U - steady| %.3e -> %.3e" % (alpha, info["steps"], info["newton_iterations"],
              np.abs(U0 - steady).max(), np.abs(U - steady).max()))
        assert info["reason"] == T.CONVERGED_STEPS and info["steps"] == 2 and info["t"] == h + h
        assert all(r["newton_reason"] > 0 for r in info["log"]) and info["newton_iterations"] == sum(r["newton_iterations"] for r in info["log"])
        assert np.array_equal(U[fixed], U0[fixed])                                   # the residual pins the stage: the faces stay
        # the scheme's own equation at the second stage, from (U, V) after one step and after two: with U_af = U_1 + af (U_2 - U_1) and
        # V_am = V_1 + am (V_2 - V_1), IFunction(a, V_am, t_1 + af h, U_af) = 0 to Newton's tolerance -- the identity the header states
        Ua, Va, one = T.integrate(newton, U0, V0, h, max_steps=1, alpha=alpha)
        am, af, g = alpha
        a = am / (af * g * h)
        F = orc.compute_ifunction("orc_form_bratu_ifunction", lam, a, Va + am * (V - Va), one["t"] + af * h, Ua + af * (U - Ua))
        F0 = orc.compute_ifunction("orc_form_bratu_ifunction", lam, a, V0, 0.0, U0)
        print("   |F(stage 2)| / |F(U_0, V_0)| = %.3e" % (np.linalg.norm(F) / np.linalg.norm(F0)))
        assert np.linalg.norm(F) <= 1e-9 * np.linalg.norm(F0)
