"""A numpy restatement of the loop of IGXSolveNonlinear (include/petiga_amd.h), written from the header's statement: newton(fun, linsolve,
x0, ...) takes the residual and the linear solve as callables, so the same loop runs on the engine's own operators (engine_callables: one
host copy each way per call, the device's IGXSolve as the linear solve), on the CPU oracle with scipy's sparse direct solve
(oracle_callables) or with a numpy Krylov loop of tests/krylov_ref.py (oracle_callables(..., iterative=...)).
  fun(x)               -> F
  linsolve(x, F, eta)  -> (d, iterations, reason)      J(x) d = F from d = 0 to the relative tolerance eta; reason: krylov_ref's numbers
newton returns (x, info): info holds the fields of IGXNewtonInfo, history, linear_its, etas, lambdas (per iteration, every lambda tried)
and iterates (every accepted x)."""
import numpy as np

import krylov_ref as K

CONVERGED_FNORM_ABS, CONVERGED_FNORM_RELATIVE, CONVERGED_SNORM_RELATIVE = 2, 3, 4
DIVERGED_LINEAR_SOLVE, DIVERGED_FNORM_NAN, DIVERGED_MAX_IT, DIVERGED_LINE_SEARCH = -3, -4, -5, -6


def state_of(a, x, W):
    """V = a x + W: the rounded product plus W"""
    return a * x + W


def _norm(v):
    return float(np.sqrt(np.dot(v, v)))


def newton(fun, linsolve, x0, rtol=1e-8, atol=0.0, stol=0.0, maxit=50, lin_rtol=1e-5, forcing="constant", linesearch="basic", max_backtracks=10):
    x = np.array(x0, dtype=float)
    F = fun(x)
    f = fnorm0 = _norm(F)
    hist, lin_its, etas, lambdas, iterates = [f], [], [], [], []
    evals = 1
    its = backtracks = last_lin = 0
    snorm = xnorm = 0.0
    reason = 0
    if np.isnan(f):
        reason = DIVERGED_FNORM_NAN
    elif f <= atol:
        reason = CONVERGED_FNORM_ABS
    elif maxit == 0:
        reason = DIVERGED_MAX_IT
    eta, fprev = lin_rtol, 0.0
    while not reason:
        if forcing == "ew2" and its > 0:
            q, floor = f / fprev, 0.9 * (eta * eta)
            e = 0.9 * (q * q)
            if floor > 0.1 and e < floor:
                e = floor
            eta = 0.9 if e > 0.9 else e
        etas.append(eta)
        d, k, last_lin = linsolve(x, F, eta)
        lin_its.append(k)
        if last_lin in (K.DIVERGED_BREAKDOWN, K.DIVERGED_NAN):
            reason = DIVERGED_LINEAR_SOLVE
            break
        lam, halvings, accepted, tried = 1.0, 0, False, []
        while True:
            xt = x - lam * d
            Ft = fun(xt)
            evals += 1
            ft = _norm(Ft)
            tried.append(lam)
            if linesearch == "basic":
                if np.isnan(ft):
                    reason = DIVERGED_FNORM_NAN
                else:
                    accepted = True
            elif np.isfinite(ft) and ft <= (1.0 - 1e-4 * lam) * f:
                accepted = True
            elif halvings == max_backtracks:
                reason = DIVERGED_LINE_SEARCH
            if accepted or reason:
                break
            lam *= 0.5
            halvings += 1
            backtracks += 1
        lambdas.append(tried)
        if not accepted:
            break
        snorm, xnorm = lam * _norm(d), _norm(xt)
        x, F, fprev, f = xt, Ft, f, ft
        its += 1
        hist.append(f)
        iterates.append(x.copy())
        if np.isnan(f):
            reason = DIVERGED_FNORM_NAN
        elif f <= atol:
            reason = CONVERGED_FNORM_ABS
        elif f <= rtol * fnorm0:
            reason = CONVERGED_FNORM_RELATIVE
        elif snorm <= stol * xnorm:
            reason = CONVERGED_SNORM_RELATIVE
        elif its >= maxit:
            reason = DIVERGED_MAX_IT
    return x, dict(iterations=its, reason=reason, linear_iterations=int(sum(lin_its)), function_evaluations=evals, backtracks=backtracks, last_linear_reason=last_lin,
                   fnorm0=fnorm0, fnorm=f, snorm=snorm, xnorm=xnorm, history=np.array(hist), linear_its=np.array(lin_its, dtype=int), etas=etas, lambdas=lambdas,
                   iterates=iterates)


def engine_callables(eng, op="jacobian", a=0.0, t=0.0, W=None, method="bicgstab", pc="none", lin_atol=0.0, lin_maxit=1000, directions=None):
    """(fun, linsolve) on the host from the engine's own calls: compute_function / compute_ifunction at V = a x + W formed here, and
    solve() from a zeroed guess.  `directions`, a list, receives every d."""
    Xv, Vv, Fv, Bv, Dv = (eng.create_vec() for _ in range(5))
    W = None if W is None else np.array(W, dtype=float)

    def put(x):
        Xv.set(x)
        if op == "ijacobian":
            Vv.set(state_of(a, x, W))

    def fun(x):
        put(x)
        if op == "jacobian":
            eng.compute_function(Xv, Fv)
        else:
            eng.compute_ifunction(a, Vv, t, Xv, Fv)
        eng.synchronize()
        return Fv.get().copy()

    def linsolve(x, F, eta):
        put(x)
        Bv.set(F)
        Dv.fill(0.0)
        state = dict(U=Xv) if op == "jacobian" else dict(a=a, t=t, V=Vv, U=Xv)
        info = eng.solve(Bv, Dv, method=method, op=op, pc=pc, rtol=eta, atol=lin_atol, maxit=lin_maxit, **state)
        d = Dv.get().copy()
        if directions is not None:
            directions.append(d)
        return d, info["iterations"], info["reason"]

    return fun, linsolve


def oracle_callables(orc, function, jacobian, ctx, op="jacobian", a=0.0, t=0.0, W=None, iterative=None, jacobi=True, lin_maxit=2000):
    """(fun, linsolve) on the CPU oracle: `function` / `jacobian` are its form names (the IFunction pair for op = "ijacobian", at
    V = a x + W).  The linear solve is scipy's sparse direct solve, or with iterative = "cg" / "bicgstab" the loop of tests/krylov_ref.py
    with the Jacobi preconditioner (jacobi=False: none) to eta."""
    import scipy.sparse.linalg as spla

    def fun(x):
        if op == "jacobian":
            return orc.compute_function(function, ctx, x)
        return orc.compute_ifunction(function, ctx, a, state_of(a, x, W), t, x)

    def matrix(x):
        if op == "jacobian":
            return orc.compute_jacobian(jacobian, ctx, x).scipy()
        return orc.compute_ijacobian(jacobian, ctx, a, state_of(a, x, W), t, x).scipy()

    def linsolve(x, F, eta):
        J = matrix(x)
        if iterative is None:
            return spla.spsolve(J.tocsc(), F), 1, K.CONVERGED_RTOL
        J = J.tocsr()
        D = J.diagonal()
        loop = K.cg if iterative == "cg" else K.bicgstab
        d, info = loop(lambda v: J @ v, (lambda v: v / D) if jacobi else (lambda v: v.copy()), F, rtol=eta, maxit=lin_maxit)
        return d, info["iterations"], info["reason"]

    return fun, linsolve
