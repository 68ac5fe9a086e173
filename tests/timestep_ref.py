"""A numpy restatement of the loop of IGXTimeStep (include/petiga_amd.h), written from the header's statement: integrate(newton, U, V, dt,
...) takes the stage solve as a callable, so the same loop runs on the engine's own Newton solve (engine_callables: one host copy each way
per stage, the device's IGXSolveNonlinear as the stage solve), on the CPU oracle through tests/newton_ref.py (oracle_callables) or on
anything else (a sparse direct solve of a linear problem).
  newton(a, t, W, x0) -> (x, info)      G(x) = IFunction(a, a x + W, t, x) = 0 from x0; info: reason (< 0: failed), iterations,
                                        linear_iterations, function_evaluations (IGXNewtonInfo's)
A rounded product followed by a rounded sum is what numpy does on separate arrays, so every line below rounds as the sweeps of
petiga_amd/csrc/timestep.hpp do.  wlte comes from an exactly rounded sum (math.fsum); summed= takes another order.
integrate returns (U, V, info): info holds the fields of IGXTimeStepInfo, log (one dict per attempt, IGXTimeStepLog's members and
host_wlte), and prev = (U_{n-1}, h_{n-1}), what resume continues from (pass it back as prev=)."""
import math

import numpy as np

CONVERGED_TIME, CONVERGED_STEPS = 1, 2
DIVERGED_NONLINEAR_SOLVE, DIVERGED_STEP_REJECTED, DIVERGED_NAN = -1, -2, -3
BACKWARD_EULER = (1.0, 1.0, 1.0)


def alphas(rho):
    """the radius parametrisation of the reference's demos"""
    am, af = (3.0 - rho) / (2.0 * (1.0 + rho)), 1.0 / (1.0 + rho)
    return am, af, 0.5 + am - af


def stage(alpha, h, U0, V0):
    """(a, W, x): the shift, W = c0 V0 - a U0 and the stage guess"""
    am, af, g = alpha
    a, c0 = am / (af * g * h), 1.0 - am / g
    return a, c0 * V0 - a * U0, U0.copy()


def update(alpha, h, x, U0, V0):
    """(U1, V1) from the stage solution"""
    am, af, g = alpha
    c1, c2, c3 = 1.0 / af, 1.0 / (g * h), 1.0 - 1.0 / g
    U1 = U0 + c1 * (x - U0)
    V1 = c2 * (U1 - U0) + c3 * V0
    return U1, V1


def error_terms(h, hprev, U1, U0, Uprev, atol, rtol):
    """q_i = e_i / (atol + rtol max(|U1_i|, |U1_i + e_i|)), e the backward-difference estimate on unequal steps"""
    r = 1.0 + hprev / h
    d1, d2, d3 = r, r - 1.0, r * (r - 1.0)
    e = (U1 / d1 - U0 / d2) + Uprev / d3
    return e / (atol + rtol * np.maximum(np.abs(U1), np.abs(U1 + e)))


def wlte_of(q, summed=None):
    q2 = q * q
    s = math.fsum(q2) if summed is None else float(summed(q2))
    return math.sqrt(s / q.size)


def factor(wlte):
    return 10.0 if wlte == 0.0 else min(10.0, max(0.1, 0.9 / math.sqrt(wlte)))


def integrate(newton, U, V, dt, max_time=float("inf"), max_steps=1, alpha=BACKWARD_EULER, t0=0.0, adapt=False, adapt_rtol=1e-3, adapt_atol=1e-3, dt_min=0.0,
              dt_max=float("inf"), max_rejections=10, prev=None, summed=None, device_wlte=None):
    """device_wlte: the device's logged wlte of every attempt.  The restatement then forms its own (host_wlte in the log) but takes fac, the
    next step and the decision from the device's value with the same host formula, so the dt sequence stays the device's."""
    U0, V0 = np.array(U, dtype=float), np.array(V, dtype=float)
    Uprev, hprev = (None, 0.0) if prev is None else (np.array(prev[0], dtype=float), float(prev[1]))
    t, h = float(t0), float(dt)
    info = dict(steps=0, reason=0, rejections=0, attempts=0, newton_iterations=0, linear_iterations=0, function_evaluations=0, t=t, dt_last=0.0, dt_next=h, unorm=0.0)
    log = []
    reason = 0
    if max_steps == 0:
        reason = CONVERGED_STEPS
    elif t == max_time:
        reason = CONVERGED_TIME
    while not reason:
        rejections = 0
        while True:      # the attempts of one step
            p = h
            left = max_time - t
            shortened = left <= (1.0 + 1e-9) * h
            if shortened:
                h = left
            a, W, x0 = stage(alpha, h, U0, V0)
            x, ni = newton(a, t + alpha[1] * h, W, x0)
            for key in ("newton_iterations", "linear_iterations", "function_evaluations"):
                info[key] += ni["iterations" if key == "newton_iterations" else key]
            rec = dict(t=t, dt=h, wlte=-1.0, host_wlte=-1.0, accepted=0, newton_iterations=ni["iterations"], newton_reason=ni["reason"], linear_iterations=ni["linear_iterations"])
            log.append(rec)
            info["attempts"] += 1
            if ni["reason"] < 0:      # a failed attempt
                if not adapt:
                    reason = DIVERGED_NONLINEAR_SOLVE
                    break
                rejections += 1
                info["rejections"] += 1
                h = h / 4
                if rejections > max_rejections or h < dt_min:
                    reason = DIVERGED_NONLINEAR_SOLVE
                    break
                continue
            U1, V1 = update(alpha, h, x, U0, V0)
            estimate = bool(adapt) and Uprev is not None
            unorm = math.sqrt(float(np.dot(U1, U1)))
            wlte = -1.0
            if estimate:
                with np.errstate(all="ignore"):
                    wlte = rec["host_wlte"] = wlte_of(error_terms(h, hprev, U1, U0, Uprev, adapt_atol, adapt_rtol), summed)
                if device_wlte is not None:
                    wlte = float(device_wlte[info["attempts"] - 1])
            rec["wlte"] = wlte
            if math.isnan(unorm) or math.isnan(wlte):
                reason = DIVERGED_NAN
                break
            nxt = p
            if estimate:
                fac = factor(wlte)
                if not wlte <= 1.0:      # rejected by the estimate
                    rejections += 1
                    info["rejections"] += 1
                    h = fac * h
                    if rejections > max_rejections or h < dt_min:
                        reason = DIVERGED_STEP_REJECTED
                        break
                    continue
                if not shortened:
                    nxt = min(dt_max, max(dt_min, fac * h))
            rec["accepted"] = 1
            Uprev, U0, V0, hprev = U0, U1, V1, h
            t = max_time if shortened else t + h
            info["steps"] += 1
            info["dt_last"], info["unorm"] = h, unorm
            h = nxt
            if t == max_time:
                reason = CONVERGED_TIME
            elif info["steps"] == max_steps:
                reason = CONVERGED_STEPS
            break
    info.update(reason=reason, t=t, dt_next=h, log=log, prev=None if Uprev is None else (Uprev, hprev))
    return U0, V0, info


def engine_callables(eng, **newton_kw):
    """newton(a, t, W, x0) through the engine's own IGXSolveNonlinear (eng.solve_nonlinear, op = "ijacobian"): one host copy each way per stage"""
    Xv, Wv = eng.create_vec(), eng.create_vec()

    def newton(a, t, W, x0):
        Xv.set(x0)
        Wv.set(W)
        info = eng.solve_nonlinear(Xv, op="ijacobian", W=Wv, a=a, t=t, **newton_kw)
        return Xv.get().copy(), info
    return newton


def oracle_callables(orc, function, jacobian, ctx, **newton_kw):
    """newton(a, t, W, x0) on the CPU oracle through tests/newton_ref.py: `function` / `jacobian` name its IFunction / IJacobian forms; the
    linear solve is scipy's sparse direct solve unless iterative= is given (newton_ref.oracle_callables)"""
    import newton_ref as N
    lin_kw = {k: newton_kw.pop(k) for k in ("iterative", "jacobi", "lin_maxit") if k in newton_kw}

    def newton(a, t, W, x0):
        fun, lin = N.oracle_callables(orc, function, jacobian, ctx, op="ijacobian", a=a, t=t, W=W, **lin_kw)
        return N.newton(fun, lin, x0, **newton_kw)
    return newton
