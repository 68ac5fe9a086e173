"""Times IGXTimeStep next to the Newton solves it calls and next to the same steps driven from Python, in one process (profiles/timestep.txt):
  Cahn-Hilliard p = 2 (bench.py's config 4 parameters) at 64^3 and 128^3 elements, 5 fixed generalized-alpha steps (rho_inf = 0.5) from a
  random state near the mean concentration with V_0 = 0; BiCGStab without a preconditioner, a bounded amount of work per stage (--maxit
  Newton iterations, --lin-maxit inner iterations at the most).
Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs.  Per step: the whole call, the operators' own kernel time summed
over the Newton solves, and the rest.  The stepper's own share is measured on a call whose Newton solves accept the stage guess at once
(atol = 1e300: one residual per stage and no linear solve): what is left after that residual's kernel time is the two sweeps, the Newton
solve's three small launches and the two blocking reads of a stage.  The sweeps' floor is written out: 8 n bytes per vector read or
written / the HBM rate, 4 vector streams for ts_stage (U0, V0 in; W, x out) and 6 for ts_update (x, U0, V0 in; U1, V1 out -- 7 with the
estimate's Uprev).  Next to these: the same five steps driven from Python with solve_nonlinear and Vec.axpby, the loop a caller without
the stepper writes (three vector passes for W, x; three for U1, V1; a norm), timed by the host's clock.

    python scripts/time_step.py [--cases 64,128] [--steps 5] [--maxit 3] [--lin-maxit 60] [--hbm-tbs 8.0]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import timed


def host_steps(g, U, V, W, x, U1, h, steps, alpha, newton):
    """the loop a caller writes today: W = c0 V - a U, x = U; solve_nonlinear; U1 = U + c1 (x - U); V = c2 (U1 - U) + c3 V; U = U1; |U|"""
    am, af, gm = alpha
    a, c0, c1, c2, c3 = am / (af * gm * h), 1.0 - am / gm, 1.0 / af, 1.0 / (gm * h), 1.0 - 1.0 / gm
    t = 0.0
    for _ in range(steps):
        W.copy_from(V).scale(c0).axpby(-a, U, 1.0)
        x.copy_from(U)
        g.solve_nonlinear(x, op="ijacobian", W=W, a=a, t=t + af * h, **newton)
        U1.copy_from(x).axpby(1.0 - c1, U, c1)            # U + c1 (x - U), as one pass
        V.scale(c3).axpby(c2, U1, 1.0).axpby(-c2, U, 1.0)
        U.copy_from(U1)
        U.norm()
        t += h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64,128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--maxit", type=int, default=3)
    ap.add_argument("--lin-maxit", type=int, default=60)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate the sweep floor is taken at, TB/s (MI355X data sheet: 8)")
    a = ap.parse_args()
    import petiga_amd as P
    print(P.device_info(), flush=True)
    alpha = P.alpha_scheme(rho_inf=0.5)
    for N in (int(v) for v in a.cases.split(",")):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, 2, N)
        g.setup()
        g.set_form("cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / (3.0 * N * N), 1.0))
        U, V, F = g.create_vec(), g.create_vec(), g.create_vec()
        n = U.n
        U0 = 0.63 + 0.05 * (2 * np.random.default_rng(7).random(n) - 1)
        h = 1e-10      # the first step of the reference demo
        newton = dict(method="bicgstab", pc="none", lin_rtol=1e-4, lin_maxit=a.lin_maxit, rtol=1e-3, maxit=a.maxit)
        print("Cahn-Hilliard p = 2, %d^3 elements, n = %d (%.1f MB per vector), %d steps of h = %g, alpha = (%.4f, %.4f, %.4f)" % ((N, n, 8 * n / 1e6, a.steps, h) + alpha), flush=True)
        t_res = timed(g, lambda: g.compute_ifunction(alpha[0] / (alpha[1] * alpha[2] * h), V.fill(0.0), 0.0, U.set(U0), F))
        print("  IGXComputeIFunction %.3f ms (kernels, median of 10)" % t_res[1], flush=True)

        seen = {}

        def reset():
            U.set(U0)
            V.fill(0.0)

        def run(**kw):
            reset()
            seen["info"] = g.time_step(U, V, h, max_steps=a.steps, alpha=alpha, **kw)

        total, kernel, _, _ = timed(g, lambda: run(**newton))
        info, launches = seen["info"], g.last_timing()[2]
        assert info["steps"] == a.steps, info      # (a stage whose Newton solve fails ends a run with fixed steps)
        print("  IGXTimeStep per step: %.3f ms, operators' own kernels %.3f ms, the rest %.3f ms; %d launches per call; %d steps, reason %s, %d Newton and %d inner iterations; %s"
              % (total / a.steps, kernel / a.steps, (total - kernel) / a.steps, launches, info["steps"], info["reason_name"], info["newton_iterations"], info["linear_iterations"], g.kernel_name()), flush=True)
        wall = []
        for _ in range(10):
            reset()
            g.synchronize()
            t0 = time.perf_counter()
            g.time_step(U, V, h, max_steps=a.steps, alpha=alpha, **newton)
            g.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        wall = statistics.median(wall)
        print("    by the host's clock with timing off: %.3f ms per step" % (wall / a.steps), flush=True)

        empty = dict(newton, atol=1e300)
        total_e, kernel_e, _, _ = timed(g, lambda: run(**empty))
        info_e, launches_e = seen["info"], g.last_timing()[2]
        own = (total_e - kernel_e) / a.steps
        for streams, what in ((4, "ts_stage"), (6, "ts_update"), (7, "ts_update with the estimate")):
            print("    floor of %-28s %d x 8 x %d bytes = %.4f GB at %.1f TB/s = %.4f ms" % (what + ":", streams, n, streams * 8.0 * n / 1e9, a.hbm_tbs, streams * 8.0 * n / (a.hbm_tbs * 1e12) * 1e3), flush=True)
        print("    the stepper's own share (Newton accepts the guess: %d steps, %d Newton iterations, %d launches per call): %.3f ms per step whole, %.3f ms the residual's kernels, %.3f ms the rest = two sweeps, "
              "the Newton solve's own launches and two blocking reads; against the floor of the two sweeps %.4f ms"
              % (info_e["steps"], info_e["newton_iterations"], launches_e, total_e / a.steps, kernel_e / a.steps, own, 10 * 8.0 * n / (a.hbm_tbs * 1e12) * 1e3), flush=True)

        W, x, U1 = g.create_vec(), g.create_vec(), g.create_vec()
        host = []
        for k in range(3 + 5):
            reset()
            g.synchronize()
            t0 = time.perf_counter()
            host_steps(g, U, V, W, x, U1, h, a.steps, alpha, newton)
            g.synchronize()
            if k >= 3:
                host.append((time.perf_counter() - t0) * 1e3)
        host = statistics.median(host)
        print("    the same steps from Python (solve_nonlinear + Vec.axpby, median of 5): %.3f ms per step, %.3f x IGXTimeStep by the same clock"
              % (host / a.steps, host / wall), flush=True)
        del U, V, F, W, x, U1, g


if __name__ == "__main__":
    main()
