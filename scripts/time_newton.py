"""Times IGXSolveNonlinear on the case of profiles/newton.txt, in one process: Bratu (lambda = 3.5) at p = 2 on 63^3 elements, n = 274 625,
Dirichlet values on six faces, from x0 = 0; BiCGStab with the Jacobi preconditioner to lin_rtol = 1e-6, backtracking line search,
rtol = 1e-8.  Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs, and the same solve by the host's clock with timing
off (the timed run synchronises after every operator call to read its events).

    python scripts/time_newton.py [--size 63]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_action import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=63)
    a = ap.parse_args()
    import petiga_amd as P
    print(P.device_info(), flush=True)
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, a.size)
    g.setup()
    for d in range(3):
        for s in range(2):
            g.set_boundary_value(d, s, 0, 0.1 * d * s)
    g.set_form("bratu", (3.5,))
    x = g.create_vec()
    kw = dict(method="bicgstab", pc="jacobi", lin_rtol=1e-6, rtol=1e-8, linesearch="bt")
    seen = {}

    def solve():
        seen["info"] = g.solve_nonlinear(x.fill(0.0), **kw)

    total, kernel, _, _ = timed(g, solve)
    info, launches = seen["info"], g.last_timing()[2]
    wall = []
    for _ in range(10):
        x.fill(0.0)
        g.synchronize()
        t0 = time.perf_counter()
        g.solve_nonlinear(x, **kw)
        g.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall = statistics.median(wall)
    its = max(info["iterations"], 1)
    print("Bratu p = 2, %d^3 elements, n = %d: %s" % (a.size, x.n, g.kernel_name()), flush=True)
    print("  reason %s, %d iterations, inner %s, %d function evaluations, %d backtracks; %d launches per call" % (
        info["reason_name"], info["iterations"], [int(k) for k in info["linear_its"]], info["function_evaluations"], info["backtracks"], launches), flush=True)
    print("  IGXSolveNonlinear per Newton iteration: %.3f ms timed, operators' own kernels %.3f ms" % (total / its, kernel / its), flush=True)
    print("    by the host's clock with timing off: %.3f ms per Newton iteration" % (wall / its), flush=True)


if __name__ == "__main__":
    main()
