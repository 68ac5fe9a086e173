"""Times IGXSolve next to the operators it calls and next to the same loop driven from the host, in one process (profiles/krylov_solve.txt):
  Poisson p = 3 on the benchmark's rational NURBS map (bench.py: _bench_geometry), zero Dirichlet values on the six faces, the form's unit
  source as the right-hand side, at 128^3 and 256^3 elements; CG with fast diagonalisation (alpha = 0, beta = 1) and CG with Jacobi.
Every solve runs a fixed number of iterations (rtol = atol = 0, maxit = --its), so the figures are per iteration.  Plain IGXSetTiming /
IGXGetLastTiming, 3 warm-ups, the median of 10 runs: the whole solve, and the sum of the action's and the preconditioner's own kernel times
in the same run (Jacobi's division is fused into a sweep of the loop and counts as a sweep).  The timed run synchronises after every
operator call to read its events, so the solve is timed once more by the host's clock with timing off.  The vector-sweep floor is written
out: sweeps x 8 n bytes / the HBM rate, with 13 sweeps per iteration for fast diagonalisation (p.Ap 2; x, r, r.r 6; r.z 2; p 3) and 14 for
Jacobi (z = r ./ D, r.z 3 instead of 2).  The host loop is pcg() of tests/fast_diag_ref.py on the same engine operators, one copy each way
per product, for --host-its iterations.

    python scripts/time_solve.py [--cases 128,256] [--its 20] [--host-its 5] [--hbm-tbs 8.0]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import timed


def bench_geometry(p, size):
    """bench.py's _bench_geometry without its periodic branch"""
    from petiga_amd.geometry import greville
    U = np.concatenate([[0.0] * (p + 1), np.arange(1, size) / size, [1.0] * (p + 1)])
    gv = [greville(U, p)] * 3
    mesh = np.meshgrid(*gv[::-1], indexing="ij")[::-1]
    X = np.stack([m.copy() for m in mesh], axis=-1)
    X[..., 0] += 0.05 * np.sin(2 * np.pi * mesh[1])
    X[..., 1] += 0.05 * np.sin(2 * np.pi * mesh[2])
    W = 1.0 + 0.1 * np.cos(2 * np.pi * mesh[0])
    return X.reshape(-1, 3), W.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128,256")
    ap.add_argument("--its", type=int, default=20)
    ap.add_argument("--host-its", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate the sweep floor is taken at, TB/s (MI355X data sheet: 8)")
    a = ap.parse_args()
    import petiga_amd as P
    from fast_diag_ref import pcg
    print(P.device_info(), flush=True)
    p = 3
    for N in (int(v) for v in a.cases.split(",")):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, p, N)
        g.setup()
        g.set_geometry(*bench_geometry(p, N))
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 0.0)
        g.set_form("poisson")
        g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
        b, x = g.create_vec(), g.create_vec()
        g.compute_vector(b)
        g.synchronize()
        n = b.n
        print("Poisson p = %d, %d^3 elements on the benchmark's NURBS map, n = %d (%.1f MB per vector), %d iterations per solve" % (p, N, n, 8 * n / 1e6, a.its), flush=True)
        Xv, Yv, Dv = g.create_vec(), g.create_vec(), g.create_vec()
        g.compute_matrix_diagonal(Dv)
        t_act = timed(g, lambda: g.compute_matrix_action(b, Yv))
        t_fd = timed(g, lambda: g.fast_diag_apply(b, Yv))
        print("  IGXComputeMatrixAction %.3f ms, IGXFastDiagApply %.3f ms (kernels, median of 10)" % (t_act[1], t_fd[1]), flush=True)
        for pc, sweeps in (("fastdiag", 13), ("jacobi", 14)):
            def solve():
                x.fill(0.0)
                return g.solve(b, x, method="cg", pc=pc, rtol=0.0, atol=0.0, maxit=a.its)
            info = solve()
            assert info["iterations"] == a.its and info["reason"] == -1, info
            total, kernel, _, _ = timed(g, solve)
            launches = g.last_timing()[2]
            wall = []
            for _ in range(10):
                g.synchronize()
                t0 = time.perf_counter()
                solve()
                g.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            wall = statistics.median(wall)
            floor = sweeps * 8.0 * n / (a.hbm_tbs * 1e12) * 1e3
            print("  CG + %-8s IGXSolve per iteration: %.3f ms by the host's clock (timing off), %.3f ms timed; operators' own kernels %.3f ms; "
                  "IGXSolve / operators = %.3f (timing off), %.3f (timed); %d launches per solve; |r_k| / |r_0| = %.3e"
                  % (pc, wall / a.its, total / a.its, kernel / a.its, wall / kernel, total / kernel, launches, info["rnorm"] / info["rnorm0"]), flush=True)
            print("    sweep floor: %d sweeps x 8 x %d bytes = %.3f GB at %.1f TB/s = %.3f ms per iteration; the loop's own share (timing off) %.3f ms"
                  % (sweeps, n, sweeps * 8.0 * n / 1e9, a.hbm_tbs, floor, (wall - kernel) / a.its), flush=True)

            def op(v):
                g.compute_matrix_action(Xv.set(v), Yv)
                g.synchronize()
                return Yv.get()

            if pc == "fastdiag":
                def prec(v):
                    g.fast_diag_apply(Xv.set(v), Yv)
                    g.synchronize()
                    return Yv.get()
            else:
                D = Dv.get()
                prec = lambda v: v / D
            rhs = b.get()
            t0 = time.perf_counter()
            _, k = pcg(op, prec, rhs, rtol=0.0, maxit=a.host_its)
            t_host = (time.perf_counter() - t0) * 1e3
            print("    the host loop (pcg of tests/fast_diag_ref.py, %d iterations): %.1f ms per iteration, %.1f x IGXSolve" % (k, t_host / k, t_host / k / (wall / a.its)), flush=True)
        del b, x, Xv, Yv, Dv, g


if __name__ == "__main__":
    main()
