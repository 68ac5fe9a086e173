"""Times the fast-diagonalisation preconditioner next to the operator it preconditions, in one process (profiles/fast_diag.txt):
  Poisson p = 3 at 128^3 and 256^3 and p = 2 at 256^3 elements, Dirichlet values on the six faces, identity geometry:
  IGXFastDiagApply beside IGXComputeMatrixAction, and the host time of IGXFastDiagSetUp.
Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs.  IGXFastDiagApply is held against the two floors it has:
12 sweeps of the vector (each of the six contractions reads it once and writes it once) at the HBM rate, and 12 sum_d m_d n^3 flops
(2 m_d flops per entry and contraction, forward and backward; n^3 entries) at the FP64 matrix rate; both are written out.

    python scripts/time_fast_diag.py [--hbm-tbs 8.0] [--fp64-tflops 78.6]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import report, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate the sweep floor is taken at, TB/s (MI355X data sheet: 8)")
    ap.add_argument("--fp64-tflops", type=float, default=78.6, help="FP64 matrix rate the flop floor is taken at, TFLOP/s (MI355X data sheet: 78.6)")
    ap.add_argument("--cases", default="3:128,3:256,2:256")
    a = ap.parse_args()
    import petiga_amd as P
    print(P.device_info(), flush=True)
    rng = np.random.default_rng(7)
    for case in a.cases.split(","):
        p, N = (int(v) for v in case.split(":"))
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, p, N)
        g.setup()
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 1.0)
        g.set_form("poisson")
        t0 = time.perf_counter()
        g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
        t_setup = time.perf_counter() - t0
        n = g.sizes()["node_sizes"]
        m = [g.fast_diag_get_axis(d, 0)[1] for d in range(3)]
        R = g.create_vec()
        R.set(rng.standard_normal(R.n))
        Z, Y = g.create_vec(), g.create_vec()
        nel, nn = float(N) ** 3, float(n[0]) * n[1] * n[2]
        print("Poisson p = %d, %d^3 elements, %d x %d x %d functions (free: %d x %d x %d); IGXFastDiagSetUp (host): %.3f s"
              % (p, N, n[0], n[1], n[2], m[0], m[1], m[2], t_setup), flush=True)
        tf = timed(g, lambda: g.fast_diag_apply(R, Z))
        report("IGXFastDiagApply", g, nel, tf)
        ta = timed(g, lambda: g.compute_matrix_action(R, Y))
        report("IGXComputeMatrixAction", g, nel, ta)
        sweep_bytes, flops = 12 * nn * 8, 12.0 * sum(m) * nn
        t_sweep, t_flop = sweep_bytes / (a.hbm_tbs * 1e12) * 1e3, flops / (a.fp64_tflops * 1e12) * 1e3
        print("  floors: 12 sweeps = %.3f GB at %.1f TB/s = %.3f ms (achieved share %.1f %%, %.2f TB/s); 12 sum m n^3 = %.2f GFLOP at %.1f TFLOP/s = %.3f ms "
              "(achieved share %.1f %%, %.2f TFLOP/s); Apply / Action = %.3f"
              % (sweep_bytes / 1e9, a.hbm_tbs, t_sweep, 100 * t_sweep / tf[1], sweep_bytes / tf[1] / 1e9, flops / 1e9, a.fp64_tflops, t_flop,
                 100 * t_flop / tf[1], flops / tf[1] / 1e9, tf[1] / ta[1]), flush=True)
        del R, Z, Y, g


if __name__ == "__main__":
    main()
