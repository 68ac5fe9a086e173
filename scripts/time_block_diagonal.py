"""Times the matrix-free point-block diagonal beside its two baselines, and Invert / Apply beside a copy (profiles/matrix_block_diagonal.txt):
  Elasticity p = 3 at 128^3 on the identity geometry and on bench.py's rational NURBS map, NS-VMS p = 2 at 96^3:
  IGXCompute*BlockDiagonal, dof x IGXCompute*Diagonal (the cost with nothing shared between the dof^2 entries' columns) and the driver
  that assembles the matrix (IGXComputeMatrix / IGXComputeIJacobian); IGXBlockDiagonalInvert and IGXBlockDiagonalApply as GB/s of the
  bytes they read and write, beside a device-to-device copy that moves the same number of bytes, timed in the same run.
Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs, one process per case (give each its own time limit):

    python scripts/time_block_diagonal.py --case elasticity-identity | elasticity-nurbs | nsvms  [--size N] [--no-matrix]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import report, timed

NU, FX, DT = 1.472e-4, 3.37204e-3, 1e-2
NS = (NU, FX, -0.4 * FX, 0.25 * FX, DT)
EL = (1.5, 0.8)


def copy_gbs(nbytes, warmup=3, runs=10):
    """GB/s (read + written) of a device-to-device copy that moves nbytes in all"""
    import torch
    n = max(nbytes // 16, 1)
    a, b = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    ms = []
    for it in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return 16.0 * n / statistics.median(ms) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["elasticity-identity", "elasticity-nurbs", "nsvms"])
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--no-matrix", action="store_true", help="leave the assembling driver out")
    a = ap.parse_args()
    import petiga_amd as P
    from bench import _bench_geometry
    nsvms = a.case == "nsvms"
    dof, p, N = (4, 2, a.size or 96) if nsvms else (3, 3, a.size or 128)
    nel = float(N) ** 3
    rng = np.random.default_rng(7)
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, N)
    g.setup()
    if a.case == "elasticity-nurbs":
        g.set_geometry(*_bench_geometry(3, N, [False] * 3))
    if nsvms:
        for s in range(2):
            for f in range(3):
                g.set_boundary_value(1, s, f, 0.0)
        g.set_form("nsvms", NS)
    else:
        for f in range(3):
            g.set_boundary_value(0, 0, f, 0.0)
        g.set_form("elasticity", EL)
    tag = "%s p = %d, %d^3" % (a.case, p, N)
    B = [g.create_vec() for _ in range(dof)]
    D, X, Y = g.create_vec(), g.create_vec(), g.create_vec()
    n = D.n
    X.set(rng.standard_normal(n))
    if nsvms:
        U, V = g.create_vec().set(0.3 * rng.standard_normal(n)), g.create_vec().set(0.1 * rng.standard_normal(n))
        block = lambda: g.compute_ijacobian_block_diagonal(2.0 / DT, V, 0.0, U, B)
        diag = lambda: g.compute_ijacobian_diagonal(2.0 / DT, V, 0.0, U, D)
    else:
        block = lambda: g.compute_matrix_block_diagonal(B)
        diag = lambda: g.compute_matrix_diagonal(D)
    tb = timed(g, block)
    report("%s block diagonal" % tag, g, nel, tb)
    td = timed(g, diag)
    report("%s diagonal" % tag, g, nel, td)
    print("%s kernels: block diagonal / (dof x diagonal) = %.3f (dof = %d: %.3f ms against %.3f ms)" % (tag, tb[1] / (dof * td[1]), dof, tb[1], dof * td[1]), flush=True)
    nnode = n // dof
    inv_bytes, app_bytes = 2 * dof * dof * 8 * nnode, (dof * dof + 2 * dof) * 8 * nnode
    ta = timed(g, lambda: g.block_diagonal_apply(B, X, Y))
    report("%s IGXBlockDiagonalApply" % tag, g, nel, ta)
    # Invert replaces B by its inverse: every timed call inverts the previous result, the same work on as regular a block
    ti = timed(g, lambda: g.block_diagonal_invert(B, count=False))
    report("%s IGXBlockDiagonalInvert" % tag, g, nel, ti)
    print("%s Invert %.1f GB/s (%.3f ms, %d bytes), a copy of as many bytes %.1f GB/s; Apply %.1f GB/s (%.3f ms, %d bytes), a copy %.1f GB/s"
          % (tag, inv_bytes / ti[1] / 1e6, ti[1], inv_bytes, copy_gbs(inv_bytes), app_bytes / ta[1] / 1e6, ta[1], app_bytes, copy_gbs(app_bytes)), flush=True)
    if not a.no_matrix:
        A = g.create_mat()
        tm = timed(g, (lambda: g.compute_ijacobian(2.0 / DT, V, 0.0, U, A)) if nsvms else (lambda: g.compute_matrix(A)))
        report("%s %s" % (tag, "IGXComputeIJacobian" if nsvms else "IGXComputeMatrix"), g, nel, tm)
        print("%s kernels: block diagonal / matrix = %.3f (1 / %.1f)" % (tag, tb[1] / tm[1], tm[1] / tb[1]), flush=True)


if __name__ == "__main__":
    main()
