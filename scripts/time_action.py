"""Times the matrix-free actions next to the drivers they stand beside, in one process (profiles/matrix_action.txt):
  config 4's state  Cahn-Hilliard p = 2, N^3: IGXComputeIJacobianAction next to IGXComputeIFunction (the same kernel family)
  Poisson p = 3, N^3: IGXComputeMatrixAction next to IGXComputeSystem
Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs; ms (whole step, and the kernels alone) and M elements/s.
IGX_LIB=<another build of the library> times that build instead; drivers it lacks are left out (the Residual of a parent build
next to this one's, same machine, same minute).

    python scripts/time_action.py [--size 256] [--skip-system]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(g, call, warmup=3, runs=10):
    g.set_timing(True)
    for _ in range(warmup):
        call()
        g.synchronize()
    total, kernel = [], []
    for _ in range(runs):
        call()
        g.synchronize()
        t = g.last_timing()
        total.append(t[0]); kernel.append(t[1])
    g.set_timing(False)
    return statistics.median(total), statistics.median(kernel), min(total), max(total)


def report(label, g, nel, t):
    print("%-44s %9.3f ms (kernels %9.3f ms; min %9.3f max %9.3f) %9.1f M el/s  %s" % (label, t[0], t[1], t[2], t[3], nel / t[0] / 1e3, g.kernel_name()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--skip-system", action="store_true", help="leave IGXComputeSystem out (its matrix takes 70 GB at 256^3)")
    a = ap.parse_args()
    import petiga_amd as P
    have_action = hasattr(P.lib(), "IGXComputeMatrixAction")
    N, nel = a.size, float(a.size) ** 3
    print("library: %s; actions: %s; %d^3 elements" % (os.environ.get("IGX_LIB", "this tree's"), "yes" if have_action else "no", N), flush=True)
    rng = np.random.default_rng(7)

    # config 4: demo/CahnHilliard3D.c, p = 2 C1 (bench.py: build_problem)
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, N)
    g.setup()
    g.set_form("cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / (3.0 * N * N), 1.0))
    F = g.create_vec()
    n = F.n
    U, V, X, Y = g.create_vec().set(0.63 + 0.05 * (2 * rng.random(n) - 1)), g.create_vec().set(0.01 * rng.standard_normal(n)), g.create_vec().set(rng.standard_normal(n)), g.create_vec()
    shift = 1e3
    report("CahnHilliard p=2 IGXComputeIFunction", g, nel, timed(g, lambda: g.compute_ifunction(shift, V, 0.0, U, F)))
    if have_action:
        report("CahnHilliard p=2 IGXComputeIJacobianAction", g, nel, timed(g, lambda: g.compute_ijacobian_action(shift, V, 0.0, U, X, Y)))
        report("CahnHilliard p=2 IGXComputeIFunction (again)", g, nel, timed(g, lambda: g.compute_ifunction(shift, V, 0.0, U, F)))
    del U, V, X, Y, F, g

    # the headline: demo/Poisson3D.c, p = 3, u = 1 on every face
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 3, N)
    g.setup()
    for d in range(3):
        for s in range(2):
            g.set_boundary_value(d, s, 0, 1.0)
    g.set_form("poisson")
    b = g.create_vec()
    X, Y = g.create_vec().set(rng.standard_normal(b.n)), g.create_vec()
    if have_action:
        report("Poisson p=3 IGXComputeMatrixAction", g, nel, timed(g, lambda: g.compute_matrix_action(X, Y)))
    report("Poisson p=3 IGXComputeVector", g, nel, timed(g, lambda: g.compute_vector(b)))
    if not a.skip_system:
        A = g.create_mat()
        report("Poisson p=3 IGXComputeSystem", g, nel, timed(g, lambda: g.compute_system(A, b)))


if __name__ == "__main__":
    main()
