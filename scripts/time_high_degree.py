"""Times the matrix-free action and diagonal above four basis functions or points per axis (vec_sumfact, one workgroup per element)
next to the matrix they replace, in one process (profiles/matrix_free_high_degree.txt):
  Poisson p = 4 at 64^3, p = 5 at 48^3, p = 6 at 32^3, Dirichlet values on the six faces, on the identity geometry and on bench.py's
  rational NURBS map: IGXComputeMatrixAction, IGXComputeMatrixDiagonal and IGXComputeMatrix on the same problem;
  Poisson p = 3 with five points per axis at 128^3: IGXComputeMatrixAction.
Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs (the matrix: 1 warm-up, 3 runs); ms (whole step, and the
kernels alone), launches, M elements/s.

--regression times the drivers a change to vec_sumfact.hpp must leave alone instead: IGXComputeMatrixAction and
IGXComputeMatrixDiagonal for Poisson p = 3 at 128^3 and IGXComputeIFunction for Cahn-Hilliard p = 2 at 256^3.  IGX_LIB=<another build
of the library> times that build: run the two builds alternately, same machine, same minutes.

    python scripts/time_high_degree.py [--regression] [--out profiles/matrix_free_high_degree.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import timed

CONFIGS = [(4, 64), (5, 48), (6, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regression", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_free_high_degree.txt"))
    ap.add_argument("--scale", type=float, default=1.0, help="scales the element counts per axis (a quick trial run)")
    a = ap.parse_args()
    import petiga_amd as P
    from bench import _bench_geometry
    out = open(a.out, "a")

    def say(text):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    def report(label, g, nel, t):
        say("%-52s %10.3f ms (kernels %10.3f ms; min %10.3f max %10.3f) %5d launches %9.2f M el/s  %s"
            % (label, t[0], t[1], t[2], t[3], g.last_timing()[2], nel / t[0] / 1e3, g.kernel_name()))

    def poisson(p, N, nqp=None, geo=False):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, p, N)
            if nqp:
                g.set_quadrature(i, nqp)
        g.setup()
        if geo:
            g.set_geometry(*_bench_geometry(p, N, [False] * 3))
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 1.0)
        g.set_form("poisson")
        return g

    rng = np.random.default_rng(7)
    sz = lambda N: max(2, int(round(N * a.scale)))
    if a.regression:
        say("library: %s" % os.environ.get("IGX_LIB", "this tree's"))
        N = sz(128)
        g = poisson(3, N)
        D = g.create_vec()
        X, Y = g.create_vec().set(rng.standard_normal(D.n)), g.create_vec()
        report("Poisson p=3 %d^3 IGXComputeMatrixAction" % N, g, float(N) ** 3, timed(g, lambda: g.compute_matrix_action(X, Y)))
        report("Poisson p=3 %d^3 IGXComputeMatrixDiagonal" % N, g, float(N) ** 3, timed(g, lambda: g.compute_matrix_diagonal(D)))
        del D, X, Y, g
        N = sz(256)
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, 2, N)
        g.setup()
        g.set_form("cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / (3.0 * N * N), 1.0))
        F = g.create_vec()
        U, V = g.create_vec().set(0.63 + 0.05 * (2 * rng.random(F.n) - 1)), g.create_vec().set(0.01 * rng.standard_normal(F.n))
        report("CahnHilliard p=2 %d^3 IGXComputeIFunction" % N, g, float(N) ** 3, timed(g, lambda: g.compute_ifunction(1e3, V, 0.0, U, F)))
        return
    for p, N in CONFIGS:
        N = sz(N)
        nel = float(N) ** 3
        for geo in (False, True):
            g = poisson(p, N, geo=geo)
            tag = "Poisson p=%d %d^3 %s" % (p, N, "NURBS map" if geo else "identity ")
            D = g.create_vec()
            X, Y = g.create_vec().set(rng.standard_normal(D.n)), g.create_vec()
            ta = timed(g, lambda: g.compute_matrix_action(X, Y))
            report("%s IGXComputeMatrixAction" % tag, g, nel, ta)
            td = timed(g, lambda: g.compute_matrix_diagonal(D))
            report("%s IGXComputeMatrixDiagonal" % tag, g, nel, td)
            A = g.create_mat()
            tm = timed(g, lambda: g.compute_matrix(A), warmup=1, runs=3)
            report("%s IGXComputeMatrix" % tag, g, nel, tm)
            say("%s kernels: action / matrix = %.4f (1 / %.1f), diagonal / matrix = %.4f (1 / %.1f), diagonal / action = %.3f"
                % (tag, ta[1] / tm[1], tm[1] / ta[1], td[1] / tm[1], tm[1] / td[1], td[1] / ta[1]))
            del A, D, X, Y, g
    N = sz(128)
    g = poisson(3, N, nqp=5)
    X, Y = g.create_vec(), g.create_vec()
    X.set(rng.standard_normal(X.n))
    report("Poisson p=3 nqp=5 %d^3 identity  IGXComputeMatrixAction" % N, g, float(N) ** 3, timed(g, lambda: g.compute_matrix_action(X, Y)))


if __name__ == "__main__":
    main()
