"""Times the matrix-free diagonal next to the two drivers it stands between, in one process (profiles/matrix_diagonal.txt):
  Poisson p = 3, N^3, Dirichlet values on the six faces, on the identity geometry and on bench.py's rational NURBS map:
  IGXComputeMatrixDiagonal, IGXComputeMatrixAction (the same kernel family) and IGXComputeMatrix (the matrix it replaces).
Plain IGXSetTiming / IGXGetLastTiming, 3 warm-ups, the median of 10 runs; ms (whole step, and the kernels alone), M elements/s, and
the shader clock IGXGetClockProbe saw on the assembly's launches.

    python scripts/time_diagonal.py [--size 128]"""
import argparse
import os
import sys

os.environ.setdefault("IGX_CLOCK_PROBE", "1")      # (read when the IGX is created)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import report, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    import petiga_amd as P
    from bench import _bench_geometry
    N, nel = a.size, float(a.size) ** 3
    print("Poisson p = 3, %d^3 elements" % N, flush=True)
    rng = np.random.default_rng(7)
    for geo in (False, True):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, 3, N)
        g.setup()
        if geo:
            g.set_geometry(*_bench_geometry(3, N, [False] * 3))
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 1.0)
        g.set_form("poisson")
        D = g.create_vec()
        X, Y = g.create_vec().set(rng.standard_normal(D.n)), g.create_vec()
        tag = "NURBS map" if geo else "identity "
        td = timed(g, lambda: g.compute_matrix_diagonal(D))
        report("%s IGXComputeMatrixDiagonal" % tag, g, nel, td)
        ta = timed(g, lambda: g.compute_matrix_action(X, Y))
        report("%s IGXComputeMatrixAction" % tag, g, nel, ta)
        A = g.create_mat()
        tm = timed(g, lambda: g.compute_matrix(A))
        report("%s IGXComputeMatrix" % tag, g, nel, tm)
        try:
            clock = "%.0f MHz" % g.clock_probe()[0]
        except P.IGXError:      # (the probe sits in the pencil kernels: an assembly on another kernel leaves nothing to read)
            clock = "not probed (no pencil-kernel launch)"
        print("%s kernels: diagonal / action = %.3f, diagonal / matrix = %.3f (1 / %.1f); shader clock on the assembly's launches: %s"
              % (tag, td[1] / ta[1], td[1] / tm[1], tm[1] / td[1], clock), flush=True)
        del A, D, X, Y, g


if __name__ == "__main__":
    main()
