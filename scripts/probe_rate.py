"""Measures IGXProbeEvaluate (probe.hpp) and writes profiles/probe.txt: p = 3 on N^3 elements (default 64), dof 1, the identity geometry
and bench.py's NURBS net, der 0 and der 1, for 2^21 seeded random points and for a 128^3 lexicographic sample grid (axis 0 fastest).
Per configuration: points per second and the kernel's own ms (IGXSetTiming / IGXGetLastTiming: HIP events around the one launch, 3
warm-ups, the median of 10 runs), the whole call (kernel + the copy of the result to the host), the bytes a point touches and the rate
that makes.  The bytes are counted from shapes: the point (dim doubles), its span triple and flag, the (p+1)^3 gathered coefficients of
every field, of W and -- with derivatives on a map -- of X, and the result; gathers are counted in full, without the reuse the caches give
neighbouring points, so the figure for the sorted grid is the traffic the kernel asks for, not what reaches HBM.
Beside these the one existing yardstick: the point rate of IGXComputeFunction (Bratu: value and gradient of u at 64 quadrature points
per element, by sum factorisation) on the same mesh -- how far per-point evaluation of a sorted grid stands from the tensor-product path.

    python scripts/probe_rate.py [--size 64] [--grid 128] [--random 2097152] [--out profiles/probe.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import timed


def bench_net(p, size):
    """bench.py's NURBS net (_bench_geometry) on the open uniform knot vectors"""
    from petiga_amd.geometry import greville
    gv = [greville(np.concatenate([[0.0] * (p + 1), np.arange(1, size) / size, [1.0] * (p + 1)]), p) for _ in range(3)]
    mesh = np.meshgrid(*gv[::-1], indexing="ij")[::-1]
    X = np.stack([m.copy() for m in mesh], axis=-1)
    X[..., 0] += 0.05 * np.sin(2 * np.pi * mesh[1])
    X[..., 1] += 0.05 * np.sin(2 * np.pi * mesh[2])
    W = 1.0 + 0.1 * np.cos(2 * np.pi * mesh[0])
    return X.reshape(-1, 3), W.reshape(-1)


def bytes_per_point(p, dof, der, rational, mapped):
    nen = (p + 1) ** 3
    gathers = nen * dof + (nen if rational else 0) + (3 * nen if (mapped and der > 0) else 0)
    return 8 * 3 + 4 * 3 + 1 + 8 * gathers + 8 * dof * 3 ** der


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--random", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe.txt"))
    a = ap.parse_args()
    import petiga_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    p, N = 3, a.size
    say(P.device_info())
    say("IGXProbeEvaluate, p = %d, %d^3 elements, dof 1; kernel ms: HIP events around the launch, median of 10 after 3 warm-ups" % (p, N))
    rng = np.random.default_rng(21)
    t = (np.arange(a.grid) + 0.5) / a.grid
    G2, G1, G0 = np.meshgrid(t, t, t, indexing="ij")
    sets = (("%d random points" % a.random, rng.random((a.random, 3))), ("%d^3 sample grid, axis 0 fastest" % a.grid, np.stack([G0.ravel(), G1.ravel(), G2.ravel()], axis=-1)))
    for geo in ("identity", "nurbs"):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, p, N)
        g.setup()
        if geo == "nurbs":
            g.set_geometry(*bench_net(p, N))
        U = g.create_vec()
        U.set(rng.uniform(-1, 1, U.n))
        for label, pts in sets:
            prb = g.probe(pts, order=1)
            for der in (0, 1):
                out = np.empty((len(pts), 1) + (3,) * der)
                total, kernel, lo, hi = timed(g, lambda: prb.evaluate(U, der, out=out))
                b = bytes_per_point(p, 1, der, geo == "nurbs", geo == "nurbs")
                say("%-8s %-36s der %d: kernel %8.3f ms, %8.1f M points/s, %5d bytes/point -> %7.1f GB/s; whole call %8.3f ms (min %.3f max %.3f); %s"
                    % (geo, label, der, kernel, len(pts) / kernel / 1e3, b, len(pts) * b / kernel / 1e6, total, lo, hi, g.kernel_name()))
            prb.close()
        if geo == "identity":
            g.set_form("bratu", (1.0,))
            F = g.create_vec()
            tf = timed(g, lambda: g.compute_function(U, F))
            npt = N ** 3 * (p + 1) ** 3
            say("yardstick  IGXComputeFunction (Bratu, u and grad u at %d points per element, sum-factorised): kernels %.3f ms, %.1f M points/s; %s"
                % ((p + 1) ** 3, tf[1], npt / tf[1] / 1e3, g.kernel_name()))
        del U, g
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
