"""The block-vector algebra and IGXEigenSolve on a GPU.
1. One IGXVecMDot of 24 x 24 and of 48 x 48 columns, and the matching IGXVecMAXPY (beta = 1), against the same work done with IGXVecDot /
   IGXVecAXPBY (nx ny calls each), at the finest lengths of scripts/multigrid_rate.py (p = 2 and p = 3, --size elements per axis).  Times
   are the host's clock around work that ends in a synchronise, after a warm-up of every shape; the two versions alternate in every round
   and the median, the least and the largest round are printed.  Bytes are counted from the shapes: MDot reads (nx + ny) vectors, MAXPY
   reads nx + ny and writes ny.  The results of the two versions are compared before anything is timed.
2. A whole solve (Poisson + Mass, all faces Dirichlet, nev 4, block 6, rtol 1e-8) with every preconditioner at --solve-size elements per
   axis: the host's clock around the solve with timing off, and from a second run with timing on the time inside the operators' kernels
   (IGXGetLastTiming: the drivers' own events).
Appends to the output file (profiles/eigen.txt).

    python scripts/eigen_rate.py [--size 128] [--solve-size 64] [--degrees 2 3] [--out profiles/eigen.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALL6 = [(d, s) for d in range(3) for s in range(2)]


def space(P, p, n, form=None):
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, p, n)
    g.setup()
    if form:
        for d, s in ALL6:
            g.set_boundary_value(d, s, 0, 0.0)
        g.set_form(form)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--solve-size", type=int, default=64)
    ap.add_argument("--degrees", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigen.txt"))
    a = ap.parse_args()
    import petiga_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rounds_of(g, versions, reps):
        """ms per call of every version: [rounds] each, the versions alternating inside a round"""
        out = [[] for _ in versions]
        for _ in range(a.rounds):
            for k, (call, r) in enumerate(zip(versions, reps)):
                g.synchronize()
                t0 = time.perf_counter()
                for _ in range(r):
                    call()
                g.synchronize()
                out[k].append((time.perf_counter() - t0) * 1e3 / r)
        return [np.array(v) for v in out]

    fmt = lambda v: "%.3f ms (%.3f .. %.3f)" % (np.median(v), v.min(), v.max())
    say("block-vector algebra and eigen solve; %s" % P.device_info())
    for p in a.degrees:
        g = space(P, p, a.size)
        n = g.create_vec().n
        rng = np.random.default_rng(p)
        X = [g.create_vec().set(rng.standard_normal(n)) for _ in range(48)]
        Y = [g.create_vec().set(rng.standard_normal(n)) for _ in range(48)]
        Z = [g.create_vec() for _ in range(48)]
        for k in (24, 48):
            Cm = rng.standard_normal((k, k))
            # the same numbers both ways, before anything is timed
            G = P.Vec.mdot(X[:k], Y[:k])
            G1 = np.array([[X[i].dot(Y[j]) for j in range(k)] for i in range(k)])
            scale = np.sqrt(np.outer([x.dot(x) for x in X[:k]], [y.dot(y) for y in Y[:k]]))
            say("p = %d, n = %d, %d x %d: IGXVecMDot against %d IGXVecDot: max |G - G1| / (|x| |y|) = %.3e" % (p, n, k, k, k * k, np.abs(G - G1).max() / scale.max()))

            def split_dots():
                for i in range(k):
                    for j in range(k):
                        X[i].dot(Y[j])

            def split_axpby():
                for j in range(k):
                    for i in range(k):
                        Z[j].axpby(Cm[i, j], X[i], 1.0)

            for j in range(k):
                Z[j].copy_from(Y[j])
            P.Vec.maxpy(Z[:k], X[:k], Cm, 1.0)
            one = Z[0].get()
            Z[0].copy_from(Y[0])
            for i in range(k):
                Z[0].axpby(Cm[i, 0], X[i], 1.0)
            say("    IGXVecMAXPY against %d IGXVecAXPBY: max deviation of column 0 / max |y| = %.3e" % (k * k, np.abs(one - Z[0].get()).max() / np.abs(one).max()))
            block, split = rounds_of(g, [lambda: P.Vec.mdot(X[:k], Y[:k]), split_dots], [20, 1])
            gb = 2 * k * n * 8e-9
            say("    IGXVecMDot  %s = %.0f GB/s over %d vectors read once; %d x IGXVecDot %s: %.0fx"
                % (fmt(block), gb / np.median(block) * 1e3, 2 * k, k * k, fmt(split), np.median(split) / np.median(block)))
            block, split = rounds_of(g, [lambda: P.Vec.maxpy(Z[:k], X[:k], Cm, 1.0), split_axpby], [20, 1])
            gb = 3 * k * n * 8e-9
            say("    IGXVecMAXPY %s = %.0f GB/s over %d vectors read and %d written; %d x IGXVecAXPBY %s: %.0fx"
                % (fmt(block), gb / np.median(block) * 1e3, 2 * k, k, k * k, fmt(split), np.median(split) / np.median(block)))
        del X, Y, Z
    for p in a.degrees:
        stiff, mass = space(P, p, a.solve_size, "poisson"), space(P, p, a.solve_size, "mass")
        stiff.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
        n = stiff.create_vec().n
        for pc in ("none", "jacobi", "pbjacobi", "fastdiag"):
            stiff.eigen(4, mass=mass, block=6, pc=pc, rtol=1e-8, maxit=3)      # warm-up: every kernel of the loop
            stiff.synchronize()
            t0 = time.perf_counter()
            out = stiff.eigen(4, mass=mass, block=6, pc=pc, rtol=1e-8, maxit=1000)
            stiff.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            launches = stiff.last_timing()[2]
            for g in (stiff, mass):      # once more with the drivers' events: every action then ends in an event synchronise, so this run is not the timed one
                g.set_timing(True)
            stiff.eigen(4, mass=mass, block=6, pc=pc, rtol=1e-8, maxit=1000)
            total, kernel, _ = stiff.last_timing()
            for g in (stiff, mass):
                g.set_timing(False)
            say("p = %d, n = %d, nev 4, block 6, pc=%-8s %4d iterations, reason %s, %d restarts, %d actions, %9.2f ms, %d launches (with timing on: %.2f ms, of which %.2f ms in the operators' kernels); "
                "lambda %s" % (p, n, pc, out["iterations"], out["reason_name"], out["restarts"], out["actions"], ms, launches, total, kernel, np.array2string(out["lambda"][:4], precision=6)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
