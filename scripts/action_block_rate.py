"""The matrix-free action on a block of vectors against the same columns through the single-column action, on a GPU.
1. IGXCompute*ActionBlock at nx = 1, 2, 4, 6 and 16 against nx calls of IGXCompute*Action on the same vectors: Poisson and Mass at
   p = 2 and p = 3 on --size elements per axis, NURBS-mapped Poisson, Elasticity and the Bratu Jacobian at p = 3, Poisson at p = 5 on
   --high-size elements per axis.  The method is that of scripts/eigen_rate.py: the host's clock around work that ends in a synchronise,
   after a warm-up of every shape; the two versions alternate in every round and the median, the least and the largest round are
   printed.  The results of the two versions are compared before anything is timed (the number of entries that differ, and the largest
   deviation over the largest entry).
2. The solves of scripts/eigen_rate.py's second part (Poisson + Mass, all faces Dirichlet, nev 4, block 6, rtol 1e-8, every preconditioner,
   p = 2 and p = 3 at --solve-size elements per axis) with IGXSetBatchedActions off and on: the host's clock around the solve with timing
   off, the launches, and from a second run with timing on the time inside the operators' kernels.
Appends to the output file (profiles/action_block.txt).

    python scripts/action_block_rate.py [--size 64] [--high-size 16] [--solve-size 64] [--out profiles/action_block.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALL6 = [(d, s) for d in range(3) for s in range(2)]
NX = (1, 2, 4, 6, 16)
EL = (1.5, 0.8)


def nurbs_map(p, n):
    """a smooth rational perturbation of the unit cube on the space's own control net: (X [nodes, 3], W [nodes])"""
    m = n + p
    t = [np.linspace(0.0, 1.0, m)] * 3
    x, y, z = np.meshgrid(*t, indexing="ij")
    amp = 0.03
    X = np.stack([x + amp * np.sin(np.pi * y) * np.sin(np.pi * z), y + amp * np.sin(np.pi * x) * np.sin(np.pi * z), z + amp * np.sin(np.pi * x) * np.sin(np.pi * y)], axis=-1)
    W = 1.0 + 0.2 * np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)
    order = lambda a: np.ascontiguousarray(np.transpose(a, (2, 1, 0) + tuple(range(3, a.ndim))))      # axis 0 fastest
    return order(X).reshape(-1, 3), order(W).reshape(-1)


def space(P, form, p, n, dof=1, params=(), geometry=False):
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, n)
    g.setup()
    if geometry:
        g.set_geometry(*nurbs_map(p, n))
    for d, s in ALL6:
        for f in range(dof):
            g.set_boundary_value(d, s, f, 0.0)
    g.set_form(form, params)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--high-size", type=int, default=16)
    ap.add_argument("--solve-size", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_block.txt"))
    a = ap.parse_args()
    import petiga_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rounds_of(g, versions, reps):
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
    say("action on a block of vectors against single-column actions; %s" % P.device_info())
    cases = [("poisson p=2", "poisson", 2, a.size, 1, (), False, "matrix"), ("mass p=2", "mass", 2, a.size, 1, (), False, "matrix"),
             ("poisson p=3", "poisson", 3, a.size, 1, (), False, "matrix"), ("mass p=3", "mass", 3, a.size, 1, (), False, "matrix"),
             ("poisson p=3 nurbs", "poisson", 3, a.size, 1, (), True, "matrix"), ("elasticity p=3", "elasticity", 3, a.size, 3, EL, False, "matrix"),
             ("bratu jacobian p=3", "bratu", 3, a.size, 1, (3.5,), False, "jacobian"), ("poisson p=5", "poisson", 5, a.high_size, 1, (), False, "matrix")]
    for name, form, p, n, dof, params, geometry, driver in cases:
        g = space(P, form, p, n, dof, params, geometry)
        nv = g.create_vec().n
        rng = np.random.default_rng(p)
        X = [g.create_vec().set(rng.standard_normal(nv)) for _ in range(max(NX))]
        Y = [g.create_vec() for _ in range(max(NX))]
        Z = [g.create_vec() for _ in range(max(NX))]
        Us = g.create_vec().set(0.3 * rng.standard_normal(nv))
        if driver == "matrix":
            block = lambda k: g.compute_matrix_action_block(X[:k], Y[:k])
            single = lambda j: g.compute_matrix_action(X[j], Z[j])
        else:
            block = lambda k: g.compute_jacobian_action_block(Us, X[:k], Y[:k])
            single = lambda j: g.compute_jacobian_action(Us, X[j], Z[j])
        block(max(NX))
        kname, launches = g.kernel_name(), g.last_timing()[2]
        for j in range(max(NX)):
            single(j)
        g.synchronize()
        differ, dev = 0, 0.0
        for j in range(max(NX)):
            yb, ys = Y[j].get(), Z[j].get()
            differ += int(np.count_nonzero(yb != ys))
            dev = max(dev, float(np.abs(yb - ys).max() / np.abs(ys).max()))
        say("%s, %d^3 elements, n = %d: %s, %d launches for %d columns against %d x %d; %d of %d entries differ from the single action's, largest deviation / largest entry %.2e"
            % (name, n, nv, kname, launches, max(NX), max(NX), g.last_timing()[2], differ, max(NX) * nv, dev))
        for k in NX:
            reps = max(1, 16 // k)

            def split():
                for j in range(k):
                    single(j)

            tb, ts = rounds_of(g, [lambda: block(k), split], [reps, reps])
            say("    nx = %2d: block %s, %d single actions %s: %.2fx (block per column %.3f ms)" % (k, fmt(tb), k, fmt(ts), np.median(ts) / np.median(tb), np.median(tb) / k))
        del X, Y, Z, g
    if not a.skip_solves:
        for p in (2, 3):
            stiff, mass = space(P, "poisson", p, a.solve_size), space(P, "mass", p, a.solve_size)
            stiff.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
            nv = stiff.create_vec().n
            for pc in ("none", "jacobi", "pbjacobi", "fastdiag"):
                for flag in (0, 1):
                    stiff.set_batched_actions(flag)
                    stiff.eigen(4, mass=mass, block=6, pc=pc, rtol=1e-8, maxit=3)      # warm-up: every kernel of the loop
                    stiff.synchronize()
                    t0 = time.perf_counter()
                    out = stiff.eigen(4, mass=mass, block=6, pc=pc, rtol=1e-8, maxit=1000)
                    stiff.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                    launches = stiff.last_timing()[2]
                    for g in (stiff, mass):
                        g.set_timing(True)
                    stiff.eigen(4, mass=mass, block=6, pc=pc, rtol=1e-8, maxit=1000)
                    total, kernel, _ = stiff.last_timing()
                    for g in (stiff, mass):
                        g.set_timing(False)
                    say("p = %d, n = %d, nev 4, block 6, pc=%-8s batched %d: %4d iterations, reason %s, %d restarts, %d actions, %9.2f ms, %d launches (with timing on: %.2f ms, of which %.2f ms in the operators' kernels); lambda %s"
                        % (p, nv, pc, flag, out["iterations"], out["reason_name"], out["restarts"], out["actions"], ms, launches, total, kernel, np.array2string(out["lambda"][:4], precision=6)))
                stiff.set_batched_actions(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
