"""IGXMultigrid on a NURBS-mapped Poisson problem, all faces Dirichlet, at p = 2 and p = 3 on N/4 ^3 -> N/2 ^3 -> N^3 elements: iterations and
time to rtol = 1e-8 of CG preconditioned by the V-cycle (Chebyshev-Jacobi, fast diagonalisation once as the coarse solve), by Jacobi and by
fast diagonalisation; the time of one cycle, split by level; and one fused Chebyshev step (mg_cheb_step) against the four IGXVec kernels it
replaces at the finest length, both taken in the same run between device events, alternating (IGXMultigridMeasureStep).
The geometry of every level is the knot refinement of the coarsest rational net: the homogeneous net is carried up by the library's own
IGXTransfer on a four-field space (knot insertion IS the prolongation of the control points).  Times are the host's clock around calls that
end in a synchronise, after one warm-up call each.  Appends to the output file (profiles/multigrid.txt).

    python scripts/multigrid_rate.py [--size 128] [--degrees 2 3] [--power-its 40] [--out profiles/multigrid.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALL6 = [(d, s) for d in range(3) for s in range(2)]


def space(P, p, n, dof=1):
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, n)
    g.setup()
    return g


def nets(P, p, sizes, amp=0.05, seed=2):
    """(X, W) per level: a warped rational net on the coarsest Greville grid, refined by the transfer of a four-field space"""
    from petiga_amd.geometry import greville
    rng = np.random.default_rng(seed)
    carriers = [space(P, p, n, dof=4) for n in sizes]
    n0 = sizes[0] + p
    U = np.r_[[0.0] * p, np.linspace(0.0, 1.0, sizes[0] + 1), [1.0] * p]
    g = greville(U, p)
    mesh = np.meshgrid(g, g, g, indexing="ij")[::-1]           # mesh[i] varies along axis i, arrays [n2][n1][n0]
    X = np.stack([m.copy() for m in mesh], axis=-1)
    ph = rng.uniform(0, 2 * np.pi, size=(3, 3))
    for i in range(3):
        for j in range(3):
            if i != j:
                X[..., i] += amp / 3 * np.sin(2 * np.pi * mesh[j] + ph[i, j]) * (0.5 + 0.5 * mesh[i])
    W = rng.uniform(0.8, 1.2, size=(n0, n0, n0))
    Pw = np.concatenate([X * W[..., None], W[..., None]], axis=-1).reshape(-1)
    out, v = [], carriers[0].create_vec().set(Pw)
    for l, c in enumerate(carriers):
        if l:
            t = c.transfer(carriers[l - 1])
            v = t.prolong(v, c.create_vec())
            c.synchronize()
            t.close()
        flat = v.get().reshape(-1, 4)
        out.append((flat[:, :3] / flat[:, 3:4], flat[:, 3].copy()))
    return out


def level(P, p, n, geometry):
    g = space(P, p, n)
    g.set_geometry(*geometry)
    for d, s in ALL6:
        g.set_boundary_value(d, s, 0, 0.0)
    g.set_form("poisson")
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--degrees", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--degree", type=int, default=2, help="Chebyshev steps per smoothing")
    ap.add_argument("--power-its", type=int, default=40, help="power iterations for lambda: 10 underestimate it by 15 %% from 64^3 elements on, more than hi = 1.1 covers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multigrid.txt"))
    a = ap.parse_args()
    import petiga_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(g, call, repeat=1):
        call()                                               # warm-up: every kernel and every table of the call
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeat):
            out = call()
        g.synchronize()
        return out, (time.perf_counter() - t0) * 1e3 / repeat

    sizes = [a.size // 4, a.size // 2, a.size]
    say("multigrid on NURBS-mapped Poisson, %s elements per axis, rtol = 1e-8, Chebyshev-Jacobi %d on [0.1, 1.1] lambda (%d power iterations), coarse fastdiag x1; %s" % (
        " -> ".join(str(n) for n in sizes), a.degree, a.power_its, P.device_info() if hasattr(P, "device_info") else ""))
    for p in a.degrees:
        levels = [level(P, p, n, geo) for n, geo in zip(sizes, nets(P, p, sizes))]
        fine = levels[-1]
        n = fine.create_vec().n
        b = fine.create_vec()
        fine.compute_vector(b)
        for g in (levels[0], fine):
            g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
        t0 = time.perf_counter()
        mg = fine.multigrid(levels[:-1], degree=a.degree, power_its=a.power_its, coarse=dict(pc="fastdiag", maxit=0)).setup()
        setup_ms = (time.perf_counter() - t0) * 1e3
        say("p = %d, n = %s: multigrid set-up %.1f ms, lambda %s" % (p, " -> ".join(str(mg.info(l)["n"]) for l in range(3)), setup_ms, ["%.4f" % mg.info(l)["lambda_"] for l in range(3)]))
        x = fine.create_vec()
        rows = [("MG-PCG", lambda: mg.solve(b, x.fill(0.0), rtol=1e-8, maxit=400)),
                ("Jacobi-PCG", lambda: fine.solve(b, x.fill(0.0), pc="jacobi", rtol=1e-8, maxit=5000)),
                ("fastdiag-PCG", lambda: fine.solve(b, x.fill(0.0), pc="fastdiag", rtol=1e-8, maxit=5000))]
        for label, call in rows:
            info, ms = timed(fine, call)
            say("  %-13s %4d iterations, reason %s, %9.2f ms, %d launches" % (label, info["iterations"], info["reason_name"], ms, fine.last_timing()[2]))
        # one cycle, split by level: the cycles of the nested hierarchies (fastdiag x1 on their coarsest level) and their differences
        r, z = fine.create_vec().set(np.random.default_rng(1).standard_normal(n)), fine.create_vec()
        _, whole = timed(fine, lambda: mg.apply(r, z), repeat=20)
        say("  one cycle on 3 levels: %.3f ms, launches per level %s" % (whole, [mg.info(l)["launches"] for l in range(3)]))
        mid = levels[1]
        m2 = mid.multigrid(levels[:1], degree=a.degree, power_its=a.power_its, coarse=dict(pc="fastdiag", maxit=0)).setup()
        r2, z2 = mid.create_vec().set(np.random.default_rng(2).standard_normal(mid.create_vec().n)), mid.create_vec()
        _, lower = timed(mid, lambda: m2.apply(r2, z2), repeat=20)
        r0, z0 = levels[0].create_vec().set(np.random.default_rng(3).standard_normal(levels[0].create_vec().n)), levels[0].create_vec()
        _, coarse = timed(levels[0], lambda: levels[0].fast_diag_apply(r0, z0), repeat=20)
        say("    level 2 (smoother, residuals, transfers): %.3f ms; level 1: %.3f ms; level 0 (fastdiag x1): %.3f ms" % (whole - lower, lower - coarse, coarse))
        m2.close()
        fused, split = mg.measure_step(2, reps=200, rounds=9)
        say("  one Chebyshev step at n = %d: fused sweep %.4f ms (median of 9 rounds of 200; %.4f .. %.4f), the four IGXVec kernels %.4f ms (%.4f .. %.4f): %.2fx; %.0f GB/s over 8 doubles per entry"
            % (n, np.median(fused), fused.min(), fused.max(), np.median(split), split.min(), split.max(), np.median(split) / np.median(fused), 64.0 * n / np.median(fused) * 1e-6))
        mg.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
