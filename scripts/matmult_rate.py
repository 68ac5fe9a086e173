"""Times IGXMatMult next to the matrix-free action it can stand in for, on an MI355X (profiles/matmult.txt):
  cases     Poisson p = 1, 2, 3 on 64^3 and 128^3 elements (u = 1 on every face), Elasticity3D p = 2 on 64^3
  per case  one IGXMatMult with the column of an entry from the axis tables (IGX_MATMULT_INDEX=0) and from bcolidx (=1);
            the bytes that product must move -- the values, bcolidx where it is read, x and y once each -- and those bytes over the
            6.3 TB/s the chip's memory achieves (MI355X: 8 TB/s peak, 6.29 TB/s measured for a float4 copy) as the floor, with the ratio to it;
            the matching IGXComputeMatrixAction
  Poisson   the time per iteration of IGXMatSolve against IGXSolve, CG with Jacobi, over a fixed number of iterations (rtol = atol = 0)
Method: every figure is the wall time of a window of calls between two stream synchronisations, per call; a window holds as many calls as
fill `--window` seconds (0.2 by default; `--reps` at the least), counted from a first timed batch per version; `rounds` such windows per
version, the versions of a comparison alternating inside a round; the median with the smallest and the largest window.  Ten untimed calls
warm every version up first.  A figure is what a caller of the Python view sees per call in a stream of calls: the kernel and, where the
kernel is shorter, the enqueue of one call through ctypes (a few us); the launches are asynchronous, so at the sizes here the device sets
the pace (the times scale with the matrix from 64^3 to 128^3).  A matrix whose bytes fit the 256 MiB Infinity Cache is re-read from it, not from HBM: such a case may run UNDER the floor,
and the table says which cases those are.

    python scripts/matmult_rate.py [--sizes 64 128] [--window 0.2] [--reps 20] [--rounds 7] [--iterations 50] [--out profiles/matmult.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.3e12          # bytes per second achievable
LLC = 256 * 2 ** 20   # the Infinity Cache


def batch(g, call, reps):
    g.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    g.synchronize()
    return (time.perf_counter() - t0) / reps


def windows(engines, calls, reps, rounds, window):
    """per call of every version: (median, min, max, calls per window) over `rounds` windows of at least `window` seconds and `reps` calls; the
    versions alternate inside a round"""
    n = []
    for g, call in zip(engines, calls):
        for _ in range(10):
            call()
        n.append(max(reps, int(window / max(batch(g, call, reps), 1e-9)) + 1))
    t = [[] for _ in calls]
    for _ in range(rounds):
        for k, (g, call) in enumerate(zip(engines, calls)):
            t[k].append(batch(g, call, n[k]))
    return [(statistics.median(v), min(v), max(v), n[k]) for k, v in enumerate(t)]


def build(form, dof, p, N, index):
    import petiga_amd as P
    os.environ["IGX_MATMULT_INDEX"] = str(index)      # read when the IGX is created
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, N)
    g.setup()
    for d in range(3):
        for s in range(2):
            for f in range(dof):
                g.set_boundary_value(d, s, f, 1.0 if dof == 1 else 0.0)
    g.set_form(form, () if form == "poisson" else (1.5, 0.8))
    A, b = g.create_mat(), g.create_vec()
    g.compute_system(A, b)
    g.synchronize()
    return g, A, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.2, help="seconds a timed window lasts at the least")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "matmult.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this script measures on a GPU: none found"
    import petiga_amd as P
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("IGXMatMult against IGXComputeMatrixAction; %s" % P.device_info())
    say("wall time per call between two synchronisations (the kernel, or the enqueue of a call where that is longer): median (min .. max) of %d windows of at least %.1f s and %d calls, the versions alternating; floor = bytes / 6.3 TB/s" % (a.rounds, a.window, a.reps))
    say()
    cases = [("poisson", 1, p, N) for N in a.sizes for p in (1, 2, 3)] + [("elasticity", 3, 2, a.sizes[0])]
    rng = np.random.default_rng(7)
    for form, dof, p, N in cases:
        (g0, A0, b0), (g1, A1, b1) = build(form, dof, p, N, 0), build(form, dof, p, N, 1)
        n = b0.n
        xh = rng.standard_normal(n)
        x0, y0, x1, y1, ya = g0.create_vec().set(xh), g0.create_vec(), g1.create_vec().set(xh), g1.create_vec(), g0.create_vec()
        (tt, tb, ta) = windows([g0, g1, g0], [lambda: A0.mult(x0, y0), lambda: A1.mult(x1, y1), lambda: g0.compute_matrix_action(x0, ya)], a.reps, a.rounds, a.window)
        A0.mult(x0, y0)
        name_t = g0.kernel_name()
        A1.mult(x1, y1)
        name_b = g1.kernel_name()
        # the variants live on two engines with an assembly each; where the assemblies differ in their last bits (the p = 2 patch walk does not
        # order its adds) the products are not comparable bit for bit
        same = "the same bits" if np.array_equal(y0.get(), y1.get()) else "DIFFERENT bits" if np.array_equal(A0.host(values_only=True), A1.host(values_only=True)) else "different bits of two assemblies that differ themselves"
        vals, idx, vecs = 8 * A0.nblocks * dof * dof, 4 * A0.nblocks, 16 * n
        say("%s p = %d, %d^3 elements, bs = %d: %d rows, %d blocks, values %.1f MB%s" % (form, p, N, dof, A0.nbrows, A0.nblocks, vals / 1e6, " (fits the Infinity Cache: re-read from it)" if vals < LLC else ""))
        for label, t, nbytes, kname in (("tables", tt, vals + vecs, name_t), ("bcolidx", tb, vals + idx + vecs, name_b)):
            floor = nbytes / HBM
            say("  IGXMatMult, columns from %-8s %9.1f us (%9.1f .. %9.1f; %5d calls per window)   bytes %10.1f MB   floor %8.1f us   time / floor %5.2f   %6.2f TB/s   %s"
                % (label + ":", t[0] * 1e6, t[1] * 1e6, t[2] * 1e6, t[3], nbytes / 1e6, floor * 1e6, t[0] / floor, nbytes / t[0] / 1e12, kname))
        say("  IGXComputeMatrixAction:           %9.1f us (%9.1f .. %9.1f)   action / product (tables) %5.2f; the two index variants give %s" % (ta[0] * 1e6, ta[1] * 1e6, ta[2] * 1e6, ta[0] / tt[0], same))
        if form == "poisson":
            k = a.iterations
            xs, xm = g0.create_vec(), g0.create_vec()
            ts, tm = windows([g0, g0], [lambda: g0.solve(b0, xs.fill(0.0), pc="jacobi", rtol=0.0, atol=0.0, maxit=k), lambda: A0.solve(b0, xm.fill(0.0), pc="jacobi", rtol=0.0, atol=0.0, maxit=k)], 1, a.rounds, a.window)
            say("  CG with Jacobi, %d iterations: IGXSolve %9.1f us per iteration (%9.1f .. %9.1f), IGXMatSolve %9.1f us (%9.1f .. %9.1f): matrix-free / matrix %5.2f"
                % (k, ts[0] / k * 1e6, ts[1] / k * 1e6, ts[2] / k * 1e6, tm[0] / k * 1e6, tm[1] / k * 1e6, tm[2] / k * 1e6, ts[0] / tm[0]))
        say()
        del A0, A1, b0, b1, x0, y0, x1, y1, ya, g0, g1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
