"""Times IGXMatMultBlock next to what it can stand in for, on an MI355X (profiles/matmult_block.txt):
  product   Poisson p = 1, 2, 3 on 64^3 and 128^3 elements (u = 1 on every face), Elasticity3D p = 2 on 64^3; for nx = 2, 4, 8, 16:
            one IGXMatMultBlock on nx columns, nx calls of IGXMatMult, and one IGXComputeMatrixActionBlock on the same columns
  solve     IGXMatEigenSolve against IGXEigenSolve, without and with IGXSetBatchedActions, on the two cases README quotes for the eigen
            solve: Poisson + Mass on 64^3 elements, nev 4, block 6, p = 3 without a preconditioner and p = 2 with fast diagonalisation
Method (scripts/matmult_rate.py's): every figure is the wall time of a window of calls between two stream synchronisations, per call; a
window holds as many calls as fill `--window` seconds (`--reps` at the least), counted from a first timed batch per version; `rounds` such
windows per version, the versions of a comparison alternating inside a round; the median with the smallest and the largest window.  Ten
untimed calls warm every version up first (the solves: one whole solve).  No figure here is a gate: every ratio is written down as found.

    python scripts/matmult_block_rate.py [--sizes 64 128] [--window 0.2] [--reps 10] [--rounds 7] [--out profiles/matmult_block.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matmult_rate import batch, windows      # noqa: E402  (the same windows as the single product's figures)

NX = (2, 4, 8, 16)


def space(P, form, dof, p, N, value):
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, N)
    g.setup()
    for d in range(3):
        for s in range(2):
            for f in range(dof):
                g.set_boundary_value(d, s, f, value)
    g.set_form(form, (1.5, 0.8) if form == "elasticity" else ())
    return g


def assembled(g):
    A = g.create_mat()
    g.compute_system(A, g.create_vec())
    g.synchronize()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.2, help="seconds a timed window lasts at the least")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--solve-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "matmult_block.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this script measures on a GPU: none found"
    import petiga_amd as P
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("IGXMatMultBlock against nx IGXMatMult and IGXComputeMatrixActionBlock; IGXMatEigenSolve against IGXEigenSolve; %s" % P.device_info())
    say("wall time per call between two synchronisations: median (min .. max) of %d windows of at least %.1f s and %d calls, the versions alternating" % (a.rounds, a.window, a.reps))
    say()
    rng = np.random.default_rng(7)
    cases = [("poisson", 1, p, N) for N in a.sizes for p in (1, 2, 3)] + [("elasticity", 3, 2, a.sizes[0])]
    for form, dof, p, N in cases:
        g = space(P, form, dof, p, N, 1.0 if dof == 1 else 0.0)
        A = assembled(g)
        n = A.nbrows * dof
        X = [g.create_vec().set(rng.standard_normal(n)) for _ in range(max(NX))]
        Y = [g.create_vec() for _ in range(max(NX))]
        say("%s p = %d, %d^3 elements, bs = %d: %d rows, values %.1f MB, chunks of NC = %d" % (form, p, N, dof, A.nbrows, 8 * A.nblocks * dof * dof / 1e6, P.mat_mult_block_plan(dof, 48)[0]))
        for nx in NX:
            def singles():
                for j in range(nx):
                    A.mult(X[j], Y[j])
            tb, ts, ta = windows([g, g, g], [lambda: A.mult_block(X[:nx], Y[:nx]), singles, lambda: g.compute_matrix_action_block(X[:nx], Y[:nx])], a.reps, a.rounds, a.window)
            A.mult_block(X[:nx], Y[:nx])
            say("  nx = %2d (launches %s): block %9.1f us (%9.1f .. %9.1f)   %2d x IGXMatMult %9.1f us (%9.1f .. %9.1f)   matrix-free block action %9.1f us (%9.1f .. %9.1f)   singles / block %5.2f   action block / block %5.2f   %s"
                % (nx, P.mat_mult_block_plan(dof, nx), tb[0] * 1e6, tb[1] * 1e6, tb[2] * 1e6, nx, ts[0] * 1e6, ts[1] * 1e6, ts[2] * 1e6, ta[0] * 1e6, ta[1] * 1e6, ta[2] * 1e6,
                   ts[0] / tb[0], ta[0] / tb[0], g.kernel_name()))
        say()
        flush()
        del A, X, Y, g
    # the eigen solve on README's two cases
    for p, pc in ((3, "none"), (2, "fastdiag")):
        N = a.sizes[0]
        stiff, mass = space(P, "poisson", 1, p, N, 0.0), space(P, "mass", 1, p, N, 0.0)
        if pc == "fastdiag":
            stiff.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
        K, M = assembled(stiff), assembled(mass)
        kw = dict(mass=mass, block=6, pc=pc, rtol=1e-8, maxit=1000)

        def matfree(flag):
            def run():
                stiff.set_batched_actions(flag)
                r = stiff.eigen(4, **kw)
                stiff.set_batched_actions(0)
                return r
            return run
        runs = [lambda: K.eigen(4, mass=M, block=6, pc=pc, rtol=1e-8, maxit=1000), matfree(0), matfree(1)]
        outs = [r() for r in runs]      # the warm-up: one whole solve of each
        t = [[] for _ in runs]
        for _ in range(a.solve_rounds):
            for k, r in enumerate(runs):
                t[k].append(batch(stiff, r, 1))
        med = [statistics.median(v) for v in t]
        say("Poisson + Mass p = %d, %d^3 elements, nev 4, block 6, pc = %s: median (min .. max) of %d solves, alternating" % (p, N, pc, a.solve_rounds))
        for label, o, v, m_ in zip(("IGXMatEigenSolve", "IGXEigenSolve", "IGXEigenSolve, batched actions"), outs, t, med):
            say("  %-32s %9.1f ms (%9.1f .. %9.1f)   %3d iterations, reason %s, lambda_1 %.10f   time / IGXMatEigenSolve %5.2f"
                % (label + ":", m_ * 1e3, min(v) * 1e3, max(v) * 1e3, o["iterations"], o["reason_name"], o["lambda"][0], m_ / med[0]))
        say()
        flush()
        del K, M, stiff, mass


if __name__ == "__main__":
    main()
