"""Nested iteration with IGXTransfer: Bratu (lambda = 3.5) at p = 2 with Dirichlet values on six faces.  Solve on N/2 ^3 elements from zero,
prolong the state to N^3 elements (IGXTransferProlong), and run IGXSolveNonlinear there from the prolonged state; beside it the same fine
solve from zero.  Reports Newton iterations, linear iterations and the host's clock of each solve.  BiCGStab with the Jacobi
preconditioner to lin_rtol = 1e-6, backtracking line search, rtol = 1e-8 (the case of scripts/time_newton.py).
Appends to the output file (profiles/transfer.txt).

    python scripts/nested_newton.py [--size 64] [--out profiles/transfer.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bratu(P, n):
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, n)
    g.setup()
    for d in range(3):
        for s in range(2):
            g.set_boundary_value(d, s, 0, 0.1 * d * s)
    g.set_form("bratu", (3.5,))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer.txt"))
    a = ap.parse_args()
    import petiga_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kw = dict(method="bicgstab", pc="jacobi", lin_rtol=1e-6, rtol=1e-8, linesearch="bt")
    c, f = bratu(P, a.size // 2), bratu(P, a.size)
    t = f.transfer(c)

    def solve(g, x):
        g.synchronize()
        t0 = time.perf_counter()
        info = g.solve_nonlinear(x, **kw)
        g.synchronize()
        return info, (time.perf_counter() - t0) * 1e3

    def row(label, info, ms):
        say("  %-44s reason %s, %d Newton iterations, linear %s = %d, %d function evaluations, %.1f ms" % (
            label, info["reason_name"], info["iterations"], [int(k) for k in info["linear_its"]], sum(int(k) for k in info["linear_its"]), info["function_evaluations"], ms))

    say("nested iteration, Bratu p = 2, %d^3 -> %d^3 elements (n = %d -> %d)" % (a.size // 2, a.size, c.create_vec().n, f.create_vec().n))
    for g in (c, f):                                     # warm every kernel once
        solve(g, g.create_vec())
    xc, xf, x0 = c.create_vec(), f.create_vec(), f.create_vec()
    info_c, ms_c = solve(c, xc)
    row("coarse solve from zero", info_c, ms_c)
    f.synchronize()
    t0 = time.perf_counter()
    t.prolong(xc, xf)
    f.synchronize()
    ms_p = (time.perf_counter() - t0) * 1e3
    say("  prolongation: %.3f ms (first call: uploads the tables); %s" % (ms_p, f.kernel_name()))
    info_n, ms_n = solve(f, xf)
    row("fine solve from the prolonged coarse state", info_n, ms_n)
    info_0, ms_0 = solve(f, x0)
    row("fine solve from zero", info_0, ms_0)
    diff = xf.axpby(-1.0, x0, 1.0).norm() / max(x0.norm(), 1e-300)
    say("  the two fine solutions differ by %.2e relative; nested: coarse + prolongation + fine = %.1f ms against %.1f ms from zero" % (diff, ms_c + ms_p + ms_n, ms_0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
