"""A SHA-256 of the result bytes of every matrix-free pass that tests/test_gpu_matfree_routing.py runs (the action, the action on a block,
the diagonal and the point-block diagonal; Poisson at p = 2, 3, 4, 6 with and without a geometry, and a run-time struct), of a 5-iteration
IGXSolve with Jacobi and of one IGXEigenSolve with IGXSetBatchedActions 0 and 1 at 4 elements per axis.  The passes use no atomics and
walk the colours in a fixed order, so two builds of the library that route the same calls to the same kernels print the same lines:
run it on both (IGX_LIB=<the other build>) and compare (profiles/matfree_routing.txt).

    python scripts/matfree_fingerprint.py [--out file]"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import petiga_amd as P
    import test_gpu_matfree_routing as R
    lines = ["library: %s; %s" % (os.environ.get("IGX_LIB", "this tree's"), P.device_info())]
    for case in R.RUNS:
        form, p, geo, kind = case.values
        g = R._form(R._space(p, R.SIZES[p], geometry=geo), form)
        for d in range(3):
            g.set_boundary_value(d, 0, 0, 0.0)
        Y = R._call(g, kind)
        lines.append("%-40s %s  %s, %d launches" % (case.id, digest(Y), g.kernel_name(), g.last_timing()[2]))
    for p in (2, 3):
        stiff, mass = R._form(R._space(p, 4), "poisson"), R._form(R._space(p, 4), "mass")
        for g in (stiff, mass):
            for d in range(3):
                for s in range(2):
                    g.set_boundary_value(d, s, 0, 0.0)
        n = stiff.create_vec().n
        b, x = stiff.create_vec().set(np.random.default_rng(11).standard_normal(n)), stiff.create_vec()
        info = stiff.solve(b, x, method="cg", pc="jacobi", rtol=1e-30, maxit=5, history=True)
        stiff.synchronize()
        lines.append("%-40s %s  %d iterations, %s" % ("solve-cg-jacobi-p%d" % p, digest([x.get(), info["history"]]), info["iterations"], stiff.kernel_name()))
        for flag in (0, 1):
            stiff.set_batched_actions(flag)
            out = stiff.eigen(2, mass=mass, block=4, pc="jacobi", rtol=1e-8, maxit=20, history=True)
            stiff.synchronize()
            lines.append("%-40s %s  %d iterations, %d actions, %d launches" % ("eigen-p%d-batched%d" % (p, flag), digest([out["lambda"], out["resid"], out["history"]] + [v.get() for v in out["X"]]),
                                                                                out["iterations"], out["actions"], stiff.last_timing()[2]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
