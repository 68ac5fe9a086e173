"""Dumps what the Gram walks produce, for a byte comparison between two builds of the library (IGX_LIB names the other one): the cases of
tests/test_gpu_walk_accounting.py (the p = 2 patch walk's default is not bit-repeatable by design and is dumped with IGX_PATCH=0; its own
tests cover it), and a fix table, boundary loads on two faces, a run-time Gram form and a run-time Tangent.  One file: per case a text
line (case, kernel name, launches, passes, or the refusal) followed by the matrix values and vectors as raw doubles.

  python scripts/dump_pencil_walks.py OUT.bin                      write the dump
  python scripts/dump_pencil_walks.py --compare A.bin B.bin        list the cases whose records differ (exit status 1 if any)"""
import os
import struct
import sys

import numpy as np

for _d in ("tests", "oracle", "scripts", ""):      # the structs are the test modules'
    sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", _d)))

from dump_element_sweeps import compare      # noqa: E402  (the same record format)

SWITCHES = ("IGX_PATCH", "IGX_PATCH3", "IGX_OVERLAP", "IGX_FUSE_RESID")


def main(out_path):
    import petiga_amd as P
    from petiga_amd.geometry import greville
    from test_gpu_walk_accounting import CH
    from test_rtc_boundary_scalar import BRATU3_WALK
    from test_rtc_forms import USER_POISSON
    out = open(out_path, "wb")
    ncases = 0

    def put(case, text, arrays):
        nonlocal ncases
        head = (case + " | " + text).encode()
        body = b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)
        out.write(struct.pack("<qq", len(head), len(body)) + head + body)
        ncases += 1

    def run(case, eng, call, results):
        try:
            call()
            eng.synchronize()
            put(case, "%s | %d launches | %d passes" % (eng.kernel_name(), eng.last_timing()[2], eng.face_passes()), [r() for r in results])
        except P.IGXError as e:
            put(case, "refused: %s" % e, [])

    def engine(p, N, env=None, comm=None, mapped=False):
        for k in SWITCHES:      # the switches are read when the engine is created
            os.environ.pop(k, None)
        os.environ.update(env or {})
        eng = P.IGX(3, 1)
        if comm:
            eng.set_comm(*comm)
        for i in range(3):
            eng.axis_uniform(i, p, N[i])
        eng.setup()
        if mapped:
            gv = [greville(np.concatenate([[0.0] * (p + 1), np.arange(1, n) / n, [1.0] * (p + 1)]), p) for n in N]
            mesh = np.meshgrid(*gv[::-1], indexing="ij")[::-1]
            X = np.stack([m.copy() for m in mesh], axis=-1)
            X[..., 0] += 0.05 * np.sin(2 * np.pi * mesh[1]); X[..., 1] += 0.05 * np.sin(2 * np.pi * mesh[2])
            eng.set_geometry(X.reshape(-1, 3))
        return eng

    def gram(case, eng, drivers=("system", "matrix")):
        A, b = eng.create_mat(), eng.create_vec()
        if "system" in drivers:
            run(case + " system", eng, lambda: eng.compute_system(A, b), [lambda: A.host(True), b.get])
        if "matrix" in drivers:
            run(case + " matrix", eng, lambda: eng.compute_matrix(A), [lambda: A.host(True)])

    def dirichlet(eng):
        eng.set_boundary_value(0, 0, 0, 2.0); eng.set_boundary_value(2, 1, 0, -1.0); eng.set_boundary_value(1, 0, 0, 0.5)

    # the walks of the accounting test, without and with Dirichlet values
    for bc in (False, True):
        tag = " dirichlet" if bc else ""
        for name, p, N, env, mapped in (("p3 pencil 8x5x4", 3, (8, 5, 4), None, False), ("p3 patch 8x9x5", 3, (8, 9, 5), {"IGX_PATCH3": "2"}, False),
                                        ("p2 pencil 8x5x4", 2, (8, 5, 4), {"IGX_PATCH": "0"}, False), ("p2 pencil 8x4x3", 2, (8, 4, 3), {"IGX_PATCH": "0"}, False),
                                        ("p3 walk 2 5x4x8", 3, (5, 4, 8), None, False), ("p3 element 5x4x3", 3, (5, 4, 3), None, False),
                                        ("p2 mapped 8x5x4", 2, (8, 5, 4), None, True), ("p3 mapped 9x5x4", 3, (9, 5, 4), None, True)):
            eng = engine(p, N, env, mapped=mapped)
            if bc:
                dirichlet(eng)
            eng.set_form("poisson")
            gram(name + tag, eng)
    # a fix table, boundary loads on two faces
    for name, p, N, env, mapped in (("p3 8x5x4", 3, (8, 5, 4), None, False), ("p2 8x5x4", 2, (8, 5, 4), {"IGX_PATCH": "0"}, False), ("p2 mapped 8x5x4", 2, (8, 5, 4), None, True)):
        eng = engine(p, N, env, mapped=mapped)
        dirichlet(eng)
        eng.set_form("poisson")
        n = eng.create_vec().n
        eng.set_fixtable(eng.create_vec().set(0.63 + 0.04 * np.cos(0.37 * np.arange(n))))
        gram("fix table " + name, eng, ("system",))
        eng = engine(p, N, env, mapped=mapped)
        eng.set_boundary_value(0, 0, 0, 2.0)
        eng.set_boundary_load(1, 1, 0, 0.75); eng.set_boundary_load(2, 0, 0, -0.5)
        eng.set_form("poisson")
        gram("boundary loads " + name, eng, ("system",))
    # a run-time Gram form and a run-time Tangent
    for name, p, N, mapped in (("p3 8x5x4", 3, (8, 5, 4), False), ("p2 8x5x4", 2, (8, 5, 4), False), ("p3 mapped 8x4x5", 3, (8, 4, 5), True)):
        eng = engine(p, N, mapped=mapped)
        dirichlet(eng)
        eng.set_form_source(USER_POISSON, "UserPoisson", (1.0,))
        gram("run-time UserPoisson " + name, eng)
    for name, p, N, mapped in (("p2 9x4x5", 2, (9, 4, 5), False), ("p3 8x4x4", 3, (8, 4, 4), False), ("p2 mapped 9x4x5", 2, (9, 4, 5), True)):
        eng = engine(p, N, mapped=mapped)
        dirichlet(eng)
        eng.set_form_source(BRATU3_WALK, "UserBratu3Walk", (3.5,))
        J, F = eng.create_mat(), eng.create_vec()
        U = eng.create_vec().set(0.3 * np.cos(0.37 * np.arange(F.n)))
        V = eng.create_vec().set(0.1 * np.sin(0.21 * np.arange(F.n)))
        run("run-time UserBratu3Walk %s jacobian" % name, eng, lambda: eng.compute_jacobian(U, J), [lambda: J.host(True)])
        run("run-time UserBratu3Walk %s ijacobian" % name, eng, lambda: eng.compute_ijacobian(4.0, V, 0.0, U, J), [lambda: J.host(True)])
    # the built-in Tangents: Cahn-Hilliard and Bratu, the fused Residual, a mapped net
    for form, params in (("cahnhilliard", CH), ("bratu", (3.5,))):
        for name, p, N, env, mapped in (("p2 8x5x4", 2, (8, 5, 4), None, False), ("p2 fused 8x5x4", 2, (8, 5, 4), {"IGX_FUSE_RESID": "1"}, False),
                                        ("p3 8x5x4", 3, (8, 5, 4), None, False), ("p2 mapped 8x5x4", 2, (8, 5, 4), None, True)):
            eng = engine(p, N, env, mapped=mapped)
            dirichlet(eng)
            eng.set_form(form, params)
            J, F = eng.create_mat(), eng.create_vec()
            U = eng.create_vec().set(0.63 + 0.05 * np.cos(0.37 * np.arange(F.n)))
            V = eng.create_vec().set(0.1 * np.sin(0.21 * np.arange(F.n)))
            tag = "%s %s " % (form, name)
            run(tag + "jacobian", eng, lambda: eng.compute_jacobian(U, J), [lambda: J.host(True)])
            run(tag + "ijacobian", eng, lambda: eng.compute_ijacobian(2.0, V, 0.0, U, J), [lambda: J.host(True)])
            run(tag + "function + jacobian", eng, lambda: eng.compute_function_jacobian(U, F, J), [lambda: J.host(True), F.get])
            run(tag + "ifunction + ijacobian", eng, lambda: eng.compute_ifunction_ijacobian(2.0, V, 0.0, U, F, J), [lambda: J.host(True), F.get])
    # rank 0 of 2 with a transport that moves nothing: the upper face of axis 2 first, and one pass
    for overlap in ("1", "0"):
        for name, p, N, mapped in (("p3 8x5x16", 3, (8, 5, 16), False), ("p2 8x5x12", 2, (8, 5, 12), False), ("p3 mapped 8x5x16", 3, (8, 5, 16), True)):
            eng = engine(p, N, {"IGX_OVERLAP": overlap}, comm=(2, 0), mapped=mapped)
            eng.set_boundary_value(0, 0, 0, 2.0)
            eng.set_form("poisson")
            eng.comm_init_transport(lambda send, recv: None)
            gram("rank 0 of 2, IGX_OVERLAP=%s, %s" % (overlap, name), eng)
    out.close()
    print("%d cases, %d bytes -> %s" % (ncases, os.path.getsize(out_path), out_path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(main(sys.argv[1]))
