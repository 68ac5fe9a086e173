"""Dumps what the element kernels' sweeps produce, for a byte comparison between two builds of the library (IGX_LIB names the other one):
the cases of tests/test_gpu_sweep_accounting.py through System, Matrix, Vector, Function and Jacobian under IGXSetKernel 1 and 3, their
functionals, and the four Cahn-Hilliard drivers at p = 2 on 4 x 4 x 4 elements.  One file: per case a text line (case, kernel name,
launches or the refusal) followed by the matrix values, vectors and scalars as raw doubles.

  python scripts/dump_element_sweeps.py OUT.bin [--skip case,case]      write the dump
  python scripts/dump_element_sweeps.py --compare A.bin B.bin           list the cases whose records differ (exit status 1 if any)"""
import os
import struct
import sys

import numpy as np

for _d in ("tests", "oracle", ""):      # the cases and structs are the test module's
    sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", _d)))


def records(path):
    """{case: bytes of its record} of a dump"""
    blob, out, pos = open(path, "rb").read(), {}, 0
    while pos < len(blob):
        nh, nb = struct.unpack_from("<qq", blob, pos)
        head = blob[pos + 16:pos + 16 + nh].decode()
        out[head.split(" | ")[0]] = blob[pos:pos + 16 + nh + nb]
        pos += 16 + nh + nb
    return out


def compare(a, b):
    ra, rb = records(a), records(b)
    bad = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print("%d cases in %s, %d in %s, %d differ" % (len(ra), a, len(rb), b, len(bad)))
    for k in bad:
        print("  differs:", k)
    return 1 if bad else 0


def main(out_path, skip):
    import petiga_amd as P
    from test_gpu_sweep_accounting import A3, B3, C2, D1, E2, E3, FORMS, FUNCTIONALS, _engine, _two_faces
    out = open(out_path, "wb")
    ncases = 0

    def put(case, text, arrays):
        nonlocal ncases
        if case in skip:
            return
        head = (case + " | " + text).encode()
        body = b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)
        out.write(struct.pack("<qq", len(head), len(body)) + head + body)
        ncases += 1

    def run(case, eng, call, results):
        try:
            call()
            eng.synchronize()
            put(case, "%s | %d launches" % (eng.kernel_name(), eng.last_timing()[2]), [r() for r in results])
        except P.IGXError as e:
            put(case, "refused: %s" % e, [])

    shapes = dict(A3=A3, B3=B3, C2=C2, D1=D1, E2=E2, E3=E3)
    plan = [("poisson", "A3 B3 C2 D1 E2 E3"), ("mass2", "A3 C2"), ("elasticity", "A3 B3"), ("nitsche", "A3 B3 C2 D1 E3")]
    for form, names in plan:
        dof, builtin, source, struct_name, params, visits = FORMS[form]
        for sname in names.split():
            sh = shapes[sname]
            dim = len(sh["N"])
            for twin in ("built-in", "run-time"):
                if twin == "run-time" and source is None:
                    continue
                eng = _engine(dof, sh["p"], sh["N"], sh.get("periodic"), _two_faces(dim) if visits else ())
                if twin == "built-in":
                    eng.set_form(*builtin)
                else:
                    eng.set_form_source(source, struct_name % dim if "%d" in struct_name else struct_name, params)
                A, b, F = eng.create_mat(), eng.create_vec(), eng.create_vec()
                U = eng.create_vec().set(np.cos(0.37 * np.arange(b.n)))
                for kernel in (1, 3) if dim >= 2 else (1,):
                    eng.set_kernel(kernel)
                    tag = "%s %s %s kernel %d " % (form, twin, sname, kernel)
                    run(tag + "system", eng, lambda: eng.compute_system(A, b), [lambda: A.host(True), b.get])
                    run(tag + "matrix", eng, lambda: eng.compute_matrix(A), [lambda: A.host(True)])
                    run(tag + "vector", eng, lambda: eng.compute_vector(b), [b.get])
                    run(tag + "function", eng, lambda: eng.compute_function(U, F), [F.get])
                    run(tag + "jacobian", eng, lambda: eng.compute_jacobian(U, A), [lambda: A.host(True)])
    for sname in ("A3", "C2", "D1"):
        sh = shapes[sname]
        dim = len(sh["N"])
        for faces in ((), _two_faces(dim)):
            eng = _engine(1, sh["p"], sh["N"], None, faces)
            U = eng.create_vec().set(np.cos(0.37 * np.arange(eng.create_vec().n)))
            for kernel in (1, 3) if dim >= 2 else (1,):
                eng.set_kernel(kernel)
                tag = "functional %s faces %d kernel %d " % (sname, len(faces), kernel)
                box = {}
                run(tag + "volume", eng, lambda: box.update(v=eng.compute_scalar("volume")), [lambda: box["v"]])
                run(tag + "x2err", eng, lambda: box.update(e=eng.compute_scalar("x2err", U)), [lambda: box["e"]])
                run(tag + "UserMeasures", eng, lambda: box.update(m=eng.compute_scalar_source(FUNCTIONALS, "UserMeasures<%d>" % dim, 3, U, (0.75,))), [lambda: box["m"]])
                run(tag + "UserX2Err", eng, lambda: box.update(x=eng.compute_scalar_source(FUNCTIONALS, "UserX2Err<%d>" % dim, 1, U)), [lambda: box["x"]])
    # Cahn-Hilliard (second-order shape features, fields at the points): Function, Jacobian, IFunction, IJacobian
    eng = _engine(1, 2, (4, 4, 4))
    eng.set_form("cahnhilliard", (3.0, 1.0 / (4 * np.pi ** 2 * 16)))
    A, F = eng.create_mat(), eng.create_vec()
    U = eng.create_vec().set(0.3 * np.cos(0.37 * np.arange(F.n)))
    V = eng.create_vec().set(0.1 * np.sin(0.21 * np.arange(F.n)))
    for kernel in (1, 3):
        eng.set_kernel(kernel)
        tag = "cahnhilliard p2 4x4x4 kernel %d " % kernel
        run(tag + "function", eng, lambda: eng.compute_function(U, F), [F.get])
        run(tag + "jacobian", eng, lambda: eng.compute_jacobian(U, A), [lambda: A.host(True)])
        run(tag + "ifunction", eng, lambda: eng.compute_ifunction(2.0, V, 0.0, U, F), [F.get])
        run(tag + "ijacobian", eng, lambda: eng.compute_ijacobian(2.0, V, 0.0, U, A), [lambda: A.host(True)])
    out.close()
    print("%d cases, %d bytes -> %s" % (ncases, os.path.getsize(out_path), out_path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    skip = set(sys.argv[3].split(",")) if len(sys.argv) == 4 and sys.argv[2] == "--skip" else set()
    sys.exit(main(sys.argv[1], skip))
