"""IGXMatMultBlock and IGXMatEigenSolve in the C ABI (include/petiga_amd.h) and their Python view, on a machine without a GPU:
  exports       declared, exported and bound with the header's arguments; Mat.mult_block and Mat.eigen exist
  refusals      a null argument answers first, with IGX_ERR_ARG_WRONG under the call's name, before anything touches a device (every later
                refusal needs a matrix, i.e. a device: tests/test_gpu_mat_mult_block.py, tests/test_gpu_mat_eigen.py)
  kernels       every mat_mult_block instantiation the launcher can reach compiles for gfx950 with 16-byte loads, no atomics and no scratch.
                The list is made twice: from the chunk plan restated in tests/mat_block_cases.py, instantiated explicitly, and by compiling a
                call of the launcher itself; the two sets of kernels must be the same, so a case forgotten on either side fails
  chunk plan    the library's plan (IGXMatMultBlockPlan, pure host code) equals the restatement for every bs 1 .. 8 and nx 1 .. 48, covers
                every column exactly once, and takes widths 2 .. NC and 1 alone
  membrane      tests/eigen_ref.py's loop on the oracle's Poisson and Mass of the 2-D membrane (p = 3, 6^2, all faces Dirichlet) and of the
                1-D rod (p = 2, 12 elements) meets Parlett's bounds against scipy.linalg.eigh, and nev cuts in a spectral gap
Every test prints what it sees before it asserts (run with -s)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eigen_ref as E
import mat_block_cases as MB

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "petiga_amd.h")
CSRC = os.path.join(ROOT, "petiga_amd", "csrc")
ARG_WRONG, OUTOFRANGE = 62, 63
U = 2.0 ** -53


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}
    L, V, dp = P.lib(), C.c_void_p, C.POINTER(C.c_double)
    for name, nargs in {"IGXMatMultBlock": 4, "IGXMatEigenSolve": 9, "IGXMatMultBlockPlan": 4}.items():
        assert name in decl, "%s is not declared in include/petiga_amd.h" % name
        assert len([a for a in decl[name].split(",") if a.strip()]) == nargs, (name, decl[name])
        f = getattr(L, name)                            # AttributeError: the library does not export it
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    assert L.IGXMatMultBlock.argtypes == [V, C.c_int, C.POINTER(V), C.POINTER(V)]
    assert L.IGXMatEigenSolve.argtypes == [V, V, C.POINTER(P.IGXEigenSpec), C.c_int, C.POINTER(V), dp, dp, C.POINTER(P.IGXEigenInfo), dp]
    assert L.IGXMatEigenSolve.argtypes[2:] == L.IGXEigenSolve.argtypes[2:]      # the contract of IGXEigenSolve, on matrices
    assert all(callable(getattr(P.Mat, a)) for a in ("mult_block", "eigen")) and callable(P.mat_mult_block_plan)


def test_a_null_argument_is_refused_first():
    import petiga_amd as P
    L = P.lib()
    why = lambda: L.IGXGetLastError().decode()
    arr = (C.c_void_p * 1)(None)
    bad = P.IGXEigenSpec(0, 99, 9, -1.0, -1.0, -5)      # every member out of range: the null matrix still answers
    info, lam = P.IGXEigenInfo(), (C.c_double * 1)()
    for name, call in (("IGXMatMultBlock", lambda: L.IGXMatMultBlock(None, -3, None, None)),
                       ("IGXMatMultBlock", lambda: L.IGXMatMultBlock(None, 1, arr, arr)),
                       ("IGXMatMultBlock", lambda: L.IGXMatMultBlock(None, 999, arr, arr)),
                       ("IGXMatEigenSolve", lambda: L.IGXMatEigenSolve(None, None, C.byref(bad), 7, arr, lam, None, C.byref(info), None)),
                       ("IGXMatEigenSolve", lambda: L.IGXMatEigenSolve(None, None, None, 0, None, None, None, None, None))):
        assert call() == ARG_WRONG and name in why() and "null" in why(), (name, why())
    n = C.c_int(0)
    assert L.IGXMatMultBlockPlan(1, 4, None, None) == ARG_WRONG
    for bs, nx in ((0, 4), (9, 4), (1, 0), (1, MB.ACTION_BLOCK_MAX + 1)):
        assert L.IGXMatMultBlockPlan(bs, nx, C.byref(n), None) == OUTOFRANGE, (bs, nx)


def test_chunk_plan_covers_every_column_once():
    import petiga_amd as P
    seen = set()
    for bs in range(1, 9):
        nc = MB.full_width(bs)
        assert nc == max(k for k in (2, 4, 8) if 2 * bs * k <= 32), (bs, nc)      # the accumulators: 2 bs NC registers, 32 at the most
        for nx in range(1, MB.ACTION_BLOCK_MAX + 1):
            w = P.mat_mult_block_plan(bs, nx)
            assert w == MB.plan(bs, nx), (bs, nx, w)
            cover = np.zeros(nx, dtype=int)
            at = 0
            for k in w:
                cover[at:at + k] += 1
                at += k
            assert at == nx and (cover == 1).all(), (bs, nx, w)
            assert w[:nx // nc] == [nc] * (nx // nc)                      # the full chunks first
            rest = w[nx // nc:]
            assert sum(rest) == nx % nc and all(k in (1, 2, 4) and k < nc for k in rest) and sorted(rest, reverse=True) == rest and len(set(rest)) == len(rest)
            seen |= {(bs, k) for k in w}
    print("widths by block size:", {bs: sorted(k for b, k in seen if b == bs) for bs in range(1, 9)})
    assert {k for _, k in seen} == {1, 2, 4, 8}


def _reachable():
    """(bs, NC) of every mat_mult_block instantiation the plan can ask for: widths above 1"""
    return sorted({(bs, k) for bs in range(1, 9) for nx in range(1, MB.ACTION_BLOCK_MAX + 1) for k in MB.plan(bs, nx) if k > 1})


def test_the_block_kernels_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    reach = _reachable()
    assert reach == [(bs, k) for bs in range(1, 9) for k in (2, 4, 8) if k <= MB.full_width(bs)]
    sig = "(const MatPat, long long, const int64_t *, const int32_t *, const double *, const MatBlockCols<%d>);\n"
    explicit = tmp_path / "explicit.hip"
    explicit.write_text('#include "mat_ops.hpp"\nnamespace igx {\n'
                        + "".join("template __global__ void mat_mult_block<%d, %d, %s, %d>%s" % (bs, g, t, nc, sig % nc)
                                  for bs, nc in reach for g in (8, 16, 32, 64) for t in ("true", "false")) + "}\n")
    # the launcher's own list: device code holds what a host call of the launcher instantiates (mat_ops.hpp alone instantiates none)
    launcher = tmp_path / "launcher.hip"
    launcher.write_text('#include "mat_block_launch.hpp"\nnamespace igx {\nbool reach(int bs, int nc, int lanes, bool tables, const MatPat &P) {\n'
                        "  return mat_mult_block_launch(bs, nc, lanes, tables, P, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);\n}\n}\n")
    jobs = [(src, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", CSRC, "-I", INCLUDE,
                                    "-o", str(src.with_suffix(".s")), str(src)])) for src in (explicit, launcher)]
    for src, job in jobs:
        assert job.wait() == 0, "hipcc failed on %s" % src.name
    found = []
    for src in (explicit, launcher):
        asm = src.with_suffix(".s").read_text()
        kernels = set(re.findall(r"^(_ZN3igx14mat_mult_block\w*):", asm, flags=re.M))
        found.append(kernels)
        for k in kernels:
            body = asm[asm.index(k + ":"):]
            body = body[:body.index(".end_amdhsa_kernel")]
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), "%s uses scratch" % k
            assert "global_load_dwordx4" in body and "atomic" not in body, k
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            assert vgpr <= 128, "%s takes %d registers: fewer than four waves per SIMD" % (k, vgpr)
    print("%d instantiations from the plan, %d from the launcher" % (len(found[0]), len(found[1])))
    assert len(found[0]) == len(reach) * 4 * 2
    assert found[0] == found[1], sorted(found[0] ^ found[1])


@pytest.mark.parametrize("name", sorted(MB.LOWDIM))
def test_the_host_loop_on_the_membrane_and_the_rod(name):
    A, B, free, nodes = MB.lowdim_oracle(name)
    c = MB.LOWDIM[name]
    nev, m = c["nev"], c["block"]
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max() and free.sum() == np.prod([n - 2 for n in nodes])
    # the fixed rows of the assembled matrices are identity rows and zero columns: what keeps the iterates exactly zero there
    for Mx in (A, B):
        D = Mx.toarray()
        assert not D[np.ix_(~free, free)].any() and not D[np.ix_(free, ~free)].any() and np.count_nonzero(D[np.ix_(~free, ~free)]) == (~free).sum()
    lam_ref, _ = E.dense_reference(A, B, free, m + 1)
    X0 = np.random.default_rng(0).standard_normal((m, A.shape[0])).T.copy()
    d = A.diagonal()
    for pc, T in (("none", None), ("jacobi", lambda r: r / d)):
        out = E.lobpcg(A, B, X0, nev, T=T, rtol=1e-8, maxit=300, fixed=~free)
        bound, rnorm = E.parlett_bounds(A, B, free, out["X"], out["lam"])
        err = np.abs(out["lam"] - lam_ref[:m])
        print("%s, pc=%s: %d iterations, reason %d, restarts %d; lambda %s (eigh %s); |theta - lambda| %s; Parlett bounds %s"
              % (name, pc, out["iterations"], out["reason"], out["restarts"], np.array2string(out["lam"][:nev], precision=8),
                 np.array2string(lam_ref, precision=6), np.array2string(err[:nev], precision=2), np.array2string(bound[:nev], precision=2)))
        assert out["reason"] == E.CONVERGED and out["nconverged"] == nev
        assert lam_ref[nev] - lam_ref[nev - 1] > 1e-3 * lam_ref[nev], "nev does not cut in a spectral gap"
        assert np.all(err[:nev] <= bound[:nev] + 64 * U * np.abs(lam_ref[:nev]))
        assert E.orthonormality_defect(B, out["X"]) <= 1e-10 and not out["X"][~free].any()
