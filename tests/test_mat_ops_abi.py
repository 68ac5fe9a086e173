"""The stored matrix as an operator in the C ABI (include/petiga_amd.h) and its Python view, on a machine without a GPU: IGXMatMult,
IGXMatGetDiagonal, IGXMatGetBlockDiagonal and IGXMatSolve are declared, exported and bound with the header's arguments; a null argument is
refused first, with IGX_ERR_ARG_WRONG and the call's name, before anything touches a device; petiga_amd/csrc/mat_ops.hpp compiles for gfx950
with 16-byte loads and no scratch (hipcc, device code only); and the table-driven column rule of the product, restated in
tests/mat_ops_ref.py, rebuilds bcolidx and finds the diagonal block on hand-built axes and against a scipy CSR of the same stencils.

Not reached here: what needs a matrix or a vector, i.e. a device (tests/test_gpu_mat_mult.py, tests/test_gpu_mat_solve.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mat_ops_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "petiga_amd.h")
CSRC = os.path.join(ROOT, "petiga_amd", "csrc")
CALLS = {"IGXMatMult": 3, "IGXMatGetDiagonal": 2, "IGXMatGetBlockDiagonal": 3, "IGXMatSolve": 6}
ARG_WRONG = 62


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}
    L, V = P.lib(), C.c_void_p
    for name, nargs in CALLS.items():
        assert name in decl, "%s is not declared in include/petiga_amd.h" % name
        assert len([a for a in decl[name].split(",") if a.strip()]) == nargs, (name, decl[name])
        f = getattr(L, name)                            # AttributeError: the library does not export it
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    assert L.IGXMatMult.argtypes == [V, V, V] and L.IGXMatGetDiagonal.argtypes == [V, V]
    assert L.IGXMatGetBlockDiagonal.argtypes == [V, C.c_int, C.POINTER(V)]
    assert L.IGXMatSolve.argtypes == [V, C.POINTER(P.IGXSolveSpec), V, V, C.POINTER(P.IGXSolveInfo), C.POINTER(C.c_double)]
    assert all(callable(getattr(P.Mat, a)) for a in ("mult", "diagonal", "block_diagonal", "solve"))


def test_a_null_argument_is_refused_first():
    import petiga_amd as P
    L = P.lib()
    why = lambda: L.IGXGetLastError().decode()
    spec = P.IGXSolveSpec(7, 9, 9, 0.0, 0.0, None, None, -1.0, -1.0, -5)      # every member out of range: the null matrix still answers
    info = P.IGXSolveInfo()
    arr = (C.c_void_p * 1)(None)
    for name, call in (("IGXMatMult", lambda: L.IGXMatMult(None, None, None)),
                       ("IGXMatGetDiagonal", lambda: L.IGXMatGetDiagonal(None, None)),
                       ("IGXMatGetBlockDiagonal", lambda: L.IGXMatGetBlockDiagonal(None, -3, None)),
                       ("IGXMatGetBlockDiagonal", lambda: L.IGXMatGetBlockDiagonal(None, 1, arr)),
                       ("IGXMatSolve", lambda: L.IGXMatSolve(None, C.byref(spec), None, None, C.byref(info), None)),
                       ("IGXMatSolve", lambda: L.IGXMatSolve(None, None, None, None, None, None))):
        assert call() == ARG_WRONG and name in why() and "null" in why(), (name, why())


def test_the_kernels_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    sig = "(const MatPat, long long, const int64_t *, const int32_t *, const double *, const double *, double *);\n"
    src = tmp_path / "mat_unit.hip"
    src.write_text('#include "mat_ops.hpp"\nnamespace igx {\n'
                   + "".join("template __global__ void mat_mult<%d, %d, %s>%s" % (bs, g, t, sig)
                             for bs in range(1, 9) for g in (8, 16, 32, 64) for t in ("true", "false"))      # every instantiation mat_mult_launch can reach
                   + "template __global__ void mat_get_diag<false>(const MatPat, long long, int, const int64_t *, const double *, const MatCols);\n"
                   + "template __global__ void mat_get_diag<true>(const MatPat, long long, int, const int64_t *, const double *, const MatCols);\n}\n")
    out = tmp_path / "mat_unit.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", CSRC, "-I", INCLUDE, "-o", str(out), str(src)])
    asm = out.read_text()
    kernels = re.findall(r"^(_ZN3igx\w*(?:mat_mult|mat_get_diag)\w*):", asm, flags=re.M)
    assert len(set(kernels)) == 8 * 4 * 2 + 2, kernels      # block sizes x sub-groups x index variants of mat_mult, and the two copies
    for k in set(kernels):
        body = asm[asm.index(k + ":"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), "%s uses scratch" % k
        if "mat_mult" in k:      # the values in 16-byte loads, no atomics
            assert "global_load_dwordx4" in body and "atomic" not in body, k


# ---- the column rule on hand-built axes
def _clamped(p, nel):
    """maximal continuity, clamped ends: nel + p functions, function i shares an element with i - p .. i + p"""
    n = nel + p
    return [range(max(0, i - p), min(n - 1, i + p) + 1) for i in range(n)]


# p = 2 on the knots [0 0 0 .5 .5 1 1 1]: two elements joined C^0, functions 0 1 2 on the first and 2 3 4 on the second
C0_AXIS = [[0, 1, 2], [0, 1, 2], [0, 1, 2, 3, 4], [2, 3, 4], [2, 3, 4]]


def _wrapped(p, n):
    """a periodic axis of n functions held by one rank: the unwrapped stencil i - p .. i + p folded with mod n (it repeats columns when n < 2p + 1)"""
    return [[(i + d) % n for d in range(-p, p + 1)] for i in range(n)]


def test_axis_tables_by_hand():
    rcnt, rcol = R.axis_tables(_clamped(2, 4), 5)
    assert rcnt.tolist() == [3, 4, 5, 5, 4, 3]
    assert rcol.tolist() == [[0, 1, 2, -1, -1], [0, 1, 2, 3, -1], [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [2, 3, 4, 5, -1], [3, 4, 5, -1, -1]]
    rcnt, rcol = R.axis_tables(C0_AXIS, 5)
    assert rcnt.tolist() == [3, 3, 5, 3, 3] and rcol[3].tolist() == [2, 3, 4, -1, -1]
    rcnt, rcol = R.axis_tables(_wrapped(2, 4), 5)      # 4 < 2p + 1 = 5 functions: every row folds onto all four columns
    assert rcnt.tolist() == [4, 4, 4, 4] and all(r.tolist() == [0, 1, 2, 3, -1] for r in rcol)
    rcnt, rcol = R.axis_tables(_wrapped(2, 6), 5)
    assert rcnt.tolist() == [5] * 6 and rcol[0].tolist() == [0, 1, 2, 4, 5] and rcol[5].tolist() == [0, 1, 3, 4, 5]
    # one axis alone: browptr, bcolidx and the diagonal's place are the axis' own
    one = [R.axis_tables(C0_AXIS, 5), R.unit_axis(), R.unit_axis()]
    cnt, col = [t[0] for t in one], [t[1] for t in one]
    assert R.browptr(cnt).tolist() == [0, 3, 6, 11, 14, 17]
    assert R.bcolidx(cnt, col, [5, 1, 1]).tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 4, 2, 3, 4, 2, 3, 4]
    assert R.diagonal_position(cnt, col).tolist() == [0, 1, 2, 1, 2]
    wr = [R.axis_tables(_wrapped(2, 4), 5), R.unit_axis(), R.unit_axis()]
    assert R.diagonal_position([t[0] for t in wr], [t[1] for t in wr]).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("axes", [("clamped", "c0", "wrapped4"), ("wrapped3", "clamped3", "unit"), ("c0", "unit", "unit"), ("wrapped6", "wrapped4", "clamped")])
def test_column_rule_against_a_scipy_csr_of_the_same_stencils(axes):
    import scipy.sparse as sp
    kinds = {"clamped": (_clamped(2, 4), 5), "clamped3": (_clamped(3, 2), 7), "c0": (C0_AXIS, 5), "wrapped4": (_wrapped(2, 4), 5), "wrapped3": (_wrapped(2, 3), 5),
             "wrapped6": (_wrapped(2, 6), 5), "unit": ([[0]], 1)}
    st = [kinds[a][0] for a in axes]
    tabs = [R.axis_tables(s, kinds[a][1]) for s, a in zip(st, axes)]
    rcnt, rcol = [t[0] for t in tabs], [t[1] for t in tabs]
    n = [len(s) for s in st]

    def pattern(s):
        m = np.zeros((len(s), len(s)))
        for i, cols in enumerate(s):
            m[i, list(cols)] = 1.0
        return sp.csr_matrix(m)
    M = sp.kron(pattern(st[2]), sp.kron(pattern(st[1]), pattern(st[0]))).tocsr()      # row and column r0 + n0 (r1 + n1 r2)
    M.eliminate_zeros()      # (kron goes through dense blocks and stores their zeros)
    M.sort_indices()
    assert np.array_equal(R.browptr(rcnt), M.indptr)
    ci = R.bcolidx(rcnt, rcol, n)
    assert np.array_equal(ci, M.indices)
    rp, pos = R.browptr(rcnt), R.diagonal_position(rcnt, rcol)
    assert (pos >= 0).all() and np.array_equal(ci[rp[:-1] + pos], np.arange(len(pos)))
    # and back: the tables read out of the pattern are the tables it was made from
    cnt2, col2 = R.tables_of_pattern(M.indptr, M.indices, n, n)
    for d in range(3):
        assert np.array_equal(cnt2[d], rcnt[d]) and np.array_equal(col2[d], rcol[d][:, :col2[d].shape[1]])
    # the long double product on this pattern with bs = 2 is the dense product
    rng = np.random.default_rng(5)
    val, x = rng.standard_normal(ci.size * 4), rng.standard_normal(len(pos) * 2)
    y, S, cnt = R.entrywise_product(rp, ci, val, 2, x)
    dense = np.zeros((len(pos) * 2, len(pos) * 2))
    for r in range(len(pos)):
        for k in range(rp[r], rp[r + 1]):
            dense[2 * r:2 * r + 2, 2 * ci[k]:2 * ci[k] + 2] = val[4 * k:4 * k + 4].reshape(2, 2)
    assert np.allclose(np.asarray(y, dtype=float), dense @ x, rtol=0, atol=1e-12) and np.all(S >= np.abs(y))
    assert np.array_equal(cnt, np.repeat(np.diff(rp) * 2, 2))
