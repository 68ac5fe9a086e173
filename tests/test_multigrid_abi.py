"""IGXMultigrid in the C ABI (include/petiga_amd.h) and its Python view, on a machine without a GPU: the seven calls are declared, exported
and bound with the header's argument counts; IGXMultigridSpec has the size a C compiler gives it; every refusal that is decided before any
HIP call comes with its code, a reason that names the multigrid, and in the order the header pins (a case below breaks two rules at once
where it can, and the earlier one must answer), staleness after IGXSetUp and the stream mismatch included; and
petiga_amd/csrc/multigrid.hpp compiles for gfx950 with every instantiation the cycle launches (hipcc, device code only: no GPU needed).

Not reached here: what needs a vector or a device -- the refusals of Apply / Solve past the null vector, a missing state at SetUp with
vectors of another IGX, what the diagonals refuse (tests/test_gpu_multigrid_cycle.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import transfer_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "petiga_amd.h")
CSRC = os.path.join(ROOT, "petiga_amd", "csrc")
CALLS = {"IGXMultigridCreate": 4, "IGXMultigridSetState": 4, "IGXMultigridSetUp": 1, "IGXMultigridGetInfo": 5, "IGXMultigridApply": 3,
         "IGXMultigridSolve": 9, "IGXMultigridDestroy": 1}
EXTRA = {"IGXMultigridMeasureStep": 6}      # beyond the contract's seven: the measurement of scripts/multigrid_rate.py
ARG_WRONG, OUTOFRANGE, ORDER, SUP, WRONGSTATE = 62, 63, 58, 56, 73


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = _header()
    assert re.search(r"typedef\s+struct\s+_p_IGXMultigrid\s*\*\s*IGXMultigrid\s*;", text)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}
    L, V = P.lib(), C.c_void_p
    for name, nargs in {**CALLS, **EXTRA}.items():
        assert name in decl, "%s is not declared in include/petiga_amd.h" % name
        assert len([a for a in decl[name].split(",") if a.strip()]) == nargs, (name, decl[name])
        f = getattr(L, name)                            # AttributeError: the library does not export it
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    assert L.IGXMultigridCreate.argtypes == [C.c_int, C.POINTER(V), C.POINTER(P.IGXMultigridSpec), C.POINTER(V)]
    assert L.IGXMultigridSolve.argtypes == [V, C.c_int, C.c_double, C.c_double, C.c_int, V, V, C.POINTER(P.IGXSolveInfo), C.POINTER(C.c_double)]
    assert callable(P.IGX.multigrid) and all(callable(getattr(P.Multigrid, a)) for a in ("set_state", "setup", "info", "apply", "solve", "close"))


def test_spec_has_the_size_and_members_of_the_header(tmp_path):
    import petiga_amd as P
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "petiga_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(IGXMultigridSpec), offsetof(IGXMultigridSpec, lo), offsetof(IGXMultigridSpec, coarse_maxit)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(P.IGXMultigridSpec), P.IGXMultigridSpec.lo.offset, P.IGXMultigridSpec.coarse_maxit.offset]
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*IGXMultigridSpec\s*;", _header())
    members = [n.strip() for d in m.group(1).split(";") if d.strip() for n in d.split(None, 1)[1].split(",")]
    assert members == [f[0] for f in P.IGXMultigridSpec._fields_]


def _space(N, p=2, dof=1, setup=True, form=True, faces=((0, 0), (0, 1)), periodic=False):
    import petiga_amd as P
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_knots(i, p, TR.uniform_knots(p, N, periodic=periodic and i == 2), periodic=periodic and i == 2)
    if setup:
        g.setup()
    if form:
        g.set_form("poisson" if dof == 1 else "elasticity", () if dof == 1 else (1.0, 0.3))
    for d, s in faces:
        for f in range(dof):
            g.set_boundary_value(d, s, f, 0.0)
    return g


def _spec(**kw):
    import petiga_amd as P
    v = dict(op=0, a=0.0, t=0.0, smoother_pc=1, degree=2, lo=0.1, hi=1.1, power_its=10, coarse_method=0, coarse_pc=1, coarse_rtol=1e-12, coarse_maxit=50)
    v.update(kw)
    return P.IGXMultigridSpec(*[v[f[0]] for f in P.IGXMultigridSpec._fields_])


def _create(levels, spec=None, n=None):
    import petiga_amd as P
    h = C.c_void_p()
    arr = (C.c_void_p * max(len(levels), 1))(*[g.h.value if g is not None else None for g in levels])
    spec = _spec() if spec is None else spec
    rc = P.lib().IGXMultigridCreate(len(levels) if n is None else n, arr, C.byref(spec), C.byref(h))
    return rc, P.lib().IGXGetLastError().decode(), h


def test_refusals_in_the_pinned_order():
    import petiga_amd as P
    L = P.lib()
    why = lambda: L.IGXGetLastError().decode()
    c, f = _space(2), _space(4)
    rc, msg, h = _create([c, f])
    assert rc == 0 and h.value, (rc, msg)
    # 1. null pointers, before the number of levels and the spec
    bad = _spec(degree=0)
    assert L.IGXMultigridCreate(1, None, C.byref(bad), C.byref(h)) == ARG_WRONG and "multigrid" in why() and "null" in why()
    arr = (C.c_void_p * 2)(c.h.value, f.h.value)
    assert L.IGXMultigridCreate(1, arr, None, C.byref(h)) == ARG_WRONG and L.IGXMultigridCreate(1, arr, C.byref(bad), None) == ARG_WRONG
    rc, msg, _ = _create([c, None], bad)
    assert rc == ARG_WRONG and "multigrid" in msg and "level 1" in msg, (rc, msg)
    # 2. the number of levels before the spec
    for n in (1, 0, -3):
        rc, msg, _ = _create([c, f], bad, n=n)
        assert rc == OUTOFRANGE and "two levels" in msg and "multigrid" in msg, (rc, msg)
    # 3. the spec, before the levels are looked at (the coarse level is not set up)
    raw = _space(2, setup=False)
    for kw, word in ((dict(op=3), "operator"), (dict(op=-1), "operator"), (dict(smoother_pc=0), "smoother_pc"), (dict(smoother_pc=3), "smoother_pc"), (dict(degree=0), "degree"),
                     (dict(lo=0.0), "lo"), (dict(lo=1.2), "lo"), (dict(hi=float("inf")), "lo"), (dict(lo=float("nan")), "lo"), (dict(power_its=0), "power_its"),
                     (dict(coarse_method=2), "coarse method"), (dict(coarse_pc=4), "coarse preconditioner"), (dict(coarse_pc=-1), "coarse preconditioner"),
                     (dict(coarse_maxit=-1), "coarse_maxit"), (dict(coarse_rtol=-1e-3), "coarse_rtol"), (dict(coarse_rtol=float("nan")), "coarse_rtol"),
                     (dict(coarse_maxit=0, coarse_pc=0), "IGX_PC_NONE")):
        rc, msg, _ = _create([raw, f], _spec(**kw))
        assert rc == OUTOFRANGE and "multigrid" in msg and word in msg, (kw, rc, msg)
    # 4. a level before IGXSetUp, before the form
    rc, msg, _ = _create([raw, _space(4, form=False)])
    assert rc == ORDER and "IGXSetUp" in msg and "multigrid" in msg and "level 0" in msg, (rc, msg)
    # 5. no form, before the forms are compared
    rc, msg, _ = _create([c, _space(4, form=False), _space(8, dof=3)])
    assert rc == WRONGSTATE and "multigrid" in msg and "level 1" in msg, (rc, msg)
    # 6. different forms, then different Dirichlet faces, before the fix table and the streams
    other = _space(4)
    other.set_form("bratu", (1.0,))
    other.set_stream(0x40)                                  # never used: nothing here reaches the device
    rc, msg, _ = _create([c, other])
    assert rc == ARG_WRONG and "same form" in msg and "multigrid" in msg, (rc, msg)
    faces = _space(4, faces=((0, 0),))
    faces.set_stream(0x40)
    rc, msg, _ = _create([c, faces])
    assert rc == ARG_WRONG and "Dirichlet faces" in msg and "level 1" in msg, (rc, msg)
    # 7. the streams, before the transfer (the spaces are not nested)
    odd = _space(3)
    odd.set_stream(0x40)
    rc, msg, _ = _create([c, odd])
    assert rc == ARG_WRONG and "stream" in msg and "multigrid" in msg, (rc, msg)
    # 8. what the transfer refuses, under its code, with the level pair
    rc, msg, _ = _create([c, f, _space(6)])
    assert rc == OUTOFRANGE and "multigrid" in msg and "levels 1 and 2" in msg and "not nested" in msg, (rc, msg)
    rc, msg, _ = _create([_space(2, p=3), f])
    assert rc == ARG_WRONG and "levels 0 and 1" in msg and "degree" in msg, (rc, msg)
    # 9. fast diagonalisation as the coarse preconditioner: accepted at Create, refused at SetUp until IGXFastDiagSetUp ran
    rc, msg, hf = _create([c, f], _spec(coarse_pc=3, coarse_maxit=0))
    assert rc == 0, (rc, msg)
    assert L.IGXMultigridSetUp(hf) == ORDER and "IGXFastDiagSetUp" in why() and "multigrid" in why()
    assert L.IGXMultigridDestroy(C.byref(hf)) == 0
    # 10. Apply and Solve before SetUp; a null multigrid; Solve's own ranges first
    assert L.IGXMultigridApply(h, None, None) == ORDER and "IGXMultigridSetUp" in why()
    info = P.IGXSolveInfo()
    assert L.IGXMultigridSolve(h, 0, 1e-8, 0.0, 10, None, None, C.byref(info), None) == ORDER and "IGXMultigridSetUp" in why()
    for args in ((2, 1e-8, 0.0, 10), (0, -1.0, 0.0, 10), (0, 1e-8, float("nan"), 10), (0, 1e-8, 0.0, -1)):
        assert L.IGXMultigridSolve(h, *args, None, None, None, None) == OUTOFRANGE and "IGXMultigridSolve" in why(), args
    for rc in (L.IGXMultigridApply(None, None, None), L.IGXMultigridSolve(None, 0, 1e-8, 0.0, 10, None, None, None, None), L.IGXMultigridSetUp(None),
               L.IGXMultigridSetState(None, 0, None, None), L.IGXMultigridGetInfo(None, 0, None, None, None)):
        assert rc == ARG_WRONG and "multigrid" in why()
    assert L.IGXMultigridMeasureStep(h, 1, 10, 3, None, None) == OUTOFRANGE and L.IGXMultigridMeasureStep(h, 2, 10, 3, None, None) == OUTOFRANGE
    two = (C.c_double * 2)()
    assert L.IGXMultigridMeasureStep(h, 1, 10, 2, two, two) == ORDER and "IGXMultigridSetUp" in why()
    # 12. a missing state at SetUp
    jc, jf = _bratu(2), _bratu(4)                           # (named: the levels outlive the multigrid made from them)
    rc, msg, hj = _create([jc, jf], _spec(op=1))
    assert rc == 0, (rc, msg)
    assert L.IGXMultigridSetUp(hj) == ARG_WRONG and "state" in why() and "level 0" in why() and "multigrid" in why()
    assert L.IGXMultigridDestroy(C.byref(hj)) == 0
    del jc, jf
    # GetInfo and SetState: the level's range
    n, lam, k = C.c_int64(), C.c_double(), C.c_int()
    assert L.IGXMultigridGetInfo(h, 1, C.byref(lam), C.byref(n), C.byref(k)) == 0 and (n.value, lam.value, k.value) == (6 ** 3, 0.0, 0)
    for level in (-1, 2):
        assert L.IGXMultigridGetInfo(h, level, None, None, None) == OUTOFRANGE and "multigrid" in why()
        assert L.IGXMultigridSetState(h, level, None, None) == OUTOFRANGE and "multigrid" in why()
    # stale after IGXSetUp on any level: every call, before its other checks
    for which in (c, f):
        rc, msg, h2 = _create([c, f])
        assert rc == 0, (rc, msg)
        which.setup()
        for rc in (L.IGXMultigridApply(h2, None, None), L.IGXMultigridSolve(h2, 7, 1e-8, 0.0, 10, None, None, None, None), L.IGXMultigridSetUp(h2),
                   L.IGXMultigridSetState(h2, 9, None, None), L.IGXMultigridGetInfo(h2, 9, None, None, None)):
            assert rc == ORDER
        assert "stale" in why() and "multigrid" in why() and "IGXSetUp" in why()
        assert L.IGXMultigridDestroy(C.byref(h2)) == 0 and not h2.value
    assert L.IGXMultigridApply(h, None, None) == ORDER and "stale" in why()      # (made before both set-ups)
    assert L.IGXMultigridDestroy(C.byref(h)) == 0 and not h.value and L.IGXMultigridDestroy(C.byref(h)) == 0 and L.IGXMultigridDestroy(None) == 0
    # the Python view
    with pytest.raises(P.IGXError) as e:
        _space(4).multigrid([_space(3)])
    assert e.value.code == OUTOFRANGE and "multigrid" in str(e.value)
    m = _space(4).multigrid([_space(2)], degree=3, coarse=dict(pc="fastdiag", maxit=0))
    assert m.info(0)["n"] == 4 ** 3 and m.spec.degree == 3 and m.spec.coarse_pc == 3 and m.spec.coarse_maxit == 0
    m.close()
    m.close()


def _bratu(N):
    g = _space(N, form=False)
    g.set_form("bratu", (1.0,))
    return g


def test_the_sweeps_compile_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    src = tmp_path / "mg_unit.hip"
    src.write_text('#include "multigrid.hpp"\nnamespace igx {\n'
                   "template __global__ void mg_cheb_first<true, false>(double *, double *, double *, const double *, const double *, double, long long);\n"
                   "template __global__ void mg_cheb_first<false, false>(double *, double *, double *, const double *, const double *, double, long long);\n"
                   "template __global__ void mg_cheb_first<true, true>(double *, double *, double *, const double *, const double *, double, long long);\n"
                   "template __global__ void mg_cheb_first<false, true>(double *, double *, double *, const double *, const double *, double, long long);\n"
                   "template __global__ void mg_cheb_step<false>(double *, double *, double *, const double *, const double *, double, double, long long);\n"
                   "template __global__ void mg_cheb_step<true>(double *, double *, double *, const double *, const double *, double, double, long long);\n"
                   "template __global__ void mg_resid<false>(double *, const double *, const double *, long long);\n"
                   "template __global__ void mg_resid<true>(double *, const double *, const double *, long long);\n}\n")
    out = tmp_path / "mg_unit.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", CSRC, "-I", INCLUDE, "-o", str(out), str(src)])
    asm = out.read_text()
    for kernel in ("mg_cheb_first", "mg_cheb_step", "mg_resid", "mg_zero_fixed"):
        assert kernel in asm, kernel
    # the fused step: 16-byte accesses and no scratch (the bit-for-bit test of tests/test_gpu_multigrid_cycle.py holds its roundings)
    step = asm[asm.index("mg_cheb_stepILb0"):]
    step = step[:step.index(".end_amdhsa_kernel")]
    assert "global_load_dwordx4" in step and "global_store_dwordx4" in step
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", step)
