"""The matrix-free actions on a block of vectors in the C ABI (include/petiga_amd.h: IGXComputeMatrixActionBlock / JacobianActionBlock /
IJacobianActionBlock, IGXSetBatchedActions) and their Python view, on a machine without a GPU: the four calls are declared, exported and
bound with the header's arguments; every refusal that needs no vector, hence no device, comes with its code in the order the header pins
(a case below breaks two rules at once where it can, and the earlier one must answer); and the batched kernel (vec_sumfact with BATCH,
petiga_amd/csrc/vec_sumfact.hpp) compiles for gfx950 for every built-in form with an action, on both geometry kinds and in the four
layouts -- 3, 4, 6 and 8 lanes per axis (hipcc, device code only: no GPU needed).

The compile is in two parts, to stay quick.  Every one of the 13 forms x 2 x 4 instantiations goes through the front end and the code
generator at -O1 (templates, static_asserts, the kernel argument of its own, the symbols); the instantiations of Poisson -- the four
layouts, both geometry kinds -- are compiled as the library compiles them, at -O3, and their assembly is looked at: no scratch, the
column loop is a loop (one body for every column), and the layouts' LDS.

Not reached here: what needs a vector -- an entry of another IGX, an aliased result, no form, the action's own IGX_ERR_SUP
(tests/test_gpu_action_block.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "petiga_amd.h")
CSRC = os.path.join(ROOT, "petiga_amd", "csrc")
ARG_WRONG, OUTOFRANGE = 62, 63
V, PV = C.c_void_p, C.POINTER(C.c_void_p)
CALLS = {"IGXComputeMatrixActionBlock": [V, C.c_int, PV, PV],
         "IGXComputeJacobianActionBlock": [V, V, C.c_int, PV, PV],
         "IGXComputeIJacobianActionBlock": [V, C.c_double, V, C.c_double, V, C.c_int, PV, PV],
         "IGXSetBatchedActions": [V, C.c_int]}
# every built-in form the action covers in 3-D (dispatch_unit.hip: dispatch_dim; order <= 2, no boundary branch, no functional)
FORMS = ["FormPoisson<3>", "FormPoissonF<3>", "FormL2ProjX2<3>", "FormErrNorm<3>", "FormMass<3, 1>", "FormMass<3, 2>", "FormMass<3, 3>", "FormMass<3, 4>",
         "FormElasticity", "FormElasticityF", "FormCahnHilliard<3>", "FormBratu<3>", "FormNSVMS"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = _header()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}
    L = P.lib()
    for name, args in CALLS.items():
        assert name in decl, "%s is not declared in include/petiga_amd.h" % name
        assert len([a for a in decl[name].split(",") if a.strip()]) == len(args), (name, decl[name])
        f = getattr(L, name)                            # AttributeError: the library does not export it
        assert f.restype is C.c_int and f.argtypes == args, name
    assert re.search(r"#define\s+IGX_ACTION_MAXCOLS\s+16\b", text)
    for view in ("compute_matrix_action_block", "compute_jacobian_action_block", "compute_ijacobian_action_block", "set_batched_actions"):
        assert callable(getattr(P.IGX, view)), view


def _space(form="poisson"):
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.setup()
    if form:
        g.set_form(form)
    return g


def test_refusals_in_the_pinned_order():
    import petiga_amd as P
    L = P.lib()
    why = lambda: L.IGXGetLastError().decode()
    g = _space()
    nulls = (V * 64)()
    state = V(0x40)                                      # never dereferenced: every case here answers before the state is looked at
    # 1. a null IGX, a null X or Y array, a null state vector -- before nx (out of range in every case)
    assert L.IGXComputeMatrixActionBlock(None, 0, nulls, nulls) == ARG_WRONG
    assert L.IGXComputeMatrixActionBlock(g.h, 0, None, nulls) == ARG_WRONG and "null array" in why()
    assert L.IGXComputeMatrixActionBlock(g.h, 49, nulls, None) == ARG_WRONG and "null array" in why()
    assert L.IGXComputeJacobianActionBlock(None, state, 0, nulls, nulls) == ARG_WRONG
    assert L.IGXComputeJacobianActionBlock(g.h, None, 0, nulls, nulls) == ARG_WRONG and "state" in why()
    assert L.IGXComputeJacobianActionBlock(g.h, state, 0, None, nulls) == ARG_WRONG and "null array" in why()
    assert L.IGXComputeIJacobianActionBlock(g.h, 1.0, None, 0.0, state, 49, nulls, nulls) == ARG_WRONG and "state" in why()
    assert L.IGXComputeIJacobianActionBlock(g.h, 1.0, state, 0.0, None, 49, nulls, nulls) == ARG_WRONG and "state" in why()
    assert L.IGXComputeIJacobianActionBlock(g.h, 1.0, state, 0.0, state, 49, nulls, None) == ARG_WRONG and "null array" in why()
    # 2. nx outside [1, 48] -- before the entries (all null)
    for nx in (0, -1, 49, 1 << 20):
        assert L.IGXComputeMatrixActionBlock(g.h, nx, nulls, nulls) == OUTOFRANGE and "1 to 48" in why() and "block" in why(), nx
        assert L.IGXComputeJacobianActionBlock(g.h, state, nx, nulls, nulls) == OUTOFRANGE, nx
        assert L.IGXComputeIJacobianActionBlock(g.h, 1.0, state, 0.0, state, nx, nulls, nulls) == OUTOFRANGE, nx
    # 3. a null entry -- before the form (none set) and before anything reaches the device
    bare = _space(form=None)
    for nx in (1, 16, 17, 48):
        assert L.IGXComputeMatrixActionBlock(bare.h, nx, nulls, nulls) == ARG_WRONG and "null direction or result" in why(), nx
    assert L.IGXComputeJacobianActionBlock(bare.h, state, 2, nulls, nulls) == ARG_WRONG and "null direction or result" in why()
    # the switch of the eigen solve
    assert L.IGXSetBatchedActions(None, 1) == ARG_WRONG
    assert L.IGXSetBatchedActions(g.h, 1) == 0 and L.IGXSetBatchedActions(g.h, 0) == 0
    g.set_batched_actions(True)
    # the Python view: lists of one length
    with pytest.raises(ValueError):
        g.compute_matrix_action_block([], [None])
    with pytest.raises(P.IGXError) as e:
        g.compute_matrix_action_block([], [])
    assert e.value.code == OUTOFRANGE


def _unit(tmp_path, forms, geos=("false", "true"), lanes=(3, 4, 6, 8)):
    src = tmp_path / "action_block_unit.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <string>\n#include "igx.hpp"\n#include "vec_sumfact.hpp"\nnamespace igx {\n'
                   + "".join("template __global__ void vec_sumfact<%s, %s, %d, true, false, false, true, ActionCols>(SpaceDev, ParamsDev, OutDev, ColorRange, long long, ActionCols);\n" % (f, geo, ns)
                             for f in forms for geo in geos for ns in lanes) + "}\n")
    return src


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    return hipcc


def _kernels(asm):
    """name -> text of every kernel of an assembly file"""
    out = {}
    for m in re.finditer(r"^(_ZN3igx11vec_sumfactI\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def test_every_instantiation_compiles_for_gfx950(tmp_path):
    out = tmp_path / "all.s"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "--cuda-device-only", "-S", "-I", CSRC, "-I", INCLUDE, "-o", str(out), str(_unit(tmp_path, FORMS))])
    assert len(_kernels(out.read_text())) == len(FORMS) * 2 * 4


def test_poisson_instantiations_as_the_library_compiles_them(tmp_path):
    out = tmp_path / "poisson.s"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-I", CSRC, "-I", INCLUDE, "-o", str(out),
                           str(_unit(tmp_path, ["FormPoisson<3>"]))])
    kernels = _kernels(out.read_text())
    assert len(kernels) == 8
    for name, body in kernels.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name       # no scratch: the table of columns stays in the kernel arguments
        ns = int(re.search(r"Lb[01]ELi(\d)E", name).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert lds <= (32 << 10 if ns <= 4 else 64 << 10), (name, lds)
        # one loop body for every column: the loop over the columns is not unrolled, so the kernel holds a backward branch behind its way back
        assert re.search(r"s_cbranch_\w+ \.LBB\d+_\d+", body), name
