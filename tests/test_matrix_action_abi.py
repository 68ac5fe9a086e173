"""The matrix-free actions in the C ABI (include/petiga_amd.h) and its Python view: the three drivers are declared, exported and
bound with the header's argument counts, and the ACTION instantiation of vec_sumfact compiles for a run-time struct (hiprtc for
gfx950: no GPU needed)."""
import ctypes as C
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
ACTIONS = {"IGXComputeMatrixAction": 3, "IGXComputeJacobianAction": 4, "IGXComputeIJacobianAction": 7}

USER_DIFFUSION = r"""
struct UserDiffusion {
  static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = NEED_X;
  static constexpr unsigned MAT_TEST_MASK = 0xEu, VEC_TEST_MASK = 0x1u;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    const double d00 = 1.0 + p.x[0], d11 = 2.0, d22 = 1.0 + p.x[1] * p.x[2], d01 = 0.3 * p.x[0];
    T[0] = d00 * Na[1] * Nb[1] + d11 * Na[2] * Nb[2] + d22 * Na[3] * Nb[3] + d01 * (Na[1] * Nb[2] + Na[2] * Nb[1]);
  }
  static __device__ void vec(const PtView &p, const double *Na, double *R) { R[0] = Na[0] * p.prm[0]; }
};
// a second-order struct with two fields: the direction's Hessians and the column sum over the trial fields
struct UserBiharmonic2 {
  static constexpr int DOF = 2, ORDER = 2; static constexpr unsigned NEED = NEED_U;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    const double la = Na[4] + Na[8] + Na[12], lb = Nb[4] + Nb[8] + Nb[12];
    T[0] = la * lb + p.shift * Na[0] * Nb[0]; T[1] = Na[0] * Nb[1] * p.u[0]; T[2] = Na[2] * Nb[0]; T[3] = Na[0] * Nb[0] + la * lb;
  }
  static __device__ void vec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; R[1] = 0.0; }
};
"""


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}


@pytest.mark.parametrize("name", sorted(ACTIONS))
def test_declared_exported_and_bound(name):
    import petiga_amd as P
    decl = _declarations()
    assert name in decl, "not declared in include/petiga_amd.h"
    nargs = len([a for a in decl[name].split(",") if a.strip()])
    assert nargs == ACTIONS[name]
    f = getattr(P.lib(), name)                      # AttributeError: the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == nargs
    # the doubles of IGXComputeIJacobianAction sit where the header puts them
    doubles = [i for i, a in enumerate(decl[name].split(",")) if a.strip().startswith("double")]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == doubles


def test_python_view_has_the_three_calls():
    import petiga_amd as P
    for m in ("compute_matrix_action", "compute_jacobian_action", "compute_ijacobian_action"):
        assert callable(getattr(P.IGX, m))


@pytest.mark.parametrize("struct,dof,p", [("UserDiffusion", 1, 2), ("UserDiffusion", 1, 3), ("UserBiharmonic2", 2, 2)])
def test_action_instantiation_of_a_run_time_struct_compiles(struct, dof, p):
    """IGXCheckFormSource(gram = 7): vec_sumfact<Struct, GEO, NS, ACTION = true>, two elements per wavefront at p = 2"""
    import petiga_amd as P
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, 4)
    g.set_form_source(USER_DIFFUSION, struct, (0.7,))
    g.check_form_source(True, 7)
    g2 = P.IGX(2, 1)
    for i in range(2):
        g2.axis_uniform(i, p, 4)
    if dof == 1:
        g2.set_form_source("struct D2 { static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = 0;"
                           " static __device__ void mat(const PtView &, const double *Na, const double *Nb, double *T) { T[0] = Na[1] * Nb[1]; }"
                           " static __device__ void vec(const PtView &, const double *, double *R) { R[0] = 0; } };", "D2")
        with pytest.raises(P.IGXError) as e:
            g2.check_form_source(True, 7)
        assert e.value.code == 56 and "dim 3" in str(e.value)
