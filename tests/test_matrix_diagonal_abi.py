"""The matrix-free diagonals in the C ABI (include/petiga_amd.h) and its Python view: the three drivers are declared, exported and
bound with the header's argument counts, and the DIAGONAL instantiation of vec_sumfact compiles for a run-time struct (hiprtc for
gfx950: no GPU needed) on the identity and on a NURBS geometry, and is refused for a struct with second-order shape features."""
import ctypes as C
import os
import re

import pytest

from common import make_pair, warped_geometry
from test_gpu_matrix_action import USER_DIFFUSION

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
DIAGONALS = {"IGXComputeMatrixDiagonal": 2, "IGXComputeJacobianDiagonal": 3, "IGXComputeIJacobianDiagonal": 6}

USER_BIHARMONIC = r"""
struct UserBiharmonic {
  static constexpr int DOF = 1, ORDER = 2; static constexpr unsigned NEED = 0;
  static __device__ void mat(const PtView &, const double *Na, const double *Nb, double *T) { T[0] = (Na[4] + Na[8] + Na[12]) * (Nb[4] + Nb[8] + Nb[12]); }
  static __device__ void vec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; }
};
"""


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}


@pytest.mark.parametrize("name", sorted(DIAGONALS))
def test_declared_exported_and_bound(name):
    import petiga_amd as P
    decl = _declarations()
    assert name in decl, "not declared in include/petiga_amd.h"
    nargs = len([a for a in decl[name].split(",") if a.strip()])
    assert nargs == DIAGONALS[name]
    f = getattr(P.lib(), name)                      # AttributeError: the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == nargs
    # the doubles of IGXComputeIJacobianDiagonal sit where the header puts them
    doubles = [i for i, a in enumerate(decl[name].split(",")) if a.strip().startswith("double")]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == doubles


def test_python_view_has_the_three_calls():
    import petiga_amd as P
    for m in ("compute_matrix_diagonal", "compute_jacobian_diagonal", "compute_ijacobian_diagonal"):
        assert callable(getattr(P.IGX, m))


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("geo", [None, "nurbs"])
def test_diagonal_instantiation_of_a_run_time_struct_compiles(geo, p):
    """IGXCheckFormSource(gram = 8): vec_sumfact<UserDiffusion, GEO, NS, false, DIAGONAL = true>, two elements per wavefront at p = 2"""
    orc, g = make_pair(3, 1, p, [4, 4, 3])
    if geo:
        X, W = warped_geometry(orc, 3, seed=2, rational=True, amp=0.05)
        g.set_geometry(X, W)
    g.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
    g.check_form_source(True, 8)


def test_diagonal_instantiation_is_refused_for_a_second_order_struct():
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.set_form_source(USER_BIHARMONIC, "UserBiharmonic", ())
    g.check_form_source(True, 7)                    # (the action takes it)
    with pytest.raises(P.IGXError) as e:
        g.check_form_source(True, 8)
    assert "second-order" in str(e.value), str(e.value)
    g2 = P.IGX(2, 1)
    for i in range(2):
        g2.axis_uniform(i, 2, 4)
    g2.set_form_source("struct D2 { static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = 0;"
                       " static __device__ void mat(const PtView &, const double *Na, const double *Nb, double *T) { T[0] = Na[1] * Nb[1]; }"
                       " static __device__ void vec(const PtView &, const double *, double *R) { R[0] = 0; } };", "D2")
    with pytest.raises(P.IGXError) as e:
        g2.check_form_source(True, 8)
    assert e.value.code == 56 and "dim 3" in str(e.value)
