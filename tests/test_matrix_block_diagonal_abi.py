"""The matrix-free point-block diagonals in the C ABI (include/petiga_amd.h) and its Python view: the three drivers, Invert and Apply
are declared, exported and bound with the header's argument counts, and the DIAGONAL + BLOCK instantiation of vec_sumfact compiles
for a two-field, non-symmetric run-time struct (hiprtc for gfx950: no GPU needed) at p = 2, 3 and 4 (3, 4 and 6 lanes per axis) on
the identity and on a rational map, and is refused by name for a struct with second-order shape features and in 2-D."""
import ctypes as C
import os
import re

import pytest

from common import make_pair, warped_geometry
from test_matrix_diagonal_abi import USER_BIHARMONIC

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
CALLS = {"IGXComputeMatrixBlockDiagonal": 3, "IGXComputeJacobianBlockDiagonal": 4, "IGXComputeIJacobianBlockDiagonal": 7,
         "IGXBlockDiagonalInvert": 4, "IGXBlockDiagonalApply": 5}

# two fields, non-symmetric: T[0] = kappa grad Na . grad Nb, T[1] = c Na d_y Nb, T[2] = 0, T[3] = Na Nb
USER_PAIR = r"""
struct UserPair {
  static constexpr int DOF = 2, ORDER = 1; static constexpr unsigned NEED = 0;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    T[0] = p.prm[0] * (Na[1] * Nb[1] + Na[2] * Nb[2] + Na[3] * Nb[3]);
    T[1] = p.prm[1] * Na[0] * Nb[2];
    T[2] = 0.0;
    T[3] = Na[0] * Nb[0];
  }
  static __device__ void vec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; R[1] = 0.5 * Na[0]; }
};
"""
PAIR_PARAMS = (0.7, 1.3)


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    import petiga_amd as P
    decl = _declarations()
    assert name in decl, "not declared in include/petiga_amd.h"
    nargs = len([a for a in decl[name].split(",") if a.strip()])
    assert nargs == CALLS[name]
    f = getattr(P.lib(), name)                      # AttributeError: the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == nargs
    # the doubles of IGXComputeIJacobianBlockDiagonal sit where the header puts them
    doubles = [i for i, a in enumerate(decl[name].split(",")) if a.strip().startswith("double")]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == doubles


def test_python_view_has_the_five_calls():
    import petiga_amd as P
    for m in ("compute_matrix_block_diagonal", "compute_jacobian_block_diagonal", "compute_ijacobian_block_diagonal",
              "block_diagonal_invert", "block_diagonal_apply"):
        assert callable(getattr(P.IGX, m))


@pytest.mark.parametrize("p", [2, 3, 4])
@pytest.mark.parametrize("geo", [None, "nurbs"])
def test_block_instantiation_of_a_run_time_struct_compiles(geo, p):
    """IGXCheckFormSource(gram = 9): vec_sumfact<UserPair, GEO, NS, false, DIAGONAL = true, BLOCK = true>, NS = 3, 4, 6"""
    orc, g = make_pair(3, 2, p, [4, 4, 3] if p < 4 else [2, 2, 1])
    if geo:
        X, W = warped_geometry(orc, 3, seed=2, rational=True, amp=0.05)
        g.set_geometry(X, W)
    g.set_form_source(USER_PAIR, "UserPair", PAIR_PARAMS)
    g.check_form_source(True, 9)


def test_block_instantiation_is_refused_by_name():
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.set_form_source(USER_BIHARMONIC, "UserBiharmonic", ())
    with pytest.raises(P.IGXError) as e:
        g.check_form_source(True, 9)
    assert "second-order" in str(e.value), str(e.value)
    g2 = P.IGX(2, 1)
    for i in range(2):
        g2.axis_uniform(i, 2, 4)
    g2.set_form_source("struct D2 { static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = 0;"
                       " static __device__ void mat(const PtView &, const double *Na, const double *Nb, double *T) { T[0] = Na[1] * Nb[1]; }"
                       " static __device__ void vec(const PtView &, const double *, double *R) { R[0] = 0; } };", "D2")
    with pytest.raises(P.IGXError) as e:
        g2.check_form_source(True, 9)
    assert e.value.code == 56 and "dim" in str(e.value) and "block diagonal" in str(e.value), str(e.value)
