"""The matrix-free point-block diagonals above four basis functions or points per axis (petiga_amd/csrc/vec_sumfact.hpp, DIAGONAL + BLOCK:
one workgroup per element, 6 x 6 x 6 lanes for elasticity-p4 and nsvms-p4 of tests/test_gpu_matrix_free_high_degree.py, 8 x 8 x 8 lanes
for elasticity p = 6 on (2, 1, 1) elements with a Dirichlet face) against the blocks of the CPU oracle's matrix, with the bound of
tests/test_gpu_matrix_block_diagonal.py: |B - R| <= tol s_ij where i and j are free, exact values elsewhere."""
import functools

import numpy as np
import pytest

import oracle_api as O
import test_gpu_matrix_free_high_degree as HD
from common import make_pair
from test_gpu_matrix_block_diagonal import blocks_of, check_blocks, fixed_rows, host_blocks

pytestmark = pytest.mark.gpu

# name -> (form, dof, p, N, Dirichlet values, tolerance, lanes per axis)
CASES = {n: (HD.CASES[n][0], HD.CASES[n][1], HD.CASES[n][2], HD.CASES[n][3], HD.CASES[n][6], HD.CASES[n][7], HD.CASES[n][8]) for n in ("elasticity-p4", "nsvms-p4")}
CASES["elasticity-p6"] = ("elasticity", 3, 6, (2, 1, 1), [(0, 0, f, 0.0) for f in range(3)], 1e-12, 8)


def _pair(name):
    form, dof, p, N, bcs = CASES[name][:5]
    orc, eng = make_pair(3, dof, p, list(N))
    for g in (orc, eng):
        for bc in bcs:
            g.set_boundary_value(*bc)
    return orc, eng


@functools.lru_cache(maxsize=None)
def _ref(name):
    form, dof = CASES[name][:2]
    orc, _ = _pair(name)
    U = V = None
    if form == "elasticity":
        M = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*HD.EL))[0].scipy()
    else:
        _, U, V = HD._reference(name)[:3]
        M = orc.compute_ijacobian("orc_form_ns_tangent", O.NSVMSCtx(*HD.NS), HD.I_SHIFT[form], V, 0.0, U).scipy()
    return U, V, blocks_of(M, dof), fixed_rows(M).reshape(-1, dof)


@pytest.mark.parametrize("name", sorted(CASES))
def test_blocks_equal_the_oracle_matrix_blocks(name):
    form, dof, p, N, bcs, tol, lanes = CASES[name]
    U, V, R, fx = _ref(name)
    _, eng = _pair(name)
    eng.set_form(form, HD.PARAMS[form])
    B = [eng.create_vec().set(np.full(R.shape[0] * dof, np.nan)) for _ in range(dof)]      # (the driver zeroes the columns)
    if form == "elasticity":
        eng.compute_matrix_block_diagonal(B)
    else:
        eng.compute_ijacobian_block_diagonal(HD.I_SHIFT[form], eng.create_vec().set(V), 0.0, eng.create_vec().set(U), B)
    eng.synchronize()
    HD._kernel(eng, "matrix block diagonal", lanes)
    assert fx.any() and (fx.any(axis=1) & ~fx.all(axis=1)).any() == (name != "elasticity-p6")
    check_blocks(host_blocks(B, dof), R, fx, tol, name)
