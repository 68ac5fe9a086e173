"""The matrix-free point-block diagonal (IGXComputeMatrixBlockDiagonal: vec_sumfact<..., DIAGONAL = true, BLOCK = true>) against the
long double tensor-product reference, ENTRY BY ENTRY: all dof^2 entries of every node of elasticity-p2 of
tests/test_gpu_action_entrywise.py's PROBE, |B - R| <= c u S with the case's own constant, S the sum of the absolute values of the
terms of R; an entry with S = 0 (beside a fixed dof, or the element count on it) is exact."""
import numpy as np
import pytest

import tensor_ref as T
import test_gpu_action_entrywise as AE
from test_gpu_matrix_block_diagonal import host_blocks

pytestmark = pytest.mark.gpu


def test_blocks_entry_by_entry():
    name = "elasticity-p2"
    kw, form, driver = AE.PROBE[name]
    act = AE._Action(kw, form, driver)
    ref, entries, _ = AE._references(act, kw)
    eng, dof = act.eng, kw["dof"]
    B = [eng.create_vec().set(np.full(act.n, np.nan)) for _ in range(dof)]      # (the driver zeroes the columns)
    eng.compute_matrix_block_diagonal(B)
    eng.synchronize()
    kn = eng.kernel_name()
    assert "vec_sumfact" in kn and "matrix block diagonal" in kn and "two elements per wavefront" in kn, kn
    Bh = host_blocks(B, dof)
    node, i, j = np.meshgrid(np.arange(act.n // dof), np.arange(dof), np.arange(dof), indexing="ij")
    rows, cols = (node * dof + i).ravel(), (node * dof + j).ravel()
    R, S = entries(rows, cols)
    fx = ref.fixed(rows)[0] | ref.fixed(cols)[0]
    assert fx.any() and np.all(S[fx] == 0) and np.all(S[~fx & (rows == cols)] > 0)
    worst = T.compare_entrywise((rows, cols, Bh.ravel()), R, S, act.c, ref, name, pattern=False)
    print("%-16s %-70s %d entries (%d beside a fixed dof), worst %.2f u S (c = %g)" % (name, kn[:70], rows.size, fx.sum(), worst, act.c))
