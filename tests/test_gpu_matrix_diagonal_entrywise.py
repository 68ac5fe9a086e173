"""The matrix-free diagonals (IGXComputeMatrixDiagonal / JacobianDiagonal / IJacobianDiagonal: vec_sumfact<..., DIAGONAL = true>)
against the long double references, ROW BY ROW: |D_r - R_rr| <= c u S_rr with the project's constants (C_ID on the identity
geometry, C_MAP on an affine map; calibrated on the CPU oracle by test_tensor_reference.py and test_pointwise_reference.py).

test_gpu_matrix_diagonal.py scales by the largest free diagonal of the field: on a graded mesh the corner rows are orders of
magnitude smaller than the largest and a wrong one passes it.  Here every row is held to its own S_rr, the sum of the absolute
values of the terms of R_rr (TensorRef.entries for Poisson and elasticity, PointwiseRef.bratu_entries at a varying state for
Bratu); a fixed row (S = 0) must hold its element count exactly.  The cases are those of tests/test_gpu_action_entrywise.py's PROBE.

Worst ratios on an MI355X (u S): 16.6 on the identity geometry (Bratu Jacobian, p = 3 graded; Poisson p = 3 graded 13.3, p = 2 graded 5.0,
elasticity 5.5, Bratu IJacobian p = 2 4.8) and 20.2 on a map (Poisson p = 3, constant NURBS weights; affine 8.4)."""
import numpy as np
import pytest

import tensor_ref as T
import test_gpu_action_entrywise as AE

pytestmark = pytest.mark.gpu

NAMES = ["poisson-p3-graded", "poisson-p2-graded-odd", "poisson-p3-affine", "poisson-p3-rational", "elasticity-p2",
         "bratu-jacobian-p3-graded", "bratu-ijacobian-p2-odd"]


@pytest.mark.parametrize("name", NAMES)
def test_diagonal_row_by_row(name):
    kw, form, driver = AE.PROBE[name]
    act = AE._Action(kw, form, driver)      # (the engine with its form set, the state on the device and the case's constant c)
    ref, entries, _ = AE._references(act, kw)
    eng, D = act.eng, act.Y                 # (NaN-poisoned: the driver zeroes it)
    if driver == "matrix":
        eng.compute_matrix_diagonal(D)
    elif driver == "jacobian":
        eng.compute_jacobian_diagonal(act.Uv, D)
    else:
        eng.compute_ijacobian_diagonal(act.shift, act.Vv, 0.0, act.Uv, D)
    eng.synchronize()
    kn = eng.kernel_name()
    assert "vec_sumfact" in kn and "matrix diagonal" in kn, kn
    degrees = act.p if isinstance(act.p, list) else [act.p] * 3
    assert ("two elements per wavefront" in kn) == all(d <= 2 for d in degrees), kn
    rows = np.arange(act.n)
    R, S = entries(rows, rows)
    fx = ref.fixed(rows)[0] if kw.get("bcs") else np.zeros(rows.size, dtype=bool)
    assert fx.any() and np.all(S[fx] == 0) and np.all(S[~fx] > 0)
    worst = T.compare_entrywise((rows, rows, D.get()), R, S, act.c, ref, name, pattern=False)
    print("%-28s %-70s %d rows (%d fixed), worst %.2f u S (c = %g)" % (name, kn[:70], rows.size, fx.sum(), worst, act.c))
