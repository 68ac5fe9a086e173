"""The matrix-free actions and diagonals of the one-workgroup-per-element layouts (vec_sumfact at nen, nqp up to 6 and up to 8 per axis)
against the long double references, ENTRY BY ENTRY and ROW BY ROW, with the project's constants (tensor_ref.C_ID on the identity
geometry, C_MAP on an affine map), as tests/test_gpu_action_entrywise.py and tests/test_gpu_matrix_diagonal_entrywise.py do it below
degree 4:
  * row by row: |Y_i - R_i| <= c u S_i with a standard-normal X and with an X whose magnitudes spread over 10^-6 ... 10^6;
  * the operator recovered from the action one column at a time (coloured probing): |Y_i - a_j R_ij| <= c u |a_j| S_ij on every row
    coupled with a probed column j, every other row exactly 0.0;
  * the diagonal row by row: |D_r - R_rr| <= c u S_rr, a fixed row its element count exactly.
For comparison, the CPU oracle's own worst ratios over degrees 4 to 7 (graded knots, mixed degrees and quadrature sizes, affine and
rational maps) are 10.0 u S for the action and 20.4 u S for the diagonal.

Every test prints its worst ratio (lines starting HD-ROWS, HD-PROBE, HD-DIAG); no MI355X figures are recorded here yet."""
import numpy as np
import pytest

import pointwise_ref as PW
import tensor_ref as T
import test_gpu_action_entrywise as AE
from test_pointwise_reference import wide

pytestmark = pytest.mark.gpu

LD = T.LD
_k = T.graded_knots
G4 = [_k(4, 3, 100.0), _k(4, 2, 0.01), _k(4, 3, 100.0)]
_bcs, BC3, EL_BCS = AE._bcs, AE.BC3, AE.EL_BCS

# name: (setup_case keywords, form, driver, lanes per axis)
ROWWISE = {
    "poisson-p4-graded": (dict(dof=1, p=4, N=0, knots=G4, bcs=_bcs()), "poisson", "matrix", 6),
    "poisson-p5": (dict(dof=1, p=5, N=[2, 2, 3], bcs=_bcs(kind="some")), "poisson", "matrix", 6),
    "poisson-p7": (dict(dof=1, p=7, N=[2, 1, 2], bcs=BC3), "poisson", "matrix", 8),
    "poisson-p546-nqp658": (dict(dof=1, p=[5, 4, 6], N=[2, 2, 2], nqp=[6, 5, 8], bcs={(1, 0, 0): 1.0}), "poisson", "matrix", 8),
    "poisson-p4-affine": (dict(dof=1, p=4, N=[2, 2, 2], geometry="affine", seed=1, bcs=_bcs()), "poisson", "matrix", 6),
    "poisson-p6-rational": (dict(dof=1, p=6, N=[2, 2, 1], geometry="rational", seed=3, bcs=BC3), "poisson", "matrix", 8),
    "elasticity-p4": (dict(dof=3, p=4, N=[2, 2, 2], bcs=EL_BCS), "elasticity", "matrix", 6),
    "bratu-jacobian-p4-graded": (dict(dof=1, p=4, N=0, knots=G4, bcs=_bcs()), "bratu", "jacobian", 6),
    "bratu-jacobian-p7": (dict(dof=1, p=7, N=[2, 1, 2], bcs=BC3), "bratu", "jacobian", 8),
    "ch-p4": (dict(dof=1, p=4, N=[2, 2, 2]), "cahnhilliard", "ijacobian", 6),
}
PROBE = {
    "poisson-p4-graded": ROWWISE["poisson-p4-graded"],
    "poisson-p6": (dict(dof=1, p=6, N=[2, 1, 1], bcs=BC3), "poisson", "matrix", 8),
}
DIAGONAL = [n for n in ROWWISE if not n.startswith("ch-")]


def _layout(kn, lanes):
    assert "one workgroup per element" in kn and "%d x %d x %d lanes" % (lanes, lanes, lanes) in kn, kn


@pytest.mark.parametrize("name", list(ROWWISE))
def test_action_row_by_row(name):
    kw, form, driver, lanes = ROWWISE[name]
    act = AE._Action(kw, form, driver)
    ref, _, action = AE._references(act, kw)
    worst = {}
    for tag, X in (("X", np.random.default_rng(31).standard_normal(act.n)), ("Xwide", wide(act.n))):
        Y = act(X)
        kn = act.check_kernel()
        _layout(kn, lanes)
        worst[tag] = PW.compare_rows(Y, *action(X), act.c, ref, "%s %s" % (name, tag))
    print("HD-ROWS %-28s %-40s worst %s u S (c = %g)" % (name, kn[-40:], "  ".join("%s %.2f" % kv for kv in worst.items()), act.c))


@pytest.mark.parametrize("name", list(PROBE))
def test_operator_recovered_from_the_action(name):
    kw, form, driver, lanes = PROBE[name]
    act = AE._Action(kw, form, driver)
    ref, entries, _ = AE._references(act, kw)
    n, dof = act.n, kw["dof"]
    rows = np.arange(n)
    cols, valid = ref.stencil(rows)
    rr, cc = np.nonzero(valid)
    er, ec = rows[rr], cols[rr, cc]
    R, S = entries(er, ec)
    fx = ref.fixed(er)[0]
    diag = fx & (er == ec)
    S[diag] = R[diag]                                    # a fixed row: m a_i, added once per element -- rounded, bound m |a_i|
    colour, ncol, per_axis = PW.colouring(ref.tabs, dof)
    rng = np.random.default_rng(17)
    amp = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    order = np.argsort(colour[ec], kind="stable")
    start = np.searchsorted(colour[ec][order], np.arange(ncol + 1))
    worst, probed = 0.0, 0
    for k in range(ncol):
        Y = act(np.where(colour == k, amp, 0.0))
        if k == 0:
            kn = act.check_kernel()
            _layout(kn, lanes)
        e = order[start[k]:start[k + 1]]
        assert np.unique(er[e]).size == e.size         # no row couples with two columns of this colour
        a = amp[ec[e]]
        worst = max(worst, T.compare_entrywise((er[e], ec[e], Y[er[e]]), LD(1) * a * R[e], np.abs(a) * S[e], act.c, ref,
                                               "%s colour %d" % (name, k), pattern=False))
        rest = np.ones(n, dtype=bool)
        rest[er[e]] = False
        bad = np.flatnonzero(rest & ~(Y == 0.0))
        assert bad.size == 0, "%s colour %d: row %d couples with no probed column and is %r" % (name, k, bad[0], Y[bad[0]])
        probed += e.size
    assert probed == er.size and ncol == int(np.prod(per_axis)) * dof
    print("HD-PROBE %-28s %-40s %d colours %s, %d entries, worst %.2f u S (c = %g)" % (name, kn[-40:], ncol, per_axis, probed, worst, act.c))


@pytest.mark.parametrize("name", DIAGONAL)
def test_diagonal_row_by_row(name):
    kw, form, driver, lanes = ROWWISE[name]
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
    _layout(kn, lanes)
    rows = np.arange(act.n)
    R, S = entries(rows, rows)
    fx = ref.fixed(rows)[0]
    assert fx.any() and np.all(S[fx] == 0) and np.all(S[~fx] > 0)
    worst = T.compare_entrywise((rows, rows, D.get()), R, S, act.c, ref, name, pattern=False)
    print("HD-DIAG %-28s %-40s %d rows (%d fixed), worst %.2f u S (c = %g)" % (name, kn[-40:], rows.size, fx.sum(), worst, act.c))
