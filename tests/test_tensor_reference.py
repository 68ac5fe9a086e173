"""The entry-wise tensor-product reference (tensor_ref.py) against the CPU oracle, its own accuracy, and what it sees that the global
tolerance of compare_mats does not.

The oracle sums the same point terms in its own order, so its entry-wise distance from the exact value, in units of u * S, calibrates
the constant c of the GPU checks: C_ID (identity geometry) and C_MAP (affine maps, whose Jacobian the engine and the oracle compute
from control points) are 4x the worst ratio met here, rounded up to a power of two."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import tensor_ref as T
from common import compare_mats

LAM = 3.5

STATE = 0.3
BC_C = {(d, s, 0): STATE for d in range(3) for s in range(2)}      # a Dirichlet value equal to the constant state keeps the state constant


def _bcs(dim, dof=1, kind="all"):
    out = {}
    for d in range(dim):
        for s in range(2):
            for f in range(dof):
                if kind == "all" or (d + s + f) % 2 == 0:
                    out[(d, s, f)] = 1.0 + 0.5 * d - 0.25 * s + 0.125 * f
    return out


class _El(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("mu", C.c_double)]


def oracle_result(orc, dim, dof, form, driver, c=STATE, v=0.7, shift=4.0):
    """(A or None, b or None) of the oracle, and the reference's form."""
    n = orc.global_size()
    if form in ("poisson", "poisson_f"):
        A, b = orc.compute_system("orc_form_" + form)
        tf = T.poisson(dim) if form == "poisson" else T.poisson_f(dim)
    elif form == "mass":
        A, b = orc.compute_system("orc_form_mass")
        tf = T.mass(dim, dof)
    elif form == "elasticity":
        A, b = orc.compute_system("orc_form_elasticity", _El(1.3, 0.7))
        tf = T.elasticity(1.3, 0.7)
    elif form == "elasticity_f":
        A, b = orc.compute_system("orc_form_elasticity_f", (C.c_double * 5)(1.3, 0.7, 0.5, -1.0, 2.0))
        tf = T.elasticity(1.3, 0.7, [0.5, -1.0, 2.0])
    else:
        lam, U, V = C.c_double(LAM), np.full(n, c), np.full(n, v)
        A = b = None
        if driver == "jacobian":
            A = orc.compute_jacobian("orc_form_bratu_jacobian", lam, U)
            tf = T.bratu(dim, LAM, c)
        elif driver == "ijacobian":
            A = orc.compute_ijacobian("orc_form_bratu_ijacobian", lam, shift, V, 0.0, U)
            tf = T.bratu(dim, LAM, c, shift=shift)
        elif driver == "function":
            b = orc.compute_function("orc_form_bratu_function", lam, U)
            tf = T.bratu(dim, LAM, c)
        else:
            b = orc.compute_ifunction("orc_form_bratu_ifunction", lam, shift, V, 0.0, U)
            tf = T.bratu(dim, LAM, c, v=v)
    return A, b, tf


def _k(p, n, ratio, **kw):
    return T.graded_knots(p, n, ratio, **kw)


# id: (setup_case keywords, form, driver)
CASES = {
    "uniform-p3": (dict(dim=3, dof=1, p=3, N=[8, 8, 8], bcs=_bcs(3)), "poisson", "system"),
    "uniform-p3-matrix": (dict(dim=3, dof=1, p=3, N=[8, 8, 8]), "poisson", "system"),
    "random-p3": (dict(dim=3, dof=1, p=3, N=0, knots=[_k(3, 9, 0, seed=1), _k(3, 8, 0, seed=2), _k(3, 7, 0, seed=3)], bcs=_bcs(3)), "poisson", "system"),
    "graded100-p3": (dict(dim=3, dof=1, p=3, N=0, knots=[_k(3, 9, 100.0), _k(3, 8, 0.01), _k(3, 7, 100.0)], bcs=_bcs(3)), "poisson", "system"),
    "graded1000-p3": (dict(dim=3, dof=1, p=3, N=0, knots=[_k(3, 8, 1000.0), _k(3, 7, 1000.0), _k(3, 6, 0.001)]), "poisson", "system"),
    "graded100-p2": (dict(dim=3, dof=1, p=2, N=0, knots=[_k(2, 10, 100.0), _k(2, 7, 0.01), _k(2, 6, 100.0)], bcs=_bcs(3)), "poisson", "system"),
    "C1-lines-p3": (dict(dim=3, dof=1, p=3, N=[7, 0, 5], knots=[None, _k(3, 6, 1.0, C=1), None], bcs=_bcs(3, kind="some")), "poisson", "system"),
    "C0-lines-p2": (dict(dim=3, dof=1, p=2, N=[6, 5, 4], C=[0, 1, 1], bcs=_bcs(3, kind="some")), "poisson_f", "system"),
    "periodic0-p3": (dict(dim=3, dof=1, p=3, N=[10, 6, 5], periodic=[True, False, False], bcs={(1, 0, 0): 0.5, (2, 1, 0): -1.5}), "poisson", "system"),
    "C1-axis0-p3": (dict(dim=3, dof=1, p=3, N=[7, 6, 5], C=[1, 2, 2], bcs=_bcs(3)), "poisson", "system"),
    "lobatto-p3": (dict(dim=3, dof=1, p=3, N=[7, 4, 4], rule="lobatto"), "poisson", "system"),
    "reduced-p3": (dict(dim=3, dof=1, p=3, N=[7, 4, 5], rule="reduced", bcs=_bcs(3, kind="some")), "poisson", "system"),
    "user-p2": (dict(dim=3, dof=1, p=2, N=[6, 5, 4], rule="user", nqp=4), "poisson", "system"),
    "nqp5-p3": (dict(dim=3, dof=1, p=3, N=[6, 5, 4], nqp=5, bcs=_bcs(3)), "poisson", "system"),
    "p4-2d": (dict(dim=2, dof=1, p=4, N=[7, 6], bcs=_bcs(2)), "poisson", "system"),
    "1d-p3-graded": (dict(dim=1, dof=1, p=3, N=0, knots=[_k(3, 12, 1000.0)], bcs={(0, 0, 0): 0.5, (0, 1, 0): -2.0}), "poisson", "system"),
    "2d-p2-periodic": (dict(dim=2, dof=1, p=2, N=[6, 7], periodic=[False, True], bcs={(0, 1, 0): 2.0}), "poisson_f", "system"),
    "load-p2": (dict(dim=3, dof=1, p=2, N=[6, 5, 4], bcs={(0, 0, 0): 0.5}, loads={(0, 1, 0): 1.5, (2, 0, 0): -0.75}), "poisson", "system"),
    "mass-dof2": (dict(dim=3, dof=2, p=3, N=[6, 5, 4], bcs=_bcs(3, 2, "some")), "mass", "system"),
    "mass-dof4-2d": (dict(dim=2, dof=4, p=2, N=[6, 5], bcs=_bcs(2, 4, "some")), "mass", "system"),
    "mass-dof1-1d": (dict(dim=1, dof=1, p=3, N=[9]), "mass", "system"),
    "elasticity-p3": (dict(dim=3, dof=3, p=3, N=[5, 4, 4], bcs=_bcs(3, 3, "some")), "elasticity", "system"),
    "elasticity_f-p2": (dict(dim=3, dof=3, p=2, N=[5, 4, 6], bcs={(0, 0, 1): 0.5, (0, 0, 0): 0.25}), "elasticity_f", "system"),
    "bratu-jacobian-p3": (dict(dim=3, dof=1, p=3, N=[6, 5, 4], bcs=BC_C), "bratu", "jacobian"),
    "bratu-ijacobian-p2": (dict(dim=3, dof=1, p=2, N=[0, 5, 6], knots=[_k(2, 8, 100.0), None, None]), "bratu", "ijacobian"),
    "bratu-function-p3": (dict(dim=3, dof=1, p=3, N=[0, 5, 4], knots=[_k(3, 7, 100.0), None, None], bcs=BC_C), "bratu", "function"),
    "bratu-ifunction-p2": (dict(dim=3, dof=1, p=2, N=[6, 5, 7]), "bratu", "ifunction"),
    "rank-box-p3": (dict(dim=3, dof=1, p=3, N=[7, 6, 10], box=(2, 1), bcs=_bcs(3)), "poisson", "system"),
    "rank-box-elasticity": (dict(dim=3, dof=3, p=2, N=[5, 4, 8], box=(2, 0), bcs=_bcs(3, 3, "some")), "elasticity", "system"),
    # affine maps
    "affine-p3": (dict(dim=3, dof=1, p=3, N=[7, 6, 5], geometry="affine", bcs=_bcs(3)), "poisson", "system"),
    # (not graded: the Jacobian of the map is summed from control points, whose cancellation grows with 1/h -- an error S does not model)
    "affine-p2-random": (dict(dim=3, dof=1, p=2, N=[0, 5, 0], knots=[_k(2, 8, 0, seed=4), None, _k(2, 6, 0, seed=5)], geometry="affine", seed=3), "poisson_f", "system"),
    "rational-p3": (dict(dim=3, dof=1, p=3, N=[6, 5, 7], geometry="rational", seed=1, bcs=_bcs(3, kind="some")), "poisson", "system"),
    "affine-2d": (dict(dim=2, dof=1, p=3, N=[7, 6], geometry="affine", seed=2), "poisson", "system"),
    "affine-elasticity": (dict(dim=3, dof=3, p=2, N=[5, 4, 4], geometry="affine", seed=4, bcs=_bcs(3, 3, "some")), "elasticity", "system"),
    "affine-mass": (dict(dim=3, dof=2, p=2, N=[5, 4, 6], geometry="rational", seed=5), "mass", "system"),
    "affine-bratu-jacobian": (dict(dim=3, dof=1, p=2, N=[6, 5, 4], geometry="affine", seed=6), "bratu", "jacobian"),
    "affine-bratu-function": (dict(dim=3, dof=1, p=2, N=[6, 5, 4], geometry="affine", seed=7), "bratu", "function"),
}


def run_case(name):
    """Worst ratio |oracle - R| / (u S) of the case's matrix and vector."""
    kw, form, driver = CASES[name]
    kw = dict(kw)
    dim, dof = kw["dim"], kw["dof"]
    orc, _, A = T.setup_case(**kw)
    Ao, bo, tf = oracle_result(orc, dim, dof, form, driver)
    ref = T.reference(orc, dim, tf, A=A, bcs=kw.get("bcs"), loads=kw.get("loads"), driver="function" if "function" in driver else "system")
    worst = 0.0
    if Ao is not None:
        r, c, v = T.matrix_coo(Ao)
        R, S = ref.entries(r, c)
        worst = max(worst, T.compare_entrywise((r, c, v), R, S, 2.0 ** 12, ref, name + " K"))
    if bo is not None:
        rows = np.arange(bo.size)
        if kw.get("box") is not None:      # rows the box's elements touch
            rows = rows[ref.multiplicity(rows) > 0]
        R, S = ref.vector(rows)
        worst = max(worst, T.compare_entrywise((rows, bo[rows]), R, S, 2.0 ** 12, ref, name + " F"))
    return worst, kw.get("geometry") is not None


@pytest.mark.parametrize("name", list(CASES))
def test_reference_against_oracle(name):
    worst, mapped = run_case(name)
    c = T.C_MAP if mapped else T.C_ID
    print("%-24s worst %.2f u S" % (name, worst))
    assert 4 * worst <= c, (name, worst, c)


def test_calibrated_constants():
    """The constants the GPU checks use: 4x the worst oracle ratio, rounded up to a power of two, never above 2^12."""
    worst = {False: 0.0, True: 0.0}
    for name in CASES:
        w, mapped = run_case(name)
        print("%-24s %8.2f" % (name, w))
        worst[mapped] = max(worst[mapped], w)
    c_id, c_map = (2.0 ** int(np.ceil(np.log2(4 * worst[m]))) for m in (False, True))
    print("worst oracle ratio: identity %.2f, affine %.2f -> c_id %g, c_map %g" % (worst[False], worst[True], c_id, c_map))
    assert c_id <= T.C_ID <= 128 and c_map <= T.C_MAP <= 1024 and T.C_ID <= T.C_MAP <= 2 ** 12


def test_longdouble_tables_against_exact_fractions():
    """One graded p = 3 axis: the long double 1-D pair matrices against the same sums in exact rational arithmetic at the same double
    points, weights and Jacobians."""
    finfo = np.finfo(np.longdouble)
    assert finfo.eps < 2.0 ** -60, "np.longdouble is only %d-bit here: the reference cannot resolve u S below the double rounding" % finfo.nmant
    orc, _, _ = T.setup_case(dim=1, dof=1, p=3, N=0, knots=[T.graded_knots(3, 6, 100.0)])
    ax, bs = orc.axis(0), orc.basis(0)
    tab = T.AxisTables(ax, bs)
    Uf = [Fraction(float(x)) for x in ax["U"]]
    p, nnp, nen = ax["p"], ax["nnp"], bs["nen"]
    exact = [[[[Fraction(0)] * nnp for _ in range(nnp)] for _ in range(2)] for _ in range(2)]
    for e in range(bs["nel"]):
        k = int(ax["span"][e])
        xs = [Fraction(float(x)) for x in bs["point"][e]]
        N0, N1 = T.bspline_1d(np.array(Uf, dtype=object), p, k, np.array(xs, dtype=object), dtype=object)
        Ns = (N0, N1)
        for q in range(bs["nqp"]):
            wJ = Fraction(float(bs["weight"][e][q])) * Fraction(float(bs["detJac"][e]))
            for a in range(nen):
                for b in range(nen):
                    A_, B_ = bs["offset"][e] + a, bs["offset"][e] + b
                    for r in range(2):
                        for s in range(2):
                            exact[r][s][A_][B_] += wJ * Ns[r][q, a] * Ns[s][q, b]
    worst = 0.0
    for r in range(2):
        for s in range(2):
            for a in range(nnp):
                for b in range(nnp):
                    S = tab.Pabs[r, s, a, b]
                    if S == 0:
                        assert exact[r][s][a][b] == 0
                        continue
                    x = tab.P[r, s, a, b]
                    hi = float(x)
                    lo = float(x - np.longdouble(hi))
                    err = abs(Fraction(hi) + Fraction(lo) - exact[r][s][a][b])
                    worst = max(worst, float(err) / (T.U_RND * float(S)))
    print("long double tables vs exact: worst %.3g u S" % worst)
    assert worst <= T.C_ID / 16 / 64, worst


class _Shim:
    def __init__(self, rows, cols, vals):
        self.coo = (rows, cols, vals)

    def to_coo_global(self):
        return self.coo


def test_teeth_on_graded_far_band():
    """The oracle's graded p = 3 matrix with ONE far-band entry (|R| < 1e-10 max) off by a relative 1e-6: compare_mats at 1e-12 lets
    it through, the entry-wise check does not.  The same for the smallest free entry of F, off by a relative 1e-7."""
    kw, form, driver = CASES["graded100-p3"]
    orc, _, A = T.setup_case(**kw)
    Ao, bo, tf = oracle_result(orc, 3, 1, form, driver)
    ref = T.reference(orc, 3, tf, bcs=kw["bcs"])
    r, c, v = T.matrix_coo(Ao)
    R, S = ref.entries(r, c)
    T.compare_entrywise((r, c, v), R, S, T.C_ID, ref)
    small = np.flatnonzero((np.abs(R) > 0) & (np.abs(R) < 1e-10 * float(np.abs(R).max())) & (r != c))
    assert small.size > 0
    k = small[0]
    v2 = v.copy()
    v2[k] *= 1 + 1e-6
    compare_mats(_Shim(r, c, v2), Ao, 1e-12)
    with pytest.raises(AssertionError, match="u S"):
        T.compare_entrywise((r, c, v2), R, S, T.C_ID, ref)
    rows = np.arange(bo.size)
    Rb, Sb = ref.vector(rows)
    T.compare_entrywise((rows, bo), Rb, Sb, T.C_ID, ref, "F")
    fx, _ = ref.fixed(rows)
    free = np.flatnonzero(~fx & (Rb != 0))
    k = free[np.argmin(np.abs(Rb[free]))]                # the smallest free entry of F
    b2 = bo.copy()
    b2[k] *= 1 + 1e-7                                   # (F has no entry as small as the far band: a relative 1e-7 here)
    assert np.abs(b2 - bo).max() <= 1e-12 * np.abs(bo).max()
    with pytest.raises(AssertionError, match="u S"):
        T.compare_entrywise((rows, b2), Rb, Sb, T.C_ID, ref, "F")


def test_reference_catches_a_dropped_element_contribution():
    """A box one element short on axis 1: the interior rows next to the missing element fail, the others pass -- the reference is
    sensitive to a seam element whose contribution is dropped."""
    kw, form, driver = CASES["uniform-p3-matrix"]
    orc, _, _ = T.setup_case(**kw)
    Ao, _, tf = oracle_result(orc, 3, 1, form, driver)
    tabs = T.axis_tables(orc, 3, box=[(0, 8), (0, 7), (0, 8)])
    ref = T.TensorRef(tabs, tf, driver="matrix")
    r, c, v = T.matrix_coo(Ao)
    R, S = ref.entries(r, c)
    with pytest.raises(AssertionError):
        T.compare_entrywise((r, c, v), R, S, T.C_ID)
