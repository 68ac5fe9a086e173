"""The point-wise long double reference (pointwise_ref.py) and the row-wise action of tensor_ref.py against the CPU oracle, their own
accuracy, and what they see that the global tolerances do not.

As in test_tensor_reference.py the oracle's distance from the reference, in units of u S, calibrates the constant of the GPU checks:
4 x the worst ratio must stay within the project's EXISTING constants, C_ID on the identity geometry and C_MAP on an affine map; no new
constant is introduced.  Worst oracle ratios met here (printed by the tests; u S):
    Bratu Function / IFunction at a varying state                     5.3   (p = 3, graded 1:100)
    Bratu J X / IJ X (the oracle's matrix times X in double)           7.2 for a standard-normal X, 12.4 for an X spread over twelve decades (p = 3, graded 1:1000)
    Bratu Jacobian / IJacobian entries at a varying state              14.4  (p = 3, graded 1:1000, Dirichlet faces)
    Bratu on affine and rational maps (F, entries, J X)                F 4.2, entries 26.2, J X 7.5  (c = C_MAP)
    Poisson / elasticity System matrix times X, row by row             10.7 on the identity geometry (Poisson p = 3 graded, the wide X), 7.8 on an affine map
    Cahn-Hilliard IFunction                                            0.20  (p = 2, graded)
    Cahn-Hilliard tangent X                                            0.52 on the free rows; 0.99 on a Dirichlet row (m X against the oracle's own sum)
The Cahn-Hilliard bound is loose because S contains sum |N''| |U| for a state near 0.63; that term bounds a summation order a kernel is
free to use, so it stays.

Every entry and every row of every comparison is checked; none is left out.  AFFINE CASES USE UNIFORM OR MILDLY NON-UNIFORM KNOTS ONLY:
under an affine map a 1:1000 graded axis puts the oracle itself about 1000 u S away, because the control-point interpolation of the map
then rounds at a scale S does not contain (test_gpu_entrywise.py keeps its affine cases on uniform knots for the same reason).  Graded
meshes are exercised on the identity geometry."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import oracle_api as O
import pointwise_ref as PW
import tensor_ref as T

LD = T.LD
LAM, SHIFT = 3.5, 4.0
CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0)
EL = (1.5, 0.8)
_k = T.graded_knots


def _bcs(kind="all"):
    return {(d, s, 0): 0.2 + 0.1 * d - 0.15 * s for d in range(3) for s in range(2) if kind == "all" or (d + s) % 2 == 0}


BC3 = {(0, 0, 0): 0.2, (1, 1, 0): -0.1, (2, 0, 0): 0.3}
BC_CH = {(0, 0, 0): 0.6, (0, 1, 0): 0.66, (1, 1, 0): 0.61, (2, 0, 0): 0.65}

# name: setup_case keywords (3-D, one field)
BRATU = {
    "p3-graded100": dict(p=3, N=0, knots=[_k(3, 6, 100.0), _k(3, 5, 0.01), _k(3, 6, 100.0)], bcs=_bcs()),
    "p3-graded1000": dict(p=3, N=0, knots=[_k(3, 5, 1000.0), _k(3, 4, 1000.0), _k(3, 5, 0.001)], bcs=_bcs("some")),
    "p2-graded-odd": dict(p=2, N=0, knots=[_k(2, 5, 100.0), _k(2, 4, 0.01), _k(2, 3, 1000.0)], bcs=_bcs("some")),
    "p3-uniform": dict(p=3, N=[4, 4, 4]),
    "p3-C1": dict(p=3, N=[4, 4, 3], C=[1, 2, 2], bcs=_bcs("some")),
    "p2-periodic": dict(p=2, N=[6, 4, 5], periodic=[True, False, True], bcs={(1, 0, 0): 0.25}),
    "mixed-degrees": dict(p=[2, 3, 2], N=[4, 3, 5], nqp=[3, 4, 4], bcs={(1, 0, 0): 0.4}),
    "p3-affine": dict(p=3, N=[5, 4, 4], geometry="affine", seed=1, bcs=BC3),
    "p2-affine-odd": dict(p=2, N=[5, 4, 3], geometry="affine", seed=5, bcs=_bcs()),
    "p3-rational": dict(p=3, N=[4, 4, 3], geometry="rational", seed=3, bcs=BC3),
}
CAHN = {
    "p2-odd": dict(p=2, N=[5, 4, 3]),
    "p2-periodic": dict(p=2, N=[6, 4, 5], periodic=[True, True, True]),
    "p2-graded": dict(p=2, N=0, knots=[_k(2, 5, 100.0), _k(2, 4, 0.01), _k(2, 3, 1000.0)]),
    "p3-C1": dict(p=3, N=[4, 5, 3], C=[1, 1, 1]),
    "p2-dirichlet": dict(p=2, N=[5, 4, 3], bcs=BC_CH),
    "p3-periodic-dirichlet": dict(p=3, N=[5, 4, 4], periodic=[False, True, False], bcs={(0, 1, 0): 0.64, (2, 0, 0): 0.61}),
}


def _el_bcs():
    return {(0, 0, 0): 0.0, (0, 0, 1): 0.5, (0, 0, 2): -0.25, (2, 1, 0): 1.0, (1, 0, 2): 0.75}


# name: (setup_case keywords, form)
LINEAR = {
    "poisson-p3-graded": (dict(dof=1, p=3, N=0, knots=[_k(3, 6, 100.0), _k(3, 5, 0.01), _k(3, 6, 100.0)], bcs=_bcs()), "poisson"),
    "poisson-p2-graded-odd": (dict(dof=1, p=2, N=0, knots=[_k(2, 5, 100.0), _k(2, 4, 0.01), _k(2, 3, 1000.0)], bcs=_bcs("some")), "poisson"),
    "poisson-p2-periodic": (dict(dof=1, p=2, N=[6, 4, 5], periodic=[True, False, True], bcs={(1, 0, 0): 2.0}), "poisson"),
    "poisson-p3-affine": (dict(dof=1, p=3, N=[5, 4, 4], geometry="affine", seed=1, bcs=_bcs()), "poisson"),
    "poisson-p3-C1": (dict(dof=1, p=3, N=[4, 4, 3], C=[1, 2, 2], bcs=_bcs("some")), "poisson"),
    "poisson-mixed-degrees": (dict(dof=1, p=[2, 3, 2], N=[4, 3, 5], nqp=[3, 4, 4], bcs={(1, 0, 0): 1.0}), "poisson"),
    "poisson-p3-rational": (dict(dof=1, p=3, N=[4, 4, 3], geometry="rational", seed=3, bcs=BC3), "poisson"),
    "elasticity-p2": (dict(dof=3, p=2, N=[4, 3, 3], bcs=_el_bcs()), "elasticity"),
    "elasticity-p3-affine": (dict(dof=3, p=3, N=[4, 3, 3], geometry="affine", seed=4, bcs=_el_bcs()), "elasticity"),
}


def wide(n, seed=3):
    """standard normal times magnitudes spread over 10^-6 ... 10^6"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)


def bratu_vectors(n, seed=7):
    rng = np.random.default_rng(seed)
    return 0.3 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)       # U, V, X


def cahn_vectors(n, seed=7):
    rng = np.random.default_rng(seed)
    return 0.63 + 0.05 * (2 * rng.random(n) - 1), rng.standard_normal(n), rng.standard_normal(n)


def _setup(kw):
    kw = dict(kw)
    kw.setdefault("dof", 1)
    orc, _, A = T.setup_case(dim=3, engine=False, **kw)
    return orc, A, kw.get("bcs")


BIG = 2.0 ** 12        # the comparisons measure; the assertion is 4 * worst <= c, on every row and entry


def _assert_calibrated(name, worst, mapped):
    c = T.C_MAP if mapped else T.C_ID
    print("%-24s %s" % (name, "  ".join("%s %.2f" % kv for kv in worst.items())))
    for what, w in worst.items():
        assert 4 * w <= c, (name, what, w, c)


@pytest.mark.parametrize("name", list(BRATU))
def test_bratu_oracle_inside_the_bound_at_a_varying_state(name):
    orc, A, bcs = _setup(BRATU[name])
    pw = PW.PointwiseRef(orc, A=A, bcs=bcs)
    U, V, X = bratu_vectors(orc.global_size())
    lam = C.c_double(LAM)
    worst = {}
    worst["F"] = PW.compare_rows(orc.compute_function("orc_form_bratu_function", lam, U), *pw.bratu_function(LAM, U), BIG, pw.tref, name + " F")
    worst["IF"] = PW.compare_rows(orc.compute_ifunction("orc_form_bratu_ifunction", lam, SHIFT, V, 0.0, U), *pw.bratu_function(LAM, U, V), BIG, pw.tref, name + " IF")
    J = orc.compute_jacobian("orc_form_bratu_jacobian", lam, U)
    IJ = orc.compute_ijacobian("orc_form_bratu_ijacobian", lam, SHIFT, V, 0.0, U)
    for tag, M, shift in (("J", J, 0.0), ("IJ", IJ, SHIFT)):
        r, c, v = T.matrix_coo(M)
        worst[tag] = T.compare_entrywise((r, c, v), *pw.bratu_entries(LAM, U, r, c, shift), BIG, pw.tref, name + " " + tag)
        for xt, Xv in (("X", X), ("Xwide", wide(X.size))):
            worst[tag + " " + xt] = PW.compare_rows(M.scipy() @ Xv, *pw.bratu_action(LAM, U, Xv, shift), BIG, pw.tref, name + " " + tag + " " + xt)
    _assert_calibrated(name, worst, A is not None)


@pytest.mark.parametrize("name", list(CAHN))
def test_cahn_hilliard_oracle_inside_the_bound(name):
    orc, A, bcs = _setup(CAHN[name])
    pw = PW.PointwiseRef(orc, bcs=bcs)
    U, V, X = cahn_vectors(orc.global_size())
    ctx = O.CahnHilliardCtx(*CH)
    worst = {}
    worst["IF"] = PW.compare_rows(orc.compute_ifunction("orc_form_ch_residual", ctx, 250.0, V, 0.0, U), *pw.ch_ifunction(CH, U, V), BIG, pw.tref, name + " IF")
    M = orc.compute_ijacobian("orc_form_ch_tangent", ctx, 250.0, V, 0.0, U).scipy()
    for xt, Xv in (("X", X), ("Xwide", wide(X.size))):
        worst["tangent " + xt] = PW.compare_rows(M @ Xv, *pw.ch_action(CH, 250.0, U, Xv), BIG, pw.tref, name + " tangent " + xt)
    _assert_calibrated(name, worst, False)


def linear_reference(orc, kw, form, A):
    tf = T.poisson(3) if form == "poisson" else T.elasticity(*EL)
    return T.reference(orc, 3, tf, A=A, bcs=kw.get("bcs"), driver="system")


@pytest.mark.parametrize("name", list(LINEAR))
def test_linear_oracle_matrix_times_x_row_by_row(name):
    kw, form = LINEAR[name]
    orc, A, _ = _setup(kw)
    ref = linear_reference(orc, kw, form, A)
    if form == "poisson":
        M = orc.compute_system("orc_form_poisson")[0].scipy()
    else:
        M = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))[0].scipy()
    n = orc.global_size()
    worst = {}
    for xt, X in (("X", np.random.default_rng(29).standard_normal(n)), ("Xwide", wide(n))):
        worst[xt] = PW.compare_rows(M @ X, *ref.action(X), BIG, ref, name + " " + xt)
    _assert_calibrated(name, worst, A is not None)


@pytest.mark.parametrize("name", ["p3-graded100", "p2-periodic", "p3-affine"])
def test_constant_state_agrees_with_the_tensor_reference(name):
    """At U = c the point-wise reference is the tensor-product one: the Function rows and the Jacobian entries agree to long double
    rounding, 1/8 u S (the bound test_tensor_reference.py sets for the long double tables; u = 2^10 long double units)."""
    kw = dict(BRATU[name])
    c0 = 0.3
    if kw.get("bcs"):
        kw["bcs"] = {k: c0 for k in kw["bcs"]}
    orc, A, bcs = _setup(kw)
    pw = PW.PointwiseRef(orc, A=A, bcs=bcs)
    n = orc.global_size()
    U = np.full(n, c0)
    rows = np.arange(n)
    Rt, St = T.reference(orc, 3, T.bratu(3, LAM, c0), A=A, bcs=bcs, driver="function").vector(rows)
    R, S = pw.bratu_function(LAM, U)
    err = np.abs(R - Rt)
    assert np.all(err <= LD(T.U_RND) / 8 * St), float((err / (LD(T.U_RND) * np.where(St > 0, St, 1))).max())
    r, c, _ = T.matrix_coo(orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(LAM), U))
    for shift in (0.0, SHIFT):
        Rt, St = T.reference(orc, 3, T.bratu(3, LAM, c0, shift=shift), A=A, bcs=bcs).entries(r, c)
        R, S = pw.bratu_entries(LAM, U, r, c, shift)
        err = np.abs(R - Rt)
        assert np.all(err <= LD(T.U_RND) / 8 * St), float((err / (LD(T.U_RND) * np.where(St > 0, St, 1))).max())
        assert np.array_equal(S == 0, St == 0)
    print("%s: constant state, worst |R_pw - R_tensor| = %.3g u S" % (name, float((err / (LD(T.U_RND) * np.where(St > 0, St, 1))).max())))


def test_second_derivative_table_against_exact_fractions():
    """One graded p = 3 axis: the long double collocation tables (r = 0, 1, 2) against exact rational arithmetic at the same points."""
    orc, _, _ = T.setup_case(dim=1, dof=1, p=3, N=0, knots=[_k(3, 6, 100.0)])
    ax, bs = orc.axis(0), orc.basis(0)
    B, w = PW.collocation(ax, bs)
    Uf = np.array([Fraction(float(x)) for x in ax["U"]], dtype=object)
    nqp, nen = bs["nqp"], bs["nen"]
    worst = 0.0
    for e in range(bs["nel"]):
        xs = np.array([Fraction(float(x)) for x in bs["point"][e]], dtype=object)
        exact = T.bspline_1d_d2(Uf, ax["p"], int(ax["span"][e]), xs, dtype=object)
        for r in range(3):
            for q in range(nqp):
                row = B[r, e * nqp + q]
                assert np.count_nonzero(row) <= nen
                for a in range(nen):
                    x = row[bs["offset"][e] + a]
                    hi = float(x)
                    lo = float(x - LD(hi))
                    ex = Fraction(exact[r][q, a])
                    if r == 2:
                        assert ex != 0                    # (a cubic's second derivative vanishes at no Gauss point here)
                    err = abs(Fraction(hi) + Fraction(lo) - ex)
                    worst = max(worst, float(err / abs(ex)) / T.U_RND if ex != 0 else float(err))
        assert w[e * nqp] == LD(bs["weight"][e][0]) * LD(bs["detJac"][e])
    # exact second derivatives sum to zero over the functions of a span (the partition of unity differentiated twice)
    assert sum(exact[2][0]) == 0 and sum(exact[1][0]) == 0 and sum(exact[0][0]) == 1
    print("collocation tables vs exact: worst relative error %.3g u" % worst)
    assert worst <= 1.0 / 16


def test_colouring_separates_every_rows_columns():
    for kw in (BRATU["p3-graded100"], BRATU["p2-periodic"], BRATU["p3-C1"]):
        orc, A, bcs = _setup(kw)
        ref = T.reference(orc, 3, T.poisson(3), bcs=bcs)
        colour, ncol, per_axis = PW.colouring(ref.tabs)
        cols, valid = ref.stencil(np.arange(orc.global_size()))
        for i in range(cols.shape[0]):
            cc = colour[cols[i][valid[i]]]
            assert np.unique(cc).size == cc.size
        assert ncol == int(np.prod(per_axis)) and colour.max() == ncol - 1
        print(per_axis, ncol)


def test_teeth_row_with_the_smallest_scale():
    """The oracle's J X on the 1:1000 graded p = 3 mesh with the row of the smallest non-zero S (the corner of the short spans) off
    by a relative 1e-6: the global check of test_gpu_matrix_action.py (1e-11 of max S) accepts it, the row-wise check does not."""
    from test_gpu_matrix_action import _check, _products
    kw = dict(BRATU["p3-graded1000"], bcs={(0, 1, 0): 0.2, (1, 1, 0): -0.1, (2, 0, 0): 0.3})     # Dirichlet on the coarse faces
    orc, A, bcs = _setup(kw)
    pw = PW.PointwiseRef(orc, bcs=bcs)
    U, _, X = bratu_vectors(orc.global_size())
    M = orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(LAM), U).scipy()
    Y = M @ X
    R, S = pw.bratu_action(LAM, U, X)
    PW.compare_rows(Y, R, S, T.C_ID, pw.tref)
    old = _products(M, X)
    _check(Y, X, *old, 1e-11)
    free = np.flatnonzero(~pw.fx & (S > 0))
    k = free[np.argmin(S[free])]
    Y2 = Y.copy()
    Y2[k] += 1e-6 * abs(float(R[k]))
    assert Y2[k] != Y[k] and pw.fx.any()
    _check(Y2, X, *old, 1e-11)
    with pytest.raises(AssertionError, match="u S"):
        PW.compare_rows(Y2, R, S, T.C_ID, pw.tref)


def test_teeth_state_read_from_another_point():
    """A Bratu IJacobian whose lambda e^u is read from the wrong point of one element (the element's point values reversed along axis
    0).  At a constant state that is the identity: the constant-state entry-wise check of test_gpu_entrywise.py passes it.  At a
    varying state the entry-wise check against the point-wise reference rejects it."""
    kw = dict(BRATU["p3-graded100"])
    c0 = 0.3
    kw["bcs"] = {k: c0 for k in kw["bcs"]}
    orc, A, bcs = _setup(kw)
    pw = PW.PointwiseRef(orc, bcs=bcs)
    nq = orc.basis(0)["nqp"]
    el = (2, 1, 3)                                      # an interior element (axis 0, 1, 2)

    def wrong_point(eu):
        out = eu.copy()
        q2, q1, q0 = (slice(e * nq, (e + 1) * nq) for e in el[::-1])
        out[q2, q1, q0] = eu[q2, q1, q0][:, :, ::-1]
        return out

    n = orc.global_size()
    r, c, _ = T.matrix_coo(orc.create_mat())
    # the constant state: the wrong kernel's matrix passes the existing check
    Uc = np.full(n, c0)
    wrong = pw.bratu_entries(LAM, Uc, r, c, SHIFT, permute=wrong_point)[0].astype(np.float64)
    ref = T.reference(orc, 3, T.bratu(3, LAM, c0, shift=SHIFT), bcs=bcs)
    T.compare_entrywise((r, c, wrong), *ref.entries(r, c), T.C_ID, ref)
    # a varying state: the right matrix passes, the wrong one does not
    U = bratu_vectors(n)[0]
    R, S = pw.bratu_entries(LAM, U, r, c, SHIFT)
    T.compare_entrywise((r, c, R.astype(np.float64)), R, S, T.C_ID, pw.tref)
    wrong = pw.bratu_entries(LAM, U, r, c, SHIFT, permute=wrong_point)[0].astype(np.float64)
    with pytest.raises(AssertionError, match="u S"):
        T.compare_entrywise((r, c, wrong), R, S, T.C_ID, pw.tref)
