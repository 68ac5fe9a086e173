"""tests/probe_ref.py, the long double restatement of the probe's contract, against two independent witnesses on the CPU, and the
constants of its bound |E - R| <= c u S.

  scipy.interpolate.BSpline   values and derivatives to order 3 on graded knot vectors with a C0 knot: at the knots, at both ends, at
                              random points (the span rule, the 1-D rows).
  the oracle's tabulation     orc.element(ID): shape[0..3], point, mapping -- the reference's own chain (rationalise per basis function,
                              geometry map, inverse map, shape functions) in double precision, at the quadrature points of several elements
                              on the identity, an affine map, the polynomial warp and the NURBS map; dof 1 and 3, 2-D and 3-D.
The oracle's doubles stay inside C_ID / C_MAP for orders 0..2; its worst order-3 ratio on a map fixes probe_ref.C3.  Five perturbed
references must reject the witnesses.  The known answer of the reference's own probe test (the cubic of test/IGAProbe.c on a p = 3
space, coefficients by tensor-product interpolation at the Greville points) holds at that test's tolerances.
"""
import functools
import math

import numpy as np
import pytest

import oracle_api as O
import probe_ref as PR
from common import greville, make_pair

LD = PR.LD

CASES = {"2d-dof1": (2, 1, [2, 3], [4, 3]), "2d-dof3": (2, 3, [3, 2], [3, 4]), "3d-dof1": (3, 1, [2, 3, 1], [3, 2, 3]), "3d-dof3": (3, 3, [3, 3, 3], [2, 3, 2])}


def _knots(p, n, seed):
    """graded spans with one C0 knot of full multiplicity in the middle"""
    import tensor_ref as T
    U = T.graded_knots(p, n, 1.7, seed=seed)
    mid = np.unique(U)[max(1, n // 2)]
    return np.sort(np.concatenate([U, [mid] * (p - 1)]))


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    dim, dof, p, N = CASES[name]
    knots = [_knots(p[d], N[d], 10 + d) for d in range(dim)]
    orc, _ = make_pair(dim, dof, p, N, knots=knots, order=3, engine=False)
    X, W = PR.geometry(orc, dim, kind)
    if X is not None:
        orc.set_geometry(X, W)
    ref = PR.ProbeRef(PR.axes_of(orc), dof, X, W)
    coef = np.random.default_rng(5).uniform(-1, 1, orc.global_size())
    nel = [orc.axis(d)["nel"] for d in range(dim)]
    ids = sorted({tuple(0 for _ in nel), tuple(n - 1 for n in nel), tuple(n // 2 for n in nel), tuple((n - 1) * (d % 2) for d, n in enumerate(nel))})
    return orc, ref, coef, ids, (X, W)


@functools.lru_cache(maxsize=None)
def _ratios(name, kind):
    """worst ratio of the oracle's doubles per derivative order, over the elements of the case"""
    orc, ref, coef, ids, _ = _case(name, kind)
    worst = [0.0] * 4
    for ID in ids:
        for der in range(4):
            pts, E = PR.oracle_at_element(orc, ID, coef, der)
            R, S = ref.evaluate(coef, pts, der)
            worst[der] = max(worst[der], PR.compare(E, R, S, float("inf"), "%s %s element %s der %d" % (name, kind, ID, der)))
    return worst


def test_rows_against_scipy():
    from scipy.interpolate import BSpline
    rng = np.random.default_rng(1)
    for p in (1, 2, 3, 5):
        U = _knots(p, 6, 20 + p)
        n = len(U) - p - 1
        c = rng.uniform(-1, 1, n)
        x = np.concatenate([np.unique(U), [U[0], U[-1]], rng.uniform(U[0], U[-1], 40)])
        ref = PR.ProbeRef([dict(p=p, U=U, nnp=n)], 1)
        spl = BSpline(U, c, p, extrapolate=False)
        for der in range(4):
            R, S = ref.evaluate(c, x[:, None], der)
            E = spl(x, nu=der) if der <= p else np.zeros_like(x)
            PR.compare(E.reshape(R.shape), R, S, 4 * PR.C_ID, "scipy p=%d der=%d" % (p, der))
        # the span rule itself
        k = PR.find_span(U, p, x)
        assert np.all((U[k] <= x) & ((x < U[k + 1]) | (x == U[-1]))) and np.all(U[k] < U[k + 1])
        assert np.all(k[x == U[-1]] == n - 1)


@pytest.mark.parametrize("kind", PR.GEOMETRIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_inside_the_bounds(name, kind):
    worst = _ratios(name, kind)
    mapped = kind != "identity"
    print("%s %s: worst ratios of the oracle's doubles, der 0..3: %s" % (name, kind, ", ".join("%.2f" % w for w in worst)))
    for der in range(3):
        assert worst[der] <= PR.bound(der, mapped), (name, kind, der, worst[der])
    assert worst[3] <= PR.bound(3, mapped)
    # geom_map: the oracle's mapX[0] at the same points
    orc, ref, coef, ids, _ = _case(name, kind)
    el = orc.element(list(ids[-1]))
    R, S = ref.geom_map(el["point"])
    E = el["mapX0"] if mapped else el["point"]
    PR.compare(E, R, S, PR.bound(0, mapped), "geom_map")


def test_c3_is_four_times_the_oracles_worst_ratio():
    worst = max(_ratios(name, kind)[3] for name in CASES for kind in PR.GEOMETRIES if kind != "identity")
    print("worst order-3 ratio of the oracle on a map: %.3f" % worst)
    assert worst <= PR.WORST3, "probe_ref.WORST3 is out of date: measured %.3f" % worst
    assert worst >= PR.WORST3 / 2, "probe_ref.WORST3 is not the measured ratio: measured %.3f" % worst
    assert PR.C3 == max(PR.C_MAP, 2 ** math.ceil(math.log2(4 * PR.WORST3)))


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_mutants_reject_the_witnesses():
    # three of them against the oracle's tabulation on the NURBS map
    orc, ref, coef, ids, (X, W) = _case("3d-dof1", "nurbs")
    for wrong, der in (("weights", 0), ("transpose", 1), ("mixed3", 3)):
        bad = PR.ProbeRef(PR.axes_of(orc), orc.dof, X, W, wrong=wrong)
        pts, E = PR.oracle_at_element(orc, ids[1], coef, der)
        PR.compare(E, *ref.evaluate(coef, pts, der), PR.bound(der, True))
        _rejects(lambda: PR.compare(E, *bad.evaluate(coef, pts, der), PR.bound(der, True)))
    # the span rule against the oracle's 1-D rows (IGA_Basis_BSpline) at a C0 knot and at the upper end
    p, n = 2, 5
    U = _knots(p, n, 31)
    nf = len(U) - p - 1
    c = np.random.default_rng(2).uniform(0.5, 1.5, nf)
    knot = np.unique(U)[max(1, n // 2)]
    good = PR.ProbeRef([dict(p=p, U=U, nnp=nf)], 1)
    for wrong, x in (("left", knot), ("endspan", U[-1])):
        k = int(PR.find_span(U, p, [x])[0])
        ders = O.bspline_ders(k, x, p, 1, U)                                      # [p + 1][der]
        for der in (0, 1):
            E = np.array([[ders[:, der] @ c[k - p:k + 1]]])
            PR.compare(E.reshape(1, 1, *([1] * der)), *good.evaluate(c, [[x]], der), PR.C_ID)
            bad = PR.ProbeRef([dict(p=p, U=U, nnp=nf)], 1, wrong=wrong)
            if wrong == "left" and der == 0:
                continue                                                          # (the value is continuous at a C0 knot: only the derivative tells)
            _rejects(lambda: PR.compare(E.reshape(1, 1, *([1] * der)), *bad.evaluate(c, [[x]], der), PR.C_ID))


def cubic(x):
    """the cubic of the reference's probe test and its closed-form derivatives at the points x [n, 3]"""
    n = len(x)
    f = (x ** 3).sum(1) + (x ** 2).sum(1) + x[:, 0] * x[:, 1] + x[:, 0] * x[:, 2] + x[:, 1] * x[:, 2] + 1
    g = 3 * x ** 2 + 2 * x + (x.sum(1)[:, None] - x)
    h = np.ones((n, 3, 3))
    t = np.zeros((n, 3, 3, 3))
    for i in range(3):
        h[:, i, i] = 6 * x[:, i] + 2
        t[:, i, i, i] = 6
    return f, g, h, t


KNOWN_TOL = ((1e-6, 1e-4), (1e-5, 1e-3), (1e-4, 1e-2), (1e-3, 1e-1))      # (rtol, atol) of the reference's test, der 0..3
KNOWN_POINTS = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]])


def known_answer_coefficients(axes):
    """the cubic in a p = 3 space: tensor-product interpolation at the Greville points (exact: the cubic is in the space)"""
    g = [greville(a["U"], a["p"]) for a in axes]
    A = []
    for a, gd in zip(axes, g):
        nf = len(a["U"]) - a["p"] - 1
        M = np.zeros((nf, nf))
        k = PR.find_span(a["U"], a["p"], gd)
        for r, (kk, x) in enumerate(zip(k, gd)):
            M[r, kk - a["p"]:kk + 1] = PR.rows_1d(a["U"], a["p"], int(kk), [x], 0)[0][0].astype(np.float64)
        A.append(np.linalg.inv(M))
    Z, Y, Xg = np.meshgrid(g[2], g[1], g[0], indexing="ij")
    F = cubic(np.stack([Xg.ravel(), Y.ravel(), Z.ravel()], axis=-1))[0].reshape(Z.shape)
    return np.einsum("kc,jb,ia,cba->kji", A[2], A[1], A[0], F).reshape(-1)


def check_known_answer(evaluate):
    exact = cubic(KNOWN_POINTS)
    for der, (rtol, atol) in enumerate(KNOWN_TOL):
        got = np.asarray(evaluate(der), dtype=np.float64).reshape(exact[der].shape)
        assert np.all(np.abs(got - exact[der]) <= atol + rtol * np.abs(exact[der])), (der, np.abs(got - exact[der]).max())


def test_known_answer():
    orc, _ = make_pair(3, 1, 3, [4, 3, 5], engine=False)
    axes = PR.axes_of(orc)
    coef = known_answer_coefficients(axes)
    ref = PR.ProbeRef(axes, 1)
    check_known_answer(lambda der: ref.evaluate(coef, KNOWN_POINTS, der)[0])
