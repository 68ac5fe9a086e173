"""Fast diagonalisation in the C ABI (include/petiga_amd.h) and its Python view, and its host half (IGXFastDiagSetUp makes no HIP call):
the three calls are declared, exported and bound with the header's argument counts; the generalised eigenpairs IGXFastDiagGetAxis hands
back are held against scipy.linalg.eigh on 1-D matrices rebuilt here from the knots (tests/fast_diag_ref.py: scipy's BSpline, numpy's
Gauss-Legendre rule); the count of zeroed modes; the refusals that need no GPU, each by code and word.

Bounds of the eigenpairs: |Lambda - Lambda_scipy| / lambda_max, max|U^T M U - I| and max|K U - M U Lambda| / lambda_max, each at most
8 x the same quantity of scipy's own eigenvectors (for Lambda that quantity is 0) with a floor of 1e-13: the factor covers a different but
equally stable algorithm, the floor the cases where scipy's own residual is a few ulps."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

from fast_diag_ref import axis_matrices

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
CALLS = {"IGXFastDiagSetUp": 4, "IGXFastDiagApply": 3, "IGXFastDiagGetAxis": 7}


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
    doubles = [i for i, a in enumerate(decl[name].split(",")) if a.strip().startswith("double") and "[" not in a]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == doubles


def test_python_view_has_the_three_calls():
    import petiga_amd as P
    for m in ("fast_diag_setup", "fast_diag_apply", "fast_diag_get_axis"):
        assert callable(getattr(P.IGX, m))


def test_header_says_it_ignores_the_geometry():
    text = open(HEADER).read()
    at = text.index("IGXFastDiagSetUp")
    assert "IGNORES THE GEOMETRY" in text[max(0, at - 6000):at]


def _uniform(p, N, C_=None, periodic=False):
    """the knot vector IGAAxisInitUniform makes on [0, 1] (src/petigaaxis.c:401-456)"""
    C_ = p - 1 if C_ is None else C_
    s = p - C_
    m = 2 * (p + 1) + (N - 1) * s - 1
    n = m - p - 1
    U = np.zeros(m + 1)
    U[m - p:] = 1.0
    k = p + 1
    for b in range(1, N):
        for _ in range(s):
            U[k] = b / N
            k += 1
    if periodic:
        for k in range(C_ + 1):
            U[C_ - k] = U[p] - U[m - p] + U[n - k]
            U[m - C_ + k] = U[m - p] - U[p] + U[p + 1 + k]
    return U


# name -> (p, knots, periodic, nqp)
AXES = {
    "p2 non-uniform": (2, [0, 0, 0, 0.1, 0.35, 0.4, 0.75, 1, 1, 1], False, None),
    "p3 non-uniform": (3, [0, 0, 0, 0, 0.2, 0.3, 0.65, 0.8, 1, 1, 1, 1], False, None),
    "p3 with a C0 knot": (3, [0, 0, 0, 0, 0.25, 0.5, 0.5, 0.5, 0.7, 1, 1, 1, 1], False, None),
    "p2 periodic": (2, _uniform(2, 7, periodic=True), True, None),
    "p3 periodic": (3, _uniform(3, 6, periodic=True), True, None),
    "p2 nqp = p + 2": (2, _uniform(2, 9), False, 4),
    "p7 with 6 elements": (7, _uniform(7, 6), False, None),
    "p3 uniform, 17 elements": (3, _uniform(3, 17), False, None),
    # axis lengths of real runs: m = 72 and 150 (the row-tile ladder of the device half), 260 (two row blocks; the benchmark's 256^3 at
    # p = 3 has 259), the ill-conditioned p = 7 at that length, and the exact eigenvalue pairs of a periodic axis
    "p2 uniform, 70 elements": (2, _uniform(2, 70), False, None),
    "p3 uniform, 147 elements": (3, _uniform(3, 147), False, None),
    "p2 uniform, 258 elements": (2, _uniform(2, 258), False, None),
    "p7 uniform, 250 elements": (7, _uniform(7, 250), False, None),
    "p2 periodic, 300 elements": (2, _uniform(2, 300, periodic=True), True, None),
}
OBSERVED = {}


def _engine_with_axis0(p, U, periodic, nqp):
    """dof = 4: field 0 free at both ends of axis 0, field 1 fixed at the first function, field 2 at the last, field 3 at both"""
    import petiga_amd as P
    g = P.IGX(3, 4)
    g.axis_knots(0, p, U, periodic=periodic)
    if nqp:
        g.set_quadrature(0, nqp)
    g.axis_uniform(1, 2, 2)
    g.axis_uniform(2, 1, 3)
    g.setup()
    for f, sides in ((1, (0,)), (2, (1,)), (3, (0, 1))):
        for s in sides:
            g.set_boundary_value(0, s, f, 0.0)
    return g


@pytest.mark.parametrize("name", sorted(AXES))
def test_eigenpairs_against_scipy(name):
    p, U, periodic, nqp = AXES[name]
    M, K, _ = axis_matrices(U, p, nqp, periodic)
    g = _engine_with_axis0(p, U, periodic, nqp)
    g.fast_diag_setup(1.0, [1.0, 1.0, 1.0])
    n = M.shape[0]
    worst = [0.0, 0.0, 0.0]
    for f in range(4):
        lo, hi = (0, 0) if periodic else (int(f in (1, 3)), int(f in (2, 3)))      # a periodic axis has no faces
        first, m, lam, V = g.fast_diag_get_axis(0, f)
        assert (first, m) == (lo, n - lo - hi)
        Ms, Ks = M[lo:n - hi, lo:n - hi], K[lo:n - hi, lo:n - hi]
        lam_s, V_s = sla.eigh(Ks, Ms)
        lmax = lam_s.max()
        assert np.all(np.diff(lam) >= 0), "Lambda is not ascending"

        def quality(l, W):
            return np.abs(W.T @ Ms @ W - np.eye(m)).max(), np.abs(Ks @ W - Ms @ W * l[None, :]).max() / lmax

        e_lam = np.abs(lam - lam_s).max() / lmax
        e_orth, e_res = quality(lam, V)
        s_orth, s_res = quality(lam_s, V_s)
        print("%s, field %d (first %d, m %d): |dLambda|/lmax %.2e; |U^T M U - I| %.2e (scipy %.2e); |K U - M U L|/lmax %.2e (scipy %.2e)"
              % (name, f, first, m, e_lam, e_orth, s_orth, e_res, s_res))
        worst = [max(a, b) for a, b in zip(worst, (e_lam, e_orth, e_res))]
        assert e_lam <= 1e-13
        assert e_orth <= max(8 * s_orth, 1e-13)
        assert e_res <= max(8 * s_res, 1e-13)
    OBSERVED[name] = worst


def test_axes_one_and_two_are_handed_back_too():
    g = _engine_with_axis0(*AXES["p2 non-uniform"])
    g.set_boundary_value(2, 1, 0, 0.0)
    g.fast_diag_setup(0.0, [1.0, 2.0, 3.0])
    first, m, lam, V = g.fast_diag_get_axis(1, 0)
    M, K, _ = axis_matrices(_uniform(2, 2), 2)
    assert (first, m) == (0, 4) and np.abs(lam - sla.eigh(K, M, eigvals_only=True)).max() <= 1e-13 * lam.max()
    first, m, lam, V = g.fast_diag_get_axis(2, 0)
    assert (first, m) == (0, 3)
    assert g.fast_diag_get_axis(2, 1)[:2] == (0, 4)
    import petiga_amd as P
    with pytest.raises(P.IGXError) as e:
        g.fast_diag_get_axis(0, 4)
    assert e.value.code == 63


def _poisson_box(dof=1, periodic=False):
    import petiga_amd as P
    g = P.IGX(3, dof)
    for i, N in enumerate((4, 3, 3)):
        g.axis_uniform(i, 2, N, periodic=periodic and i == 0)
    g.setup()
    return g


def test_nzeroed():
    g = _poisson_box()
    assert g.fast_diag_setup(0.0, [1.0, 1.0, 1.0]) == 1           # the constant of pure-Neumann Poisson
    assert g.fast_diag_setup(1.0, [1.0, 1.0, 1.0]) == 0           # (a second set-up replaces the first)
    assert g.fast_diag_setup(1.0, [0.0, 0.0, 0.0]) == 0
    g.set_boundary_value(1, 1, 0, 0.0)
    assert g.fast_diag_setup(0.0, [1.0, 1.0, 1.0]) == 0
    g2 = _poisson_box(dof=2)
    g2.set_boundary_value(0, 0, 1, 0.0)
    assert g2.fast_diag_setup(0.0, [1.0, 1.0, 1.0]) == 1          # field 0 keeps its constant, field 1 does not


def test_refusals_by_code_and_word():
    import petiga_amd as P
    g = P.IGX(2, 1)
    for i in range(2):
        g.axis_uniform(i, 2, 4)
    g.setup()
    with pytest.raises(P.IGXError) as e:
        g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    assert e.value.code == 56 and "fast diagonalisation" in str(e.value) and "dim" in str(e.value), str(e.value)

    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.set_comm(2, 0)
    g.set_processors(1, 2)
    g.setup()
    with pytest.raises(P.IGXError) as e:
        g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    assert e.value.code == 56 and "fast diagonalisation" in str(e.value) and "rank" in str(e.value), str(e.value)

    g = _poisson_box()
    for alpha, beta in ((0.0, [1.0, -1.0, 1.0]), (-1.0, [1.0, 1.0, 1.0]), (0.0, [0.0, 0.0, 0.0])):
        with pytest.raises(P.IGXError) as e:
            g.fast_diag_setup(alpha, beta)
        assert e.value.code == 63 and "fast diagonalisation" in str(e.value), str(e.value)

    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    with pytest.raises(P.IGXError) as e:      # before IGXSetUp
        g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    assert e.value.code == 58


def test_apply_before_setup_is_an_order_error():
    """IGXFastDiagApply checks the order before it looks at its vectors, so this needs no device"""
    import petiga_amd as P
    g = _poisson_box()
    rc = P.lib().IGXFastDiagApply(g.h, None, None)
    assert rc == 58 and "IGXFastDiagSetUp" in P.lib().IGXGetLastError().decode()
    g.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    g.setup()                                  # IGXSetUp drops the state
    assert P.lib().IGXFastDiagApply(g.h, None, None) == 58
