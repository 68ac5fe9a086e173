"""GPU parity of the matrix-free actions (include/petiga_amd.h: IGXComputeMatrixAction / JacobianAction / IJacobianAction;
petiga_amd/csrc/vec_sumfact.hpp, ACTION): Y = A X without A.  The reference of every value test is the CPU oracle's matrix times
the same X, formed on the host in float64: R = A_o X and, row by row, S = |A_o| |X|.
  rows without a Dirichlet condition   |Y - R| <= tol max(S)   (the maximum over those rows), tol = 1e-12 for the linear forms
                                       (the project's matrix-parity tolerance), 1e-11 for Tangents (tests/test_gpu_patch.py)
  Dirichlet rows                       |Y_i - m_i X_i| <= 1e-12 |m_i X_i|, m_i the oracle's diagonal (the element count)
X is standard normal; the states are those of tests/test_gpu_state_pencil.py.  The shapes are the smallest that reach each branch
of the kernel: one wavefront per element (p = 3), two elements per wavefront with an odd element count (p = 2), mixed degrees,
reduced continuity, periodic axes, the three geometry kinds, second-order features, several fields."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_api as O
from common import make_pair, warped_geometry

pytestmark = pytest.mark.gpu

CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0)
NU, FX, DT = 1.472e-4, 3.37204e-3, 1e-2
NS = (NU, FX, -0.4 * FX, 0.25 * FX, DT)
EL = (1.5, 0.8)
KNOTS_C0 = [np.r_[[0] * 3, 0.2, 0.5, 0.7, [1] * 3], np.r_[[0] * 3, 0.3, 0.3, 0.6, 0.6, [1] * 3], np.r_[[0] * 3, 0.1, 0.3, 0.9, [1] * 3]]

# name -> (form, dof, p, N, make_pair keywords, geometry, Dirichlet values (axis, side, field, value), tolerance)
CASES = {
    "poisson-p3-dirichlet": ("poisson", 1, 3, (5, 4, 4), {}, None, [(d, s, 0, 0.5 + 0.25 * d + 0.125 * s) for d in range(3) for s in range(2)], 1e-12),
    "poisson-p2-odd": ("poisson", 1, 2, (5, 4, 3), {}, None, [], 1e-12),
    "poisson-mixed-degrees": ("poisson", 1, (2, 3, 2), (4, 3, 5), {"nqp": [3, 4, 4]}, None, [(1, 0, 0, 1.0)], 1e-12),
    "poisson-p2-c0-knots": ("poisson", 1, 2, (0, 0, 0), {"knots": KNOTS_C0}, None, [(2, 1, 0, -1.0)], 1e-12),
    "poisson-p2-periodic": ("poisson", 1, 2, (6, 4, 5), {"periodic": [True, False, True]}, None, [(1, 0, 0, 2.0)], 1e-12),
    "poisson-p3-poly": ("poisson", 1, 3, (4, 4, 3), {}, "poly", [(0, 0, 0, 1.0)], 1e-12),
    "poisson-p3-nurbs": ("poisson", 1, 3, (4, 4, 3), {}, "nurbs", [(0, 0, 0, 1.0)], 1e-12),
    "ch-p2-nurbs": ("cahnhilliard", 1, 2, (4, 4, 4), {}, "nurbs", [], 1e-11),
    "ch-p2": ("cahnhilliard", 1, 2, (5, 4, 3), {}, None, [], 1e-11),
    "ch-p2-dirichlet": ("cahnhilliard", 1, 2, (5, 4, 3), {}, None, [(0, 0, 0, 0.6), (0, 1, 0, 0.66), (1, 1, 0, 0.61), (2, 0, 0, 0.65)], 1e-11),
    "bratu-p3": ("bratu", 1, 3, (4, 4, 4), {}, None, [(d, s, 0, 0.1 * d * s) for d in range(3) for s in range(2)], 1e-11),
    "elasticity-p3": ("elasticity", 3, 3, (4, 3, 3), {}, None, [(0, 0, 0, 0.0), (0, 0, 1, 0.0), (0, 0, 2, 0.0), (2, 1, 0, 1.0)], 1e-12),
    "nsvms-p2": ("nsvms", 4, 2, (4, 4, 4), {}, None, [(1, s, f, 0.1 * f - 0.05 * s) for s in range(2) for f in range(3)], 1e-11),
    "nsvms-p2-nurbs": ("nsvms", 4, 2, (4, 4, 4), {}, "nurbs", [(1, s, f, 0.1 * f - 0.05 * s) for s in range(2) for f in range(3)], 1e-11),
}


def _pair(name):
    form, dof, p, N, kw, geo, bcs, tol = CASES[name]
    orc, eng = make_pair(3, dof, list(p) if isinstance(p, tuple) else p, list(N), **kw)
    if geo:
        Xg, Wg = warped_geometry(orc, 3, seed=11, rational=(geo == "nurbs"), amp=0.08)
        orc.set_geometry(Xg, Wg)
        eng.set_geometry(Xg, Wg)
    for g in (orc, eng):
        for bc in bcs:
            g.set_boundary_value(*bc)
    return orc, eng


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(X, U, V, R, S, Dirichlet rows, the oracle's diagonal) of a case: computed once, shared by the tests, never written to"""
    form = CASES[name][0]
    orc, _ = _pair(name)
    rng = np.random.default_rng(29)
    n = orc.global_size()
    X, V = rng.standard_normal(n), rng.standard_normal(n)
    U = None
    if form == "poisson":
        A_o = orc.compute_system("orc_form_poisson")[0]
    elif form == "elasticity":
        A_o = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))[0]
    elif form == "cahnhilliard":
        U = 0.63 + 0.05 * (2 * rng.random(n) - 1)
        A_o = orc.compute_ijacobian("orc_form_ch_tangent", O.CahnHilliardCtx(*CH), 250.0, V, 0.0, U)
    elif form == "bratu":
        U = 0.3 * rng.standard_normal(n)
        A_o = orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(3.5), U)
    else:
        U, V = 0.3 * rng.standard_normal(n), 0.1 * V
        A_o = orc.compute_ijacobian("orc_form_ns_tangent", O.NSVMSCtx(*NS), 2.0 / DT, V, 0.0, U)
    return (X, U, V) + _products(A_o.scipy(), X)


def _products(M, X):
    R, S = M @ X, abs(M) @ np.abs(X)
    diag = M.diagonal()
    off = abs(M)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0      # a fixed row holds only its diagonal
    for a in (R, S, diag, fixed):
        a.setflags(write=False)
    return R, S, fixed, diag


def _action(name, eng, X, U, V, Y=None):
    form = CASES[name][0]
    eng.set_form(form, {"poisson": (), "elasticity": EL, "cahnhilliard": CH, "bratu": (3.5,), "nsvms": NS}[form])
    Xv, Y = eng.create_vec().set(X), (Y if Y is not None else eng.create_vec())
    if form in ("poisson", "elasticity"):
        eng.compute_matrix_action(Xv, Y)
    elif form == "bratu":
        eng.compute_jacobian_action(eng.create_vec().set(U), Xv, Y)
    else:
        eng.compute_ijacobian_action(250.0 if form == "cahnhilliard" else 2.0 / DT, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), Xv, Y)
    eng.synchronize()
    assert "vec_sumfact" in eng.kernel_name() and "action" in eng.kernel_name(), eng.kernel_name()
    return Y


def _check(Y, X, R, S, fixed, diag, tol):
    free = ~fixed
    err, scale = np.abs(Y - R)[free].max(), S[free].max()
    print("free rows: max|Y - R| = %.3e, max S = %.3e, ratio %.3e (tol %g); Dirichlet rows: %d" % (err, scale, err / scale, tol, fixed.sum()))
    assert err <= tol * scale
    want = diag[fixed] * X[fixed]
    assert np.all(np.abs(Y[fixed] - want) <= 1e-12 * np.abs(want))


@pytest.mark.parametrize("name", sorted(CASES))
def test_action_equals_the_oracle_matrix_times_x(name):
    X, U, V, R, S, fixed, diag = _reference(name)
    _, eng = _pair(name)
    Y = _action(name, eng, X, U, V).get()
    assert ("two elements per wavefront" in eng.kernel_name()) == (CASES[name][2] == 2)
    assert fixed.any() == bool(CASES[name][6])
    _check(Y, X, R, S, fixed, diag, CASES[name][7])


@pytest.mark.parametrize("name", ["poisson-p3-dirichlet", "ch-p2", "poisson-p2-odd"])
def test_action_equals_the_engines_own_matrix_times_x(name):
    """the matrix the engine assembles for the same problem (System: with IGAElementFixSystem's matrix half; Matrix where no value
    is fixed; IJacobian), its coordinate list times X on the host: same bound.  Two calls return the same bits (the colours run in a
    fixed order), and so does a call into a NaN-poisoned Y (the driver zeroes it)."""
    import scipy.sparse as sp
    X, U, V = _reference(name)[:3]
    _, eng = _pair(name)
    Y = _action(name, eng, X, U, V)
    Y1 = Y.get().copy()
    assert np.array_equal(_action(name, eng, X, U, V).get(), Y1)
    Y.set(np.full(Y1.size, np.nan))
    assert np.array_equal(_action(name, eng, X, U, V, Y).get(), Y1)
    A = eng.create_mat()
    if name == "poisson-p3-dirichlet":
        eng.compute_system(A, eng.create_vec())
    elif name == "poisson-p2-odd":
        eng.compute_matrix(A)
    else:
        eng.compute_ijacobian(250.0, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), A)
    eng.synchronize()
    rows, cols, vals = A.to_coo_global()
    M = sp.coo_matrix((vals, (rows, cols)), shape=(X.size, X.size)).tocsr()
    _check(Y1, X, *_products(M, X), CASES[name][7])


def test_refusals_name_their_reason(monkeypatch):
    import petiga_amd as P
    X, U, V = _reference("poisson-p2-odd")[:3]

    def refused(eng, word, code=56):
        eng.set_form("poisson")
        Y = eng.create_vec()
        Xv = eng.create_vec().set(np.ones(Y.n))
        with pytest.raises(P.IGXError) as e:
            eng.compute_matrix_action(Xv, Y)
        assert e.value.code == code and word in str(e.value), str(e.value)

    _, eng = _pair("poisson-p2-odd")
    eng.set_boundary_form(0, 1, True)
    refused(eng, "boundary-form")
    eng.set_boundary_form(0, 1, False)
    eng.set_kernel(1)
    refused(eng, "IGXSetKernel")
    eng.set_kernel(0)
    _action("poisson-p2-odd", eng, X, U, V)      # a refused call leaves nothing behind: the covered call reports its own kernel
    Xv = eng.create_vec().set(X)
    with pytest.raises(P.IGXError) as e:
        eng.compute_matrix_action(Xv, Xv)
    assert e.value.code == 62
    other = _pair("poisson-p2-odd")[1]
    with pytest.raises(P.IGXError) as e:
        eng.compute_matrix_action(Xv, other.create_vec())
    assert e.value.code == 62
    g2 = P.IGX(2, 1)
    for i in range(2):
        g2.axis_uniform(i, 2, 4)
    g2.setup()
    refused(g2, "dim")
    monkeypatch.setenv("IGX_VEC_SUMFACT", "0")      # (read when the IGX is created)
    _, off = _pair("poisson-p2-odd")
    refused(off, "IGX_VEC_SUMFACT")


# the x-dependent anisotropic diffusion struct of tests/test_rtc_forms.py: D(x) = diag(1 + x0, 2, 1 + x1 x2) + off-diagonal 0.3 x0 on (0,1)
USER_DIFFUSION = r"""
struct UserDiffusion {
  static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = NEED_X;
  static constexpr unsigned MAT_TEST_MASK = 0xEu, VEC_TEST_MASK = 0x1u;
  static constexpr bool MAT_SYMMETRIC = true;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    const double d00 = 1.0 + p.x[0], d11 = 2.0, d22 = 1.0 + p.x[1] * p.x[2], d01 = 0.3 * p.x[0];
    T[0] = d00 * Na[1] * Nb[1] + d11 * Na[2] * Nb[2] + d22 * Na[3] * Nb[3] + d01 * (Na[1] * Nb[2] + Na[2] * Nb[1]);
  }
  static __device__ void vec(const PtView &p, const double *Na, double *R) { R[0] = Na[0] * p.prm[0] * (1.0 + p.x[0] - p.x[2]); }
};
"""


class _OrcPoint(C.Structure):      # struct OrcPoint, oracle/igaoracle.h
    _dp = C.POINTER(C.c_double)
    _fields_ = [("iga", C.c_void_p), ("atboundary", C.c_int), ("boundary_id", C.c_int), ("count", C.c_int), ("index", C.c_int),
                ("neq", C.c_int), ("nen", C.c_int), ("dof", C.c_int), ("dim", C.c_int), ("nsd", C.c_int),
                ("rational", _dp), ("geometry", _dp), ("weight", _dp), ("detJac", _dp), ("point", _dp), ("normal", _dp),
                ("basis", _dp * 5), ("shape", _dp * 5), ("mapU", _dp * 5), ("mapX", _dp * 5), ("detX", _dp), ("detS", _dp),
                ("ID", C.c_int * 3), ("property", _dp), ("npd", C.c_int)]


def _oracle_user_diffusion(orc):
    """the oracle's System matrix of the struct above: its assembly loop with the form restated as a point callback (IGAFormSystem)"""
    geommap = C.CFUNCTYPE(None, C.POINTER(_OrcPoint), C.POINTER(C.c_double))(("orc_point_geommap", O.lib()))

    @C.CFUNCTYPE(C.c_int, C.POINTER(_OrcPoint), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
    def form(p, K, F, ctx):
        q = p.contents
        nen = q.nen
        x = (C.c_double * 3)()
        geommap(p, x)
        N1 = np.ctypeslib.as_array(q.shape[1], shape=(nen, 3))
        D = np.array([[1.0 + x[0], 0.3 * x[0], 0.0], [0.3 * x[0], 2.0, 0.0], [0.0, 0.0, 1.0 + x[1] * x[2]]])
        np.ctypeslib.as_array(K, shape=(nen, nen))[:] = N1 @ D @ N1.T
        np.ctypeslib.as_array(F, shape=(nen,))[:] = 0.0
        return 0

    A = orc.create_mat()
    B = np.zeros(orc.global_size())
    orc._ck(orc.L.orc_compute_system(orc.p, C.cast(form, C.c_void_p), None, A.ptr, B.ctypes.data_as(C.POINTER(C.c_double))))
    return A


@pytest.mark.parametrize("geo", [None, "poly"])
def test_run_time_form(geo):
    orc, eng = make_pair(3, 1, 2, [4, 4, 3])
    if geo:
        Xg, Wg = warped_geometry(orc, 3, seed=9, rational=False, amp=0.08)
        orc.set_geometry(Xg, Wg)
        eng.set_geometry(Xg, Wg)
    for g in (orc, eng):
        g.set_boundary_value(0, 0, 0, 2.0)
        g.set_boundary_value(2, 1, 0, -1.0)
    X = np.random.default_rng(31).standard_normal(orc.global_size())
    eng.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
    Y = eng.create_vec()
    eng.compute_matrix_action(eng.create_vec().set(X), Y)
    eng.synchronize()
    assert "hiprtc" in eng.kernel_name() and "action" in eng.kernel_name(), eng.kernel_name()
    _check(Y.get(), X, *_products(_oracle_user_diffusion(orc).scipy(), X), 1e-12)
