"""GPU parity of the matrix-free diagonals (include/petiga_amd.h: IGXComputeMatrixDiagonal / JacobianDiagonal / IJacobianDiagonal;
petiga_amd/csrc/vec_sumfact.hpp, DIAGONAL): D = diag A without A.  The reference is the diagonal R of the CPU oracle's matrix, the
cases, states and tolerances are those of tests/test_gpu_matrix_action.py (all but Cahn-Hilliard, whose second-order shape features
the diagonal refuses):
  free dofs    |D - R| <= tol max|R|, the maximum over the free dofs of the same field; tol = 1e-12 for the linear forms, 1e-11 for
               the Tangents
  fixed dofs   D == R exactly: the number of elements at the node, a small integer
Further: the engine's own assembled matrix, the action on a unit vector, repeatability, a run-time struct, the refusals, and a
Jacobi-preconditioned CG run with the action as the operator."""
import numpy as np
import pytest

from common import make_pair, warped_geometry
from test_gpu_matrix_action import CASES, DT, EL, NS, USER_DIFFUSION, _action, _oracle_user_diffusion, _pair, _reference

pytestmark = pytest.mark.gpu

COVERED = sorted(n for n in CASES if not n.startswith("ch-"))
PARAMS = {"poisson": (), "elasticity": EL, "bratu": (3.5,), "nsvms": NS}


def _diagonal(name, eng, U, V, D=None):
    form = CASES[name][0]
    eng.set_form(form, PARAMS[form])
    D = D if D is not None else eng.create_vec()
    if form in ("poisson", "elasticity"):
        eng.compute_matrix_diagonal(D)
    elif form == "bratu":
        eng.compute_jacobian_diagonal(eng.create_vec().set(U), D)
    else:
        eng.compute_ijacobian_diagonal(2.0 / DT, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), D)
    eng.synchronize()
    kn = eng.kernel_name()
    assert "vec_sumfact" in kn and "matrix diagonal" in kn, kn
    assert ("two elements per wavefront" in kn) == (CASES[name][2] == 2), kn
    assert ("one wavefront per element" in kn) == (CASES[name][2] != 2), kn
    return D


def _check(D, R, fixed, dof, tol, what=""):
    """free dofs field by field, fixed dofs exactly; returns the worst ratio |D - R| / max|R|"""
    worst = 0.0
    for f in range(dof):
        free = ~fixed[f::dof]
        err, scale = np.abs(D[f::dof] - R[f::dof])[free].max(), np.abs(R[f::dof])[free].max()
        print("%s field %d: max|D - R| = %.3e, max|R| = %.3e, ratio %.3e (tol %g)" % (what, f, err, scale, err / scale, tol))
        assert err <= tol * scale
        worst = max(worst, err / scale)
    assert np.array_equal(D[fixed], R[fixed])
    assert np.all(R[fixed] == np.round(R[fixed])) and np.all(R[fixed] >= 1)
    return worst


@pytest.mark.parametrize("name", COVERED)
def test_diagonal_equals_the_oracle_matrix_diagonal(name):
    _, U, V, _, _, fixed, diag = _reference(name)
    dof = CASES[name][1]
    _, eng = _pair(name)
    D = _diagonal(name, eng, U, V).get()
    assert fixed.any() == bool(CASES[name][6])
    _check(D, diag, fixed, dof, CASES[name][7], name)
    if name in ("elasticity-p3", "nsvms-p2"):      # a node with fixed and free fields: the free ones keep their own K_aa^ii
        fx = fixed.reshape(-1, dof)
        mixed = fx.any(axis=1) & ~fx.all(axis=1)
        assert mixed.any()
        for f in range(dof):
            rows = np.flatnonzero(mixed & ~fx[:, f]) * dof + f
            if rows.size == 0:
                continue
            scale = np.abs(diag[f::dof])[~fx[:, f]].max()
            assert np.abs(D[rows] - diag[rows]).max() <= CASES[name][7] * scale


@pytest.mark.parametrize("name", ["poisson-p3-dirichlet", "poisson-p2-odd", "nsvms-p2"])
def test_diagonal_equals_the_engines_own_matrix_diagonal(name):
    """the matrix the engine assembles for the same problem (System: with IGAElementFixSystem's matrix half; Matrix where no value is
    fixed; IJacobian), the diagonal of its coordinate list: same bound"""
    import scipy.sparse as sp
    _, U, V, _, _, fixed, _ = _reference(name)
    _, eng = _pair(name)
    D = _diagonal(name, eng, U, V).get().copy()
    A = eng.create_mat()
    if name == "poisson-p3-dirichlet":
        eng.compute_system(A, eng.create_vec())
    elif name == "poisson-p2-odd":
        eng.compute_matrix(A)
    else:
        eng.compute_ijacobian(2.0 / DT, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), A)
    eng.synchronize()
    rows, cols, vals = A.to_coo_global()
    M = sp.coo_matrix((vals, (rows, cols)), shape=(D.size, D.size)).tocsr()
    _check(D, M.diagonal(), fixed, CASES[name][1], CASES[name][7], name + " (engine)")


@pytest.mark.parametrize("name", ["elasticity-p3", "poisson-p3-nurbs"])
def test_diagonal_is_consistent_with_the_action_on_a_unit_vector(name):
    """at a random free dof r of every field, Y = A e_r from the action: Y_r and D_r within the bound above"""
    _, U, V, _, _, fixed, diag = _reference(name)
    dof = CASES[name][1]
    _, eng = _pair(name)
    D = _diagonal(name, eng, U, V).get().copy()
    rng = np.random.default_rng(41)
    for f in range(dof):
        free = np.flatnonzero(~fixed[f::dof]) * dof + f
        r = int(rng.choice(free))
        e = np.zeros(D.size)
        e[r] = 1.0
        Y = _action(name, eng, e, U, V).get()
        scale = np.abs(diag[free]).max()
        print("%s field %d dof %d: Y_r = %.17g, D_r = %.17g, |Y_r - D_r| / max|R| = %.3e" % (name, f, r, Y[r], D[r], abs(Y[r] - D[r]) / scale))
        assert abs(Y[r] - D[r]) <= CASES[name][7] * scale


@pytest.mark.parametrize("name", ["poisson-p3-dirichlet", "nsvms-p2"])
def test_diagonal_is_bit_repeatable(name):
    """two calls return the same bits (the colours run in a fixed order), and so does a call into a NaN-poisoned D (the driver zeroes it)"""
    _, U, V = _reference(name)[:3]
    _, eng = _pair(name)
    D = _diagonal(name, eng, U, V)
    D1 = D.get().copy()
    assert np.all(np.isfinite(D1))
    assert np.array_equal(_diagonal(name, eng, U, V).get(), D1)
    D.set(np.full(D1.size, np.nan))
    assert np.array_equal(_diagonal(name, eng, U, V, D).get(), D1)


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
    eng.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
    D = eng.create_vec()
    eng.compute_matrix_diagonal(D)
    eng.synchronize()
    kn = eng.kernel_name()
    assert "hiprtc" in kn and "matrix diagonal" in kn and "two elements per wavefront" in kn, kn
    M = _oracle_user_diffusion(orc).scipy()
    off = abs(M)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    assert fixed.any()
    _check(D.get(), M.diagonal(), fixed, 1, 1e-12, "UserDiffusion %s" % geo)


def test_refusals_name_their_reason(monkeypatch):
    import petiga_amd as P
    n = _reference("poisson-p2-odd")[0].size
    U, V = 0.3 * np.random.default_rng(3).standard_normal(n), None      # (a state for the Jacobian driver's argument checks)

    def refused(eng, word, code=56, form="poisson", params=()):
        eng.set_form(form, params)
        D = eng.create_vec()
        with pytest.raises(P.IGXError) as e:
            eng.compute_matrix_diagonal(D)
        assert e.value.code == code and word in str(e.value) and "diagonal" in str(e.value), str(e.value)

    _, ch = _pair("ch-p2")
    ch.set_form("cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0))
    Uv, Vv, D = ch.create_vec(), ch.create_vec(), ch.create_vec()
    with pytest.raises(P.IGXError) as e:
        ch.compute_ijacobian_diagonal(250.0, Vv, 0.0, Uv, D)
    assert e.value.code == 56 and "second-order" in str(e.value), str(e.value)

    _, eng = _pair("poisson-p2-odd")
    eng.set_boundary_form(0, 1, True)
    refused(eng, "boundary-form")
    eng.set_boundary_form(0, 1, False)
    eng.set_kernel(1)
    refused(eng, "IGXSetKernel")
    eng.set_kernel(0)
    _diagonal("poisson-p2-odd", eng, U, V)      # a refused call leaves nothing behind: the covered call reports its own kernel
    eng.set_form("bratu", (3.5,))
    Uv = eng.create_vec().set(U)
    with pytest.raises(P.IGXError) as e:
        eng.compute_jacobian_diagonal(Uv, Uv)     # D aliasing U
    assert e.value.code == 62
    other = _pair("poisson-p2-odd")[1]
    with pytest.raises(P.IGXError) as e:
        eng.compute_jacobian_diagonal(Uv, other.create_vec())
    assert e.value.code == 62
    with pytest.raises(P.IGXError) as e:
        eng.compute_jacobian_diagonal(other.create_vec(), eng.create_vec())
    assert e.value.code == 62
    _diagonal("poisson-p2-odd", eng, U, V)
    g2 = P.IGX(2, 1)
    for i in range(2):
        g2.axis_uniform(i, 2, 4)
    g2.setup()
    refused(g2, "dim")
    monkeypatch.setenv("IGX_VEC_SUMFACT", "0")      # (read when the IGX is created)
    _, off = _pair("poisson-p2-odd")
    refused(off, "IGX_VEC_SUMFACT")


def test_jacobi_preconditioned_cg_on_the_action():
    """End to end: Poisson p = 2 on (5, 4, 3) elements with Dirichlet values on all six faces; CG on the host with the GPU's
    IGXComputeMatrixAction as the operator, 1 / D of IGXComputeMatrixDiagonal as the preconditioner and IGXComputeSystem's right-hand
    side.  It reaches a relative residual of 1e-10 in no more iterations than there are unknowns, and the solution agrees with a
    sparse direct solve of the oracle's system to 1e-8.  The residual is held to 1e-10 in BOTH norms, |r| <= 1e-10 |b| and the
    preconditioned |r / D| <= 1e-10 |b / D|: 150 of the 210 rows are Dirichlet rows whose right-hand side is the element count times
    the value, so |b| = 58.9 is carried by them and the plain norm alone stops while the 60 interior rows (b ~ 1e-2) are still
    1e-8 off -- the same CG on the oracle's own matrix stops after 24 iterations with an error of 1.36e-8 then, after 27 with
    5.4e-10 under both.  Seen on an MI355X: 27 iterations for 210 unknowns (max|x - spsolve| = 5.4e-10)."""
    import scipy.sparse.linalg as spla
    orc, eng = make_pair(3, 1, 2, [5, 4, 3])
    for g in (orc, eng):
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 0.5 + 0.25 * d + 0.125 * s)
    eng.set_form("poisson")
    A, b = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, b)
    eng.synchronize()
    rhs = b.get().copy()
    n = rhs.size
    Dv = eng.create_vec()
    eng.compute_matrix_diagonal(Dv)
    eng.synchronize()
    assert "matrix diagonal" in eng.kernel_name()
    D = Dv.get().copy()
    assert np.all(D > 0)
    Xv, Yv = eng.create_vec(), eng.create_vec()

    def op(x):
        Xv.set(x)
        eng.compute_matrix_action(Xv, Yv)
        eng.synchronize()
        return Yv.get().copy()

    x = np.zeros(n)
    r = rhs - op(x)
    z = r / D
    p = z.copy()
    rz, norm0, normz0, its = r @ z, np.linalg.norm(rhs), np.linalg.norm(rhs / D), 0
    while (np.linalg.norm(r) > 1e-10 * norm0 or np.linalg.norm(z) > 1e-10 * normz0) and its < n:
        Ap = op(p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = r / D
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        its += 1
    print("Jacobi-preconditioned CG: %d iterations for %d unknowns, relative residual %.3e, preconditioned %.3e"
          % (its, n, np.linalg.norm(r) / norm0, np.linalg.norm(z) / normz0))
    assert np.linalg.norm(r) <= 1e-10 * norm0 and np.linalg.norm(z) <= 1e-10 * normz0 and its <= n
    A_o, b_o = orc.compute_system("orc_form_poisson")
    want = spla.spsolve(A_o.scipy().tocsc(), np.asarray(b_o))
    print("max|x - spsolve| = %.3e, max|spsolve| = %.3f" % (np.abs(x - want).max(), np.abs(want).max()))
    assert np.abs(x - want).max() <= 1e-8 * np.abs(want).max()
