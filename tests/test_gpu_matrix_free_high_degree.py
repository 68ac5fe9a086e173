"""GPU parity of the matrix-free actions and diagonals above four basis functions or points per axis (petiga_amd/csrc/vec_sumfact.hpp:
one workgroup per element, 6 x 6 x 6 lanes up to nen, nqp = 6 and 8 x 8 x 8 lanes up to 8).  References and bounds are those of
tests/test_gpu_matrix_action.py and tests/test_gpu_matrix_diagonal.py: the CPU oracle's matrix times a standard-normal X,
  rows without a Dirichlet condition   |Y - R| <= tol max(S), S = |A_o| |X|
  Dirichlet rows                       |Y_i - m_i X_i| <= 1e-12 |m_i X_i|
  the diagonal                         free dofs |D - R| <= tol max|R| per field, fixed dofs exactly
with tol = 1e-12 for the linear forms on the identity geometry, 2e-11 on warped poly / NURBS maps (the geometry tolerance of
tests/test_gpu_high_degree.py), 1e-11 for Tangents.  The shapes are the smallest that reach each branch: both layouts, padded lanes on
some axes only (mixed degrees), more points than nodes and more nodes than points, one element, reduced continuity, a periodic axis,
the three geometry kinds, second-order features, several fields, a run-time struct."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_api as O
from common import make_pair, warped_geometry
from test_gpu_matrix_action import CH, DT, EL, NS, USER_DIFFUSION, _check, _oracle_user_diffusion, _products
from test_gpu_matrix_diagonal import _check as _check_diagonal

pytestmark = pytest.mark.gpu

ALL6 = [(d, s, 0, 0.5 + 0.25 * d + 0.125 * s) for d in range(3) for s in range(2)]
EL_BCS = [(0, 0, 0, 0.0), (0, 0, 1, 0.0), (0, 0, 2, 0.0), (2, 1, 0, 1.0)]
NS_BCS = [(1, s, f, 0.1 * f - 0.05 * s) for s in range(2) for f in range(3)]
BR_BCS = [(d, s, 0, 0.1 * d * s) for d in range(3) for s in range(2)]
PARAMS = {"poisson": (), "elasticity": EL, "cahnhilliard": CH, "bratu": (3.5,), "bratu-i": (3.5,), "nsvms": NS}

# name -> (form, dof, p, N, make_pair keywords, geometry, Dirichlet values (axis, side, field, value), tolerance, lanes per axis)
CASES = {
    "poisson-p4-dirichlet": ("poisson", 1, 4, (3, 2, 2), {}, None, ALL6, 1e-12, 6),
    "poisson-p5": ("poisson", 1, 5, (2, 2, 3), {}, None, [(0, 1, 0, 1.0)], 1e-12, 6),
    "poisson-p5-one-element": ("poisson", 1, 5, (1, 1, 1), {}, None, [(2, 0, 0, -1.0)], 1e-12, 6),
    "poisson-p453-nqp564": ("poisson", 1, (4, 5, 3), (3, 2, 2), {"nqp": [5, 6, 4]}, None, [(1, 0, 0, 1.0)], 1e-12, 6),
    "poisson-p3-nqp5": ("poisson", 1, 3, (4, 3, 3), {"nqp": [5, 5, 5]}, None, [(0, 0, 0, 2.0)], 1e-12, 6),
    "poisson-p5-nqp4": ("poisson", 1, 5, (2, 2, 2), {"nqp": [4, 4, 4]}, None, [(2, 1, 0, -1.0)], 1e-12, 6),
    "poisson-p4-c123": ("poisson", 1, 4, (3, 3, 2), {"C": [1, 2, 3]}, None, [(1, 1, 0, 0.5)], 1e-12, 6),
    "poisson-p4-periodic": ("poisson", 1, 4, (9, 2, 2), {"periodic": [True, False, False]}, None, [(1, 0, 0, 2.0)], 1e-12, 6),
    "poisson-p6": ("poisson", 1, 6, (2, 2, 1), {}, None, [(0, 0, 0, 1.0)], 1e-12, 8),
    "poisson-p7": ("poisson", 1, 7, (2, 1, 2), {}, None, [(2, 1, 0, 0.25)], 1e-12, 8),
    "poisson-p546-nqp658": ("poisson", 1, (5, 4, 6), (2, 3, 2), {"nqp": [6, 5, 8]}, None, [(1, 1, 0, 1.0)], 1e-12, 8),
    "poisson-p712": ("poisson", 1, (7, 1, 2), (1, 3, 2), {}, None, [(0, 0, 0, 1.0)], 1e-12, 8),
    "poisson-p4-poly": ("poisson", 1, 4, (2, 3, 2), {}, "poly", [(0, 0, 0, 1.0)], 2e-11, 6),
    "poisson-p5-nurbs": ("poisson", 1, 5, (2, 2, 2), {}, "nurbs", [(0, 0, 0, 1.0)], 2e-11, 6),
    "poisson-p6-nurbs": ("poisson", 1, 6, (2, 1, 2), {}, "nurbs", [(0, 0, 0, 1.0)], 2e-11, 8),
    "elasticity-p4": ("elasticity", 3, 4, (2, 2, 2), {}, None, EL_BCS, 1e-12, 6),
    "bratu-p4": ("bratu", 1, 4, (2, 3, 2), {}, None, BR_BCS, 1e-11, 6),
    "bratu-p6": ("bratu", 1, 6, (2, 1, 2), {}, None, BR_BCS, 1e-11, 8),
    "bratu-i-p4": ("bratu-i", 1, 4, (2, 3, 2), {}, None, BR_BCS, 1e-11, 6),
    "bratu-i-p6": ("bratu-i", 1, 6, (2, 1, 2), {}, None, BR_BCS, 1e-11, 8),
    "ch-p4": ("cahnhilliard", 1, 4, (3, 2, 2), {}, None, [], 1e-11, 6),
    "ch-p4-nurbs": ("cahnhilliard", 1, 4, (3, 2, 2), {}, "nurbs", [], 1e-11, 6),
    "nsvms-p4": ("nsvms", 4, 4, (2, 2, 2), {}, None, NS_BCS, 1e-11, 6),
    "nsvms-p4-nurbs": ("nsvms", 4, 4, (2, 2, 2), {}, "nurbs", NS_BCS, 1e-11, 6),
}
WITH_DIAGONAL = sorted(n for n in CASES if not n.startswith("ch-"))
I_SHIFT = {"cahnhilliard": 250.0, "bratu-i": 4.0, "nsvms": 2.0 / DT}


def _pair(name):
    form, dof, p, N, kw, geo, bcs = CASES[name][:7]
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
        A_o = orc.compute_ijacobian("orc_form_ch_tangent", O.CahnHilliardCtx(*CH), I_SHIFT[form], V, 0.0, U)
    elif form == "bratu":
        U = 0.3 * rng.standard_normal(n)
        A_o = orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(3.5), U)
    elif form == "bratu-i":
        U = 0.3 * rng.standard_normal(n)
        A_o = orc.compute_ijacobian("orc_form_bratu_ijacobian", C.c_double(3.5), I_SHIFT[form], V, 0.0, U)
    else:
        U, V = 0.3 * rng.standard_normal(n), 0.1 * V
        A_o = orc.compute_ijacobian("orc_form_ns_tangent", O.NSVMSCtx(*NS), I_SHIFT[form], V, 0.0, U)
    for a in (X, U, V):
        if a is not None:
            a.setflags(write=False)
    return (X, U, V) + _products(A_o.scipy(), X)


def _kernel(eng, what, lanes):
    kn = eng.kernel_name()
    assert "vec_sumfact" in kn and what in kn and "one workgroup per element" in kn and "%d x %d x %d lanes" % (lanes, lanes, lanes) in kn, kn
    return kn


def _set_form(name, eng):
    form = CASES[name][0]
    eng.set_form("bratu" if form == "bratu-i" else form, PARAMS[form])
    return form


def _action(name, eng, X, U, V, Y=None):
    form = _set_form(name, eng)
    Xv, Y = eng.create_vec().set(X), (Y if Y is not None else eng.create_vec())
    if form in ("poisson", "elasticity"):
        eng.compute_matrix_action(Xv, Y)
    elif form == "bratu":
        eng.compute_jacobian_action(eng.create_vec().set(U), Xv, Y)
    else:
        eng.compute_ijacobian_action(I_SHIFT[form], eng.create_vec().set(V), 0.0, eng.create_vec().set(U), Xv, Y)
    eng.synchronize()
    _kernel(eng, "matrix action", CASES[name][8])
    return Y


def _diagonal(name, eng, U, V, D=None):
    form = _set_form(name, eng)
    D = D if D is not None else eng.create_vec()
    if form in ("poisson", "elasticity"):
        eng.compute_matrix_diagonal(D)
    elif form == "bratu":
        eng.compute_jacobian_diagonal(eng.create_vec().set(U), D)
    else:
        eng.compute_ijacobian_diagonal(I_SHIFT[form], eng.create_vec().set(V), 0.0, eng.create_vec().set(U), D)
    eng.synchronize()
    _kernel(eng, "matrix diagonal", CASES[name][8])
    return D


@pytest.mark.parametrize("name", sorted(CASES))
def test_action_equals_the_oracle_matrix_times_x(name):
    X, U, V, R, S, fixed, diag = _reference(name)
    _, eng = _pair(name)
    Y = _action(name, eng, X, U, V).get()
    assert fixed.any() == bool(CASES[name][6])
    _check(Y, X, R, S, fixed, diag, CASES[name][7])


@pytest.mark.parametrize("name", WITH_DIAGONAL)
def test_diagonal_equals_the_oracle_matrix_diagonal(name):
    _, U, V, _, _, fixed, diag = _reference(name)
    _, eng = _pair(name)
    D = _diagonal(name, eng, U, V).get()
    assert fixed.any()
    _check_diagonal(D, diag, fixed, CASES[name][1], CASES[name][7], name)


@pytest.mark.parametrize("name", ["ch-p4", "ch-p4-nurbs"])
def test_diagonal_of_second_order_features_stays_refused(name):
    import petiga_amd as P
    _, eng = _pair(name)
    eng.set_form("cahnhilliard", CH)
    Uv, Vv, D = eng.create_vec(), eng.create_vec(), eng.create_vec()
    with pytest.raises(P.IGXError) as e:
        eng.compute_ijacobian_diagonal(250.0, Vv, 0.0, Uv, D)
    assert e.value.code == 56 and "second-order" in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["poisson-p4-dirichlet", "poisson-p546-nqp658", "nsvms-p4"])
def test_bit_repeatable(name):
    """two calls return the same bits (the colours run in a fixed order), and so does a call into a NaN-poisoned output (the driver
    zeroes it): the action and the diagonal, both layouts"""
    X, U, V = _reference(name)[:3]
    _, eng = _pair(name)
    for run, args in ((_action, (X, U, V)), (_diagonal, (U, V))):
        Y = run(name, eng, *args)
        Y1 = Y.get().copy()
        assert np.all(np.isfinite(Y1))
        assert np.array_equal(run(name, eng, *args).get(), Y1)
        Y.set(np.full(Y1.size, np.nan))
        assert np.array_equal(run(name, eng, *args, Y).get(), Y1)


def _sample_rows(orc, fixed, dof, rng):
    """two corner nodes, a node on an edge, nodes on faces, Dirichlet rows and random free rows (no periodic axis)"""
    n0, n1, n2 = (len(orc.axis(i)["U"]) - orc.axis(i)["p"] - 1 for i in range(3))
    assert n0 * n1 * n2 * dof == fixed.size
    node = lambda a, b, c: a + n0 * (b + n1 * c)
    rows = set()
    for nd in (node(0, 0, 0), node(n0 - 1, n1 - 1, n2 - 1), node(n0 // 2, 0, 0), node(0, n1 - 1, n2 // 2), node(n0 // 2, n1 // 2, 0)):
        rows.update(nd * dof + f for f in range(dof))
    fx, fr = np.flatnonzero(fixed), np.flatnonzero(~fixed)
    rows.update(int(r) for r in rng.choice(fx, size=min(3, fx.size), replace=False))
    rows.update(int(r) for r in rng.choice(fr, size=min(4, fr.size), replace=False))
    return sorted(rows)


@pytest.mark.parametrize("name", ["poisson-p4-dirichlet", "poisson-p6-nurbs", "elasticity-p4"])
def test_diagonal_is_consistent_with_the_action_on_unit_vectors(name):
    """Y = A e_r from the action at corner, edge, face, Dirichlet and random free rows r: Y_r and D_r within the diagonal's bound
    (a Dirichlet row: both the element count, exactly)"""
    _, U, V, _, _, fixed, diag = _reference(name)
    dof, tol = CASES[name][1], CASES[name][7]
    orc, eng = _pair(name)
    D = _diagonal(name, eng, U, V).get().copy()
    rows = _sample_rows(orc, fixed, dof, np.random.default_rng(41))
    assert fixed[rows].any() and (~fixed[rows]).any()
    for r in rows:
        e = np.zeros(D.size)
        e[r] = 1.0
        Y = _action(name, eng, e, U, V).get()
        f = r % dof
        scale = np.abs(diag[f::dof])[~fixed[f::dof]].max()
        print("%s dof %d (%s): Y_r = %.17g, D_r = %.17g, |Y_r - D_r| / max|R| = %.3e" % (name, r, "fixed" if fixed[r] else "free", Y[r], D[r], abs(Y[r] - D[r]) / scale))
        if fixed[r]:
            assert Y[r] == D[r] == diag[r]
        else:
            assert abs(Y[r] - D[r]) <= tol * scale


def test_engines_own_matrix():
    """Poisson p = 4: the matrix the engine assembles for the same problem (System, with IGAElementFixSystem's matrix half), its
    coordinate list times X and its diagonal: the same bounds"""
    import scipy.sparse as sp
    name = "poisson-p4-dirichlet"
    X, U, V, _, _, fixed, _ = _reference(name)
    _, eng = _pair(name)
    Y = _action(name, eng, X, U, V).get().copy()
    D = _diagonal(name, eng, U, V).get().copy()
    A = eng.create_mat()
    eng.compute_system(A, eng.create_vec())
    eng.synchronize()
    rows, cols, vals = A.to_coo_global()
    M = sp.coo_matrix((vals, (rows, cols)), shape=(X.size, X.size)).tocsr()
    _check(Y, X, *_products(M, X), CASES[name][7])
    _check_diagonal(D, M.diagonal(), fixed, 1, CASES[name][7], name + " (engine)")


@pytest.mark.parametrize("what", ["action", "diagonal"])
def test_run_time_form_on_nurbs(what):
    orc, eng = make_pair(3, 1, 4, [2, 2, 2])
    Xg, Wg = warped_geometry(orc, 3, seed=9, rational=True, amp=0.08)
    orc.set_geometry(Xg, Wg)
    eng.set_geometry(Xg, Wg)
    for g in (orc, eng):
        g.set_boundary_value(0, 0, 0, 2.0)
        g.set_boundary_value(2, 1, 0, -1.0)
    eng.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
    M = _oracle_user_diffusion(orc).scipy()
    if what == "action":
        X = np.random.default_rng(31).standard_normal(orc.global_size())
        Y = eng.create_vec()
        eng.compute_matrix_action(eng.create_vec().set(X), Y)
        eng.synchronize()
        assert "hiprtc" in _kernel(eng, "matrix action", 6)
        _check(Y.get(), X, *_products(M, X), 2e-11)
    else:
        D = eng.create_vec()
        eng.compute_matrix_diagonal(D)
        eng.synchronize()
        assert "hiprtc" in _kernel(eng, "matrix diagonal", 6)
        fixed = _products(M, np.ones(M.shape[0]))[2]
        assert fixed.any()
        _check_diagonal(D.get(), M.diagonal(), fixed, 1, 2e-11, "UserDiffusion nurbs")


def test_more_than_eight_per_axis_is_still_refused():
    """nine points per axis answer 56 with both limits named, for both driver groups.  Degree 8 (nen = 9) answers 56 as well, but from
    IGXAxisSetDegree ("degree > 7 not supported": the library as a whole stops at degree 7), before any driver is reached."""
    import petiga_amd as P
    _, eng = make_pair(3, 1, 3, [2, 2, 2], nqp=9)
    eng.set_form("poisson")
    Xv, Y = eng.create_vec(), eng.create_vec()
    Xv.set(np.ones(Y.n))
    for call, word in ((lambda: eng.compute_matrix_action(Xv, Y), "action"), (lambda: eng.compute_matrix_diagonal(Y), "diagonal")):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == 56 and "nen <= 8" in str(e.value) and "nqp <= 8" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(P.IGXError) as e:
        g8 = P.IGX(3, 1)
        for i in range(3):
            g8.axis_uniform(i, 8, 1)
        g8.setup()
        g8.set_form("poisson")
        g8.compute_matrix_diagonal(g8.create_vec())
    assert e.value.code == 56 and ("nen <= 8" in str(e.value) or "degree > 7" in str(e.value)), str(e.value)


def test_jacobi_preconditioned_cg_on_the_action():
    """End to end, as tests/test_gpu_matrix_diagonal.py's: Poisson p = 5 on (3, 3, 3) elements with Dirichlet values on all six faces;
    CG on the host with the GPU's IGXComputeMatrixAction as the operator, 1 / D of IGXComputeMatrixDiagonal as the preconditioner and
    IGXComputeSystem's right-hand side.  It reaches a relative residual of 1e-10 in both norms, |r| <= 1e-10 |b| and the preconditioned
    |r / D| <= 1e-10 |b / D|, in no more iterations than there are unknowns, and the solution agrees with a sparse direct solve of the
    oracle's system to 1e-8."""
    import scipy.sparse.linalg as spla
    orc, eng = make_pair(3, 1, 5, [3, 3, 3])
    for g in (orc, eng):
        for bc in ALL6:
            g.set_boundary_value(*bc)
    eng.set_form("poisson")
    A, b = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, b)
    eng.synchronize()
    rhs = b.get().copy()
    n = rhs.size
    Dv = eng.create_vec()
    eng.compute_matrix_diagonal(Dv)
    eng.synchronize()
    _kernel(eng, "matrix diagonal", 6)
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
    _kernel(eng, "matrix action", 6)
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
