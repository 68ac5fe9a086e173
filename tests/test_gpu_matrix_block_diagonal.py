"""GPU parity of the matrix-free point-block diagonals (include/petiga_amd.h: IGXComputeMatrixBlockDiagonal / JacobianBlockDiagonal /
IJacobianBlockDiagonal, IGXBlockDiagonalInvert, IGXBlockDiagonalApply; petiga_amd/csrc/vec_sumfact.hpp, DIAGONAL + BLOCK, and
block_diag.hpp).  B[j][n * dof + i] = A_(n,i),(n,j); the reference is R[n, i, j] = M[n * dof + i, n * dof + j] of the CPU oracle's matrix, the
cases, states and tolerances are those of tests/test_gpu_matrix_action.py plus elasticity-p2-nurbs:
  i and j free   |B - R| <= tol s_ij, s_ij = max(max_n |R_n,ij|, sqrt(s_i s_j)) over the nodes where both are free, s_f the largest free
                 |R_ff| of field f (the diagonal test's scale); tol = 1e-12 for the linear forms, 1e-11 for the Tangents
  else           exactly 0 off the diagonal, exactly the element count on it
Further: the scalar diagonal, the engine's own assembled matrix, the action on unit vectors, repeatability, a two-field run-time
struct, the refusals, Apply, Invert and a point-block-Jacobi-preconditioned CG run with the action as the operator.
Every test prints its worst ratio before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import oracle_api as O
from common import make_pair, warped_geometry
from test_gpu_matrix_action import CASES, DT, EL, NS, _action, _reference
from test_gpu_matrix_diagonal import _diagonal
from test_matrix_block_diagonal_abi import PAIR_PARAMS, USER_PAIR

pytestmark = pytest.mark.gpu

U_ROUND = 2.0 ** -53
BCASES = {k: CASES[k] for k in ("elasticity-p3", "nsvms-p2", "nsvms-p2-nurbs", "poisson-p2-odd")}
BCASES["elasticity-p2-nurbs"] = ("elasticity", 3, 2, (3, 3, 3), {}, "nurbs", CASES["elasticity-p3"][6], 1e-12)
MULTI = ["elasticity-p3", "nsvms-p2", "nsvms-p2-nurbs"]
PARAMS = {"poisson": (), "elasticity": EL, "nsvms": NS}


def _pair(name):
    form, dof, p, N, kw, geo, bcs, tol = BCASES[name]
    orc, eng = make_pair(3, dof, p, list(N), **kw)
    if geo:
        Xg, Wg = warped_geometry(orc, 3, seed=11, rational=(geo == "nurbs"), amp=0.08)
        orc.set_geometry(Xg, Wg)
        eng.set_geometry(Xg, Wg)
    for g in (orc, eng):
        for bc in bcs:
            g.set_boundary_value(*bc)
    return orc, eng


def blocks_of(M, dof):
    """R[n, i, j] = M[n * dof + i, n * dof + j] of a scipy matrix"""
    M = M.tocsr()
    n = M.shape[0] // dof
    R = np.zeros((n, dof, dof))
    rows = np.arange(n) * dof
    for i in range(dof):
        for j in range(dof):
            R[:, i, j] = np.asarray(M[rows + i, rows + j]).ravel()
    return R


def fixed_rows(M):
    off = abs(M).tolil()
    off.setdiag(0.0)
    return np.asarray(off.tocsr().sum(axis=1)).ravel() == 0.0      # a fixed row holds only its diagonal


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(U, V, R, fixed[n, dof]) of a case: computed once, shared by the tests, never written to"""
    form, dof = BCASES[name][0], BCASES[name][1]
    orc, _ = _pair(name)
    U = V = None
    if form == "poisson":
        A_o = orc.compute_system("orc_form_poisson")[0]
    elif form == "elasticity":
        A_o = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))[0]
    else:
        _, U, V = _reference(name)[:3]
        A_o = orc.compute_ijacobian("orc_form_ns_tangent", O.NSVMSCtx(*NS), 2.0 / DT, V, 0.0, U)
    M = A_o.scipy()
    R, fx = blocks_of(M, dof), fixed_rows(M).reshape(-1, dof)
    R.setflags(write=False)
    fx.setflags(write=False)
    return U, V, R, fx


def host_blocks(B, dof):
    """Bh[n, i, j] from the dof column vectors"""
    return np.stack([b.get().reshape(-1, dof) for b in B], axis=2)


def _block_diagonal(name, eng, U, V, B=None):
    form, dof = BCASES[name][0], BCASES[name][1]
    eng.set_form(form, PARAMS[form])
    B = B if B is not None else [eng.create_vec() for _ in range(dof)]
    if form in ("poisson", "elasticity"):
        eng.compute_matrix_block_diagonal(B)
    else:
        eng.compute_ijacobian_block_diagonal(2.0 / DT, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), B)
    eng.synchronize()
    kn = eng.kernel_name()
    assert "vec_sumfact" in kn and "matrix block diagonal" in kn, kn
    assert ("two elements per wavefront" in kn) == (BCASES[name][2] == 2), kn
    assert ("one wavefront per element" in kn) == (BCASES[name][2] != 2), kn
    return B


def check_blocks(Bh, R, fx, tol, what=""):
    """the bound of the module's docstring; returns the worst ratio |B - R| / s_ij over the field pairs"""
    dof = R.shape[1]
    s = [np.abs(R[:, f, f])[~fx[:, f]].max() for f in range(dof)]
    worst = 0.0
    for i in range(dof):
        for j in range(dof):
            free = ~fx[:, i] & ~fx[:, j]
            sij = max(np.abs(R[:, i, j])[~fx[:, i] & ~fx[:, j]].max(), np.sqrt(s[i] * s[j]))
            err = np.abs(Bh[:, i, j] - R[:, i, j])[free].max()
            print("%s pair (%d, %d): max|B - R| = %.3e, s_ij = %.3e, ratio %.3e (tol %g)" % (what, i, j, err, sij, err / sij, tol))
            assert err <= tol * sij
            worst = max(worst, err / sij)
            if i != j:
                assert np.all(Bh[~free, i, j] == 0.0) and np.all(R[~free, i, j] == 0.0)
            else:
                assert np.array_equal(Bh[~free, i, i], R[~free, i, i])
                assert np.all(R[~free, i, i] == np.round(R[~free, i, i])) and np.all(R[~free, i, i] >= 1)
    return worst


@pytest.mark.parametrize("name", sorted(BCASES))
def test_blocks_equal_the_oracle_matrix_blocks(name):
    U, V, R, fx = _ref(name)
    dof = BCASES[name][1]
    _, eng = _pair(name)
    Bh = host_blocks(_block_diagonal(name, eng, U, V), dof)
    assert fx.any() == bool(BCASES[name][6])
    check_blocks(Bh, R, fx, BCASES[name][7], name)
    if dof > 1:      # nodes with fixed and free fields exist in both multi-field families
        mixed = fx.any(axis=1) & ~fx.all(axis=1)
        print("%s: %d mixed nodes" % (name, mixed.sum()))
        assert mixed.any()


def test_blocks_are_not_transposed():
    """NS-VMS: the reference blocks are non-symmetric (max|R_30| = 1.90e-2 against max|R_03| = 9.51e-3) and B matches them as they are"""
    U, V, R, fx = _ref("nsvms-p2")
    a, b = np.abs(R[:, 3, 0]).max(), np.abs(R[:, 0, 3]).max()
    print("max|R_30| = %.3e, max|R_03| = %.3e" % (a, b))
    assert abs(a - b) > 0.1 * max(a, b)
    asym = np.abs(R - R.transpose(0, 2, 1)).max()
    assert asym > 1e-3
    _, eng = _pair("nsvms-p2")
    Bh = host_blocks(_block_diagonal("nsvms-p2", eng, U, V), 4)
    check_blocks(Bh, R, fx, BCASES["nsvms-p2"][7], "nsvms-p2 (as it is)")
    assert np.abs(Bh - R.transpose(0, 2, 1)).max() > 0.5 * asym


@pytest.mark.parametrize("name", MULTI)
def test_block_diagonals_agree_with_the_scalar_diagonal(name):
    U, V, R, fx = _ref(name)
    dof = BCASES[name][1]
    _, eng = _pair(name)
    Bh = host_blocks(_block_diagonal(name, eng, U, V), dof)
    D = _diagonal(name, eng, U, V).get().reshape(-1, dof)
    for f in range(dof):
        free = ~fx[:, f]
        s = np.abs(R[:, f, f])[free].max()
        err = np.abs(Bh[:, f, f] - D[:, f]).max()
        print("%s field %d: max|B_ff - D_f| = %.3e, ratio %.3e" % (name, f, err, err / s))
        assert err <= BCASES[name][7] * s
        assert np.array_equal(Bh[~free, f, f], D[~free, f])


def test_blocks_equal_the_engines_own_ijacobian_blocks():
    import scipy.sparse as sp
    name = "nsvms-p2"
    U, V, R, fx = _ref(name)
    _, eng = _pair(name)
    Bh = host_blocks(_block_diagonal(name, eng, U, V), 4)
    A = eng.create_mat()
    eng.compute_ijacobian(2.0 / DT, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), A)
    eng.synchronize()
    rows, cols, vals = A.to_coo_global()
    M = sp.coo_matrix((vals, (rows, cols)), shape=(R.shape[0] * 4,) * 2).tocsr()
    check_blocks(Bh, blocks_of(M, 4), fx, BCASES[name][7], name + " (engine)")


@pytest.mark.parametrize("name", ["elasticity-p3", "nsvms-p2-nurbs"])
def test_blocks_are_consistent_with_the_action_on_unit_vectors(name):
    """at a random node n and every j, Y = A e_(n,j) from the action: Y at rows (n, .) is column j of the node's block"""
    U, V, R, fx = _ref(name)
    dof = BCASES[name][1]
    _, eng = _pair(name)
    Bh = host_blocks(_block_diagonal(name, eng, U, V), dof)
    s = [np.abs(R[:, f, f])[~fx[:, f]].max() for f in range(dof)]
    n = int(np.random.default_rng(43).integers(R.shape[0]))
    for j in range(dof):
        e = np.zeros(R.shape[0] * dof)
        e[n * dof + j] = 1.0
        Y = _action(name, eng, e, U, V).get().reshape(-1, dof)
        for i in range(dof):
            sij = max(np.abs(R[:, i, j])[~fx[:, i] & ~fx[:, j]].max(), np.sqrt(s[i] * s[j]))
            print("%s node %d (%d, %d): Y = %.17g, B = %.17g, ratio %.3e" % (name, n, i, j, Y[n, i], Bh[n, i, j], abs(Y[n, i] - Bh[n, i, j]) / sij))
            assert abs(Y[n, i] - Bh[n, i, j]) <= BCASES[name][7] * sij


@pytest.mark.parametrize("name", ["elasticity-p3", "nsvms-p2"])
def test_block_diagonal_is_bit_repeatable(name):
    """two calls return the same bits (the colours run in a fixed order), and so does a call into NaN-poisoned columns (the driver zeroes them)"""
    U, V = _ref(name)[:2]
    dof = BCASES[name][1]
    _, eng = _pair(name)
    B = _block_diagonal(name, eng, U, V)
    B1 = host_blocks(B, dof).copy()
    assert np.all(np.isfinite(B1))
    assert np.array_equal(host_blocks(_block_diagonal(name, eng, U, V), dof), B1)
    for b in B:
        b.set(np.full(b.n, np.nan))
    assert np.array_equal(host_blocks(_block_diagonal(name, eng, U, V, B), dof), B1)


@pytest.mark.parametrize("geo", [None, "poly"])
def test_run_time_two_field_struct(geo):
    """UserPair against the engine's own IGXComputeMatrix of the same struct (another kernel) and against the action on unit vectors"""
    import scipy.sparse as sp
    orc, eng = make_pair(3, 2, 2, [4, 4, 3])
    if geo:
        Xg, Wg = warped_geometry(orc, 3, seed=9, rational=False, amp=0.08)
        eng.set_geometry(Xg, Wg)
    eng.set_boundary_value(0, 0, 0, 2.0)
    eng.set_boundary_value(2, 1, 1, -1.0)
    eng.set_form_source(USER_PAIR, "UserPair", PAIR_PARAMS)
    B = [eng.create_vec() for _ in range(2)]
    eng.compute_matrix_block_diagonal(B)
    eng.synchronize()
    kn = eng.kernel_name()
    assert "hiprtc" in kn and "matrix block diagonal" in kn and "two elements per wavefront" in kn, kn
    Bh = host_blocks(B, 2)
    A, A2 = eng.create_mat(), eng.create_mat()
    eng.compute_matrix(A)                       # (IGAComputeMatrix fixes nothing: the entries with i and j free)
    eng.compute_system(A2, eng.create_vec())    # (IGAElementFixSystem's matrix half is IGAElementFixJacobian: the others)
    eng.synchronize()
    blocks = []
    for Am in (A, A2):
        rows, cols, vals = Am.to_coo_global()
        blocks.append(blocks_of(sp.coo_matrix((vals, (rows, cols)), shape=(Bh.shape[0] * 2,) * 2).tocsr(), 2))
    Rm, R = blocks
    fx = np.zeros(R.shape[:2], dtype=bool)
    nn = orc.global_size() // 2
    assert nn == 6 * 6 * 5                     # nodes per axis: 6, 6, 5, axis 0 fastest
    idx = np.arange(nn)
    fx[:, 0] = idx % 6 == 0                    # field 0 on the lower face of axis 0
    fx[:, 1] = idx // 36 == 4                  # field 1 on the upper face of axis 2
    assert np.abs(R[:, 0, 1]).max() > 0 and np.all(R[:, 1, 0] == 0)      # the struct is not symmetric
    check_blocks(Bh, R, fx, 1e-12, "UserPair %s" % geo)
    for i in range(2):
        for j in range(2):
            free = ~fx[:, i] & ~fx[:, j]
            assert np.array_equal(Rm[free, i, j], R[free, i, j])
    s = [np.abs(R[:, f, f])[~fx[:, f]].max() for f in range(2)]
    n = int(np.random.default_rng(47).integers(nn))
    Xv, Yv = eng.create_vec(), eng.create_vec()
    for j in range(2):
        e = np.zeros(nn * 2)
        e[n * 2 + j] = 1.0
        eng.compute_matrix_action(Xv.set(e), Yv)
        eng.synchronize()
        Y = Yv.get().reshape(-1, 2)
        for i in range(2):
            assert abs(Y[n, i] - Bh[n, i, j]) <= 1e-12 * max(np.abs(R[:, i, j])[~fx[:, i] & ~fx[:, j]].max(), np.sqrt(s[i] * s[j]))


def test_refusals_name_their_reason(monkeypatch):
    import petiga_amd as P
    from test_gpu_matrix_action import _pair as action_pair

    def refused(eng, word, code=56, form="poisson", params=(), nb=1):
        eng.set_form(form, params)
        B = [eng.create_vec() for _ in range(nb)]
        with pytest.raises(P.IGXError) as e:
            eng.compute_matrix_block_diagonal(B)
        assert e.value.code == code and word in str(e.value) and "block diagonal" in str(e.value), str(e.value)

    _, ch = action_pair("ch-p2")
    ch.set_form("cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0))
    Uv, Vv, B = ch.create_vec(), ch.create_vec(), [ch.create_vec()]
    with pytest.raises(P.IGXError) as e:
        ch.compute_ijacobian_block_diagonal(250.0, Vv, 0.0, Uv, B)
    assert e.value.code == 56 and "second-order" in str(e.value) and "block diagonal" in str(e.value), str(e.value)

    _, eng = _pair("poisson-p2-odd")
    eng.set_boundary_form(0, 1, True)
    refused(eng, "boundary-form")
    eng.set_boundary_form(0, 1, False)
    eng.set_kernel(1)
    refused(eng, "IGXSetKernel")
    eng.set_kernel(0)
    _block_diagonal("poisson-p2-odd", eng, None, None)      # a refused call leaves nothing behind: the covered call reports its own kernel
    g2 = P.IGX(2, 1)
    for i in range(2):
        g2.axis_uniform(i, 2, 4)
    g2.setup()
    refused(g2, "dim")

    U, V = _ref("nsvms-p2")[:2]
    _, ns = _pair("nsvms-p2")
    ns.set_form("nsvms", NS)
    Uv, Vv = ns.create_vec().set(U), ns.create_vec().set(V)
    B = [ns.create_vec() for _ in range(4)]
    other = _pair("nsvms-p2")[1]
    for bad in (B[:3], B[:3] + [B[0]], B[:3] + [other.create_vec()], B[:3] + [Uv]):      # nb != dof, a repeated column, another IGX, aliasing U
        with pytest.raises(P.IGXError) as e:
            ns.compute_ijacobian_block_diagonal(2.0 / DT, Vv, 0.0, Uv, bad)
        assert e.value.code == 62, str(e.value)
    Xv = ns.create_vec()
    for X, Y in ((Xv, Xv), (B[1], Xv), (Xv, B[2])):
        with pytest.raises(P.IGXError) as e:
            ns.block_diagonal_apply(B, X, Y)
        assert e.value.code == 62, str(e.value)
    _block_diagonal("nsvms-p2", ns, U, V, B)
    fresh = P.IGX(3, 1)
    for i in range(3):
        fresh.axis_uniform(i, 2, 3)
    fresh.setup()
    with pytest.raises(P.IGXError) as e:
        fresh.compute_matrix_block_diagonal([fresh.create_vec()])      # no form set
    assert e.value.code == 73, str(e.value)
    monkeypatch.setenv("IGX_VEC_SUMFACT", "0")      # (read when the IGX is created)
    _, off = _pair("poisson-p2-odd")
    refused(off, "IGX_VEC_SUMFACT")


@pytest.mark.parametrize("name", MULTI)
def test_apply(name):
    """Y_n = B_n X_n against einsum on the read-back blocks: |Y - R| <= 4 dof u (|B| |X|)_row, the rounding of a dof-term dot product
    with margin for the order of the fused multiply-adds"""
    U, V = _ref(name)[:2]
    dof = BCASES[name][1]
    _, eng = _pair(name)
    B = _block_diagonal(name, eng, U, V)
    Bh = host_blocks(B, dof)
    X = np.random.default_rng(53).standard_normal(Bh.shape[:2])
    Xv, Yv = eng.create_vec().set(X.ravel()), eng.create_vec()
    eng.block_diagonal_apply(B, Xv, Yv)
    eng.synchronize()
    assert "block_diag_apply" in eng.kernel_name()
    Y = Yv.get().reshape(-1, dof)
    want, bound = np.einsum("nij,nj->ni", Bh, X), np.einsum("nij,nj->ni", np.abs(Bh), np.abs(X))
    ratio = (np.abs(Y - want) / np.where(bound > 0, bound, 1.0)).max() / U_ROUND
    print("%s Apply: worst |Y - R| / (u (|B||X|)_row) = %.3f (bound %d)" % (name, ratio, 4 * dof))
    assert np.all(np.abs(Y - want) <= 4 * dof * U_ROUND * bound), ratio


@pytest.mark.parametrize("name", MULTI)
def test_invert(name):
    """per node max|B_n Binv_n - I| <= 16 dof u cond(B_n): the first-order bound of a backward-stable solve with a factor 16 for
    pivot growth; cond <= 1e6 on the read-back blocks so that the test cannot pass on garbage"""
    U, V = _ref(name)[:2]
    dof = BCASES[name][1]
    _, eng = _pair(name)
    B = _block_diagonal(name, eng, U, V)
    Bh = host_blocks(B, dof).copy()
    cond = np.linalg.cond(Bh)
    print("%s: cond up to %.3e" % (name, cond.max()))
    assert np.all(np.isfinite(cond)) and cond.max() <= 1e6
    assert eng.block_diagonal_invert(B) == 0
    assert "block_diag_invert" in eng.kernel_name()
    Bi = host_blocks(B, dof)
    res = np.abs(np.einsum("nij,njk->nik", Bh, Bi) - np.eye(dof)).max(axis=(1, 2))
    ratio = (res / (dof * U_ROUND * cond)).max()
    print("%s Invert: worst max|B Binv - I| / (dof u cond) = %.3f (bound 16)" % (name, ratio))
    assert np.all(res <= 16 * dof * U_ROUND * cond), ratio


def test_invert_counts_a_singular_block_and_zeroes_it():
    name = "elasticity-p3"
    _, eng = _pair(name)
    B = _block_diagonal(name, eng, None, None)
    Bh = host_blocks(B, 3).copy()
    Bh[5] = 0.0
    for j, b in enumerate(B):
        b.set(Bh[:, :, j].ravel())
    assert eng.block_diagonal_invert(B) == 1
    Bi = host_blocks(B, 3)
    assert np.all(Bi[5] == 0.0)
    keep = np.arange(Bh.shape[0]) != 5
    res = np.abs(np.einsum("nij,njk->nik", Bh[keep], Bi[keep]) - np.eye(3)).max(axis=(1, 2))
    assert np.all(res <= 16 * 3 * U_ROUND * np.linalg.cond(Bh[keep]))
    assert eng.block_diagonal_invert(B, count=False) is None      # (no count, no synchronisation)


def test_point_block_jacobi_preconditioned_cg_on_the_action():
    """End to end: Elasticity (lambda, mu) = (1.5, 0.8), p = 2 on (4, 3, 3) elements, 450 unknowns; the three fields are 0 on the lower
    face of axis 0 and field 0 is 0.1 on the upper one.  CG on the host with IGXComputeMatrixAction as the operator, the GPU's inverted
    blocks through IGXBlockDiagonalApply as the preconditioner and IGXComputeSystem's right-hand side, both stopping norms of the
    Jacobi test at 1e-10.  On the oracle's own matrix this CG takes 57 iterations (error 5.6e-11) against 55 for scalar Jacobi: no
    gain in iterations is asserted, on this isotropic problem there is none to expect."""
    import scipy.sparse.linalg as spla
    orc, eng = make_pair(3, 3, 2, [4, 3, 3])
    for g in (orc, eng):
        for f in range(3):
            g.set_boundary_value(0, 0, f, 0.0)
        g.set_boundary_value(0, 1, 0, 0.1)
    eng.set_form("elasticity", EL)
    A, b = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, b)
    eng.synchronize()
    rhs = b.get().copy()
    n = rhs.size
    assert n == 450
    B = [eng.create_vec() for _ in range(3)]
    eng.compute_matrix_block_diagonal(B)
    assert eng.block_diagonal_invert(B) == 0
    Xv, Yv = eng.create_vec(), eng.create_vec()

    def op(x):
        eng.compute_matrix_action(Xv.set(x), Yv)
        eng.synchronize()
        return Yv.get().copy()

    def pc(r):
        eng.block_diagonal_apply(B, Xv.set(r), Yv)
        eng.synchronize()
        return Yv.get().copy()

    x = np.zeros(n)
    r = rhs - op(x)
    z = pc(r)
    p = z.copy()
    rz, norm0, normz0, its = r @ z, np.linalg.norm(rhs), np.linalg.norm(pc(rhs)), 0
    while (np.linalg.norm(r) > 1e-10 * norm0 or np.linalg.norm(z) > 1e-10 * normz0) and its < n:
        Ap = op(p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = pc(r)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        its += 1
    print("point-block-Jacobi CG: %d iterations for %d unknowns, relative residual %.3e, preconditioned %.3e"
          % (its, n, np.linalg.norm(r) / norm0, np.linalg.norm(z) / normz0))
    assert np.linalg.norm(r) <= 1e-10 * norm0 and np.linalg.norm(z) <= 1e-10 * normz0 and its <= n
    A_o, b_o = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))
    want = spla.spsolve(A_o.scipy().tocsc(), np.asarray(b_o))
    print("max|x - spsolve| = %.3e, max|spsolve| = %.3f" % (np.abs(x - want).max(), np.abs(want).max()))
    assert np.abs(x - want).max() <= 1e-8 * np.abs(want).max()
