"""tests/multigrid_ref.py, the numpy restatement of IGXMultigrid's cycle, calibrated on the CPU: 3-D Poisson on the parametric cube with all
faces Dirichlet, the oracle's matrices (orc.compute_system("orc_form_poisson"): fixed rows included, as the engine's actions see them) and
transfer_ref's P = T (x) T (x) T, an exact coarse solve, the outer loop krylov_ref.cg to rtol = 1e-10 on a random right-hand side.

  B is symmetric      |x.By - y.Bx| <= 1e-12 |x| |By| on random vectors, and e_i.B e_i > 0 on unit vectors
  B A contracts       p = 2, 4^3 -> 8^3 elements (n = 1000): the spectral radius of I - B A from the dense eigenvalues is below 1
  the counts          MG-PCG at 4 -> 8 -> 16 needs at most 4 iterations more than at 4 -> 8 (p = 2, degree 2); MG-PCG needs at most half of
                      Jacobi-PCG's count at p = 2 and p = 3.  Seen with these matrices: 14 and 15 against Jacobi's 46 and 54 at p = 2,
                      49 against 156 at p = 3 (degree 2); with Chebyshev degree 3: 10, 12 and 37.  The counts are printed: if the oracle's
                      matrices move them, the printed counts are the record.  They are flat in the mesh and grow with the degree p: a
                      Jacobi smoother is not p-robust on splines.
  three wrong cycles  "post-zero" (the post-smoother starts from zero and so throws the coarse correction away: I - B A is then the
                      smoother's own error polynomial p_k(D^-1 A), whose largest value on the spectrum the true cycle beats by 0.1 and more), "unmasked" (the coarse fixed rows keep
                      what the restriction put there: the correction is then not zero on the fine fixed rows) and "stale-rho" (rho_j not
                      updated: the smoother's error is then not the Chebyshev polynomial T_k((theta - t) / delta) / T_k(theta / delta)) are
                      each caught by the property named."""
import functools

import numpy as np
import pytest

import krylov_ref as K
import multigrid_ref as M
import transfer_ref as TR
from common import make_pair

ALL6 = [(d, s) for d in range(3) for s in range(2)]
FIXED = [(d, s, 0) for d, s in ALL6]


@functools.lru_cache(maxsize=None)
def _matrix(p, N):
    orc, _ = make_pair(3, 1, p, [N] * 3, engine=False)
    for d, s in ALL6:
        orc.set_boundary_value(d, s, 0, 0.0)
    return orc.compute_system("orc_form_poisson")[0].scipy().tocsr()


@functools.lru_cache(maxsize=None)
def _prolongation(p, Nc, Nf):
    import scipy.sparse as sp
    T = sp.csr_matrix(np.asarray(TR.matrix_rowwise(p, TR.uniform_knots(p, Nc), TR.uniform_knots(p, Nf)), dtype=np.float64))
    return sp.kron(sp.kron(T, T), T).tocsr()


def hierarchy(p, Ns, **kw):
    As = [_matrix(p, N) for N in Ns]
    Ps = [_prolongation(p, Nc, Nf) for Nc, Nf in zip(Ns[:-1], Ns[1:])]
    masks = [M.fixed_mask([N + p] * 3, 1, FIXED) for N in Ns]
    return As[-1], masks, M.dense_hierarchy(As, Ps, masks, **kw).setup()


def _counts(p, Ns, degree):
    A, _, h = hierarchy(p, Ns, degree=degree)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    D = A.diagonal()
    _, mg = K.cg(lambda v: A @ v, h.apply, b, rtol=1e-10, maxit=2000)
    _, jac = K.cg(lambda v: A @ v, lambda v: v / D, b, rtol=1e-10, maxit=2000)
    assert mg["reason"] == K.CONVERGED_RTOL == jac["reason"]
    print("p = %d, elements %s, Chebyshev degree %d: MG-PCG %d iterations, Jacobi-PCG %d; lambda %s"
          % (p, " -> ".join(str(N) for N in Ns), degree, mg["iterations"], jac["iterations"], ["%.4f" % l.lam for l in h.levels[1:]]))
    return mg["iterations"], jac["iterations"]


def test_b_is_symmetric_and_positive():
    A, _, h = hierarchy(2, (4, 8))
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(4):
        x, y = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        Bx, By = h.apply(x), h.apply(y)
        gap = abs(x @ By - y @ Bx) / (np.linalg.norm(x) * np.linalg.norm(By))
        worst = max(worst, gap)
    print("|x.By - y.Bx| / (|x| |By|) <= %.3e" % worst)
    assert worst <= 1e-12
    for i in rng.choice(A.shape[0], 40, replace=False):
        e = np.zeros(A.shape[0])
        e[i] = 1.0
        assert e @ h.apply(e) > 0.0


def _radius(h, A):
    n = A.shape[0]
    BA = np.column_stack([h.apply(A[:, j].toarray().ravel()) for j in range(n)])
    return float(np.abs(np.linalg.eigvals(np.eye(n) - BA)).max())


def test_the_cycle_contracts_and_a_post_smoother_from_zero_is_caught():
    A, _, h = hierarchy(2, (4, 8))
    assert A.shape[0] == 1000
    rho = _radius(h, A.tocsc())
    _, _, wrong = hierarchy(2, (4, 8), wrong="post-zero")
    rho_wrong = _radius(wrong, A.tocsc())
    # the post-smoother from zero throws the coarse correction away: I - B A is then the smoother's own error polynomial p_k(D^-1 A), whose
    # largest value on the spectrum the true cycle has to beat
    t = np.linalg.eigvals(A.toarray() / A.diagonal()[:, None]).real
    lam, k = h.levels[1].lam, h.degree
    theta, delta = (h.hi + h.lo) * lam / 2, (h.hi - h.lo) * lam / 2
    Tk = lambda x: np.polynomial.chebyshev.chebval(x, [0.0] * k + [1.0])
    smoother = float(np.abs(Tk((theta - t) / delta) / Tk(theta / delta)).max())
    print("spectral radius of I - B A: %.4f; with the post-smoother from a zero guess: %.4f; max |p_k| on the spectrum of D^-1 A: %.4f" % (rho, rho_wrong, smoother))
    assert rho < 1.0
    assert abs(rho_wrong - smoother) <= 1e-8 and rho < smoother - 0.1


def test_counts_are_flat_in_the_mesh_and_at_most_half_of_jacobi():
    two, jac2 = _counts(2, (4, 8), 2)
    three, jac3 = _counts(2, (4, 8, 16), 2)
    assert three <= two + 4
    assert 2 * two <= jac2 and 2 * three <= jac3
    mg, jac = _counts(3, (4, 8), 2)
    assert 2 * mg <= jac


def test_unmasked_coarse_rows_are_caught():
    """a right-hand side that is not zero on the Dirichlet rows: with the mask the coarse right-hand side and the correction are exactly zero on
    the fixed rows of their levels; without it neither is"""
    rng = np.random.default_rng(9)
    for wrong in (None, "unmasked"):
        A, masks, h = hierarchy(2, (4, 8, 16), wrong=wrong)
        h.apply(rng.standard_normal(A.shape[0]))
        coarse = [np.abs(h.trace[("restricted", l)][masks[l]]).max() for l in (0, 1)]
        fine = [np.abs(h.trace[("correction", l)][masks[l]]).max() for l in (1, 2)]
        print("%s: max |b_coarse| on the fixed rows %s, max |P e| on the fine fixed rows %s" % (wrong or "the cycle", coarse, fine))
        if wrong is None:
            assert coarse == [0.0, 0.0] and fine == [0.0, 0.0]
        else:
            assert min(coarse) > 0.0 and min(fine) > 0.0


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_the_smoother_is_the_chebyshev_polynomial_and_a_stale_rho_is_caught(degree):
    """On A = diag(t), D = I the error after Smooth from a zero guess is e_k = p_k(t) e_0 with p_k(t) = T_k((theta - t) / delta) / T_k(theta / delta)"""
    t = np.linspace(0.05, 2.0, 40)
    lam, lo, hi = 1.9, 0.1, 1.1
    theta, delta = (hi + lo) * lam / 2, (hi - lo) * lam / 2
    Tk = lambda x: np.polynomial.chebyshev.chebval(x, [0.0] * degree + [1.0])
    want = Tk((theta - t) / delta) / Tk(theta / delta)
    x_true = np.ones_like(t)
    for wrong in (None, "stale-rho"):
        lv = M.Level(t.size, (lambda v: t * v), (lambda v: v.copy()), lam=lam)
        h = M.Hierarchy([lv], degree=degree, lo=lo, hi=hi, wrong=wrong)
        x, _, _ = M.smooth(h, 0, t * x_true)
        err = np.abs((x_true - x) - want).max()
        print("degree %d, %s: max |e_k - p_k(t)| = %.3e" % (degree, wrong or "the smoother", err))
        if wrong is None or degree < 3:      # rho_2 is formed from rho_1 either way: the stale rho shows from step 3 on
            assert err <= 1e-13
        else:
            assert err > 1e-3
