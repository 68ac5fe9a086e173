"""tests/eigen_ref.py -- the numpy restatement of IGXEigenSolve's loop -- calibrated on the oracle's matrices, without a GPU: Poisson and Mass,
p = 2, 6^3 elements, all faces Dirichlet (the cube's spectrum: a single lowest eigenvalue, then a triple one, so nev = 4 cuts in a gap).
The reference is scipy.linalg.eigh on the free rows.
  eigenvalues    |theta_k - lambda_k| <= |B^-1/2 r_k| / |B^1/2 x_k| in sorted order (Parlett's residual bound for a definite pencil: derived,
                 no constant to tune), to which the rounding of the reference itself is added: 64 u lambda_k (eigh's backward error on a
                 216 x 216 pencil of condition < 100 stays far below it)
  orthonormality max |X^T B X - I| <= ORTHO_TOL = 1e-10: X = S C with C^T G_B C = I to the rounding of the dense solve, q u kappa(G_B) with
                 q = 18 and the scaled G_B's condition below 1e4 while the block is away from exact dependence (printed below)
  fixed rows     exactly zero
  wrong loops    P never dropped on an indefinite G_B; the residual formed with a stale theta; W not passed through B in G_B: each is
                 caught by one of the checks above
Every test prints what it sees before it asserts (run with -s)."""
import functools

import numpy as np

import eigen_ref as E
import oracle_api as O
from common import make_pair

U = 2.0 ** -53
ORTHO_TOL = 1e-10
ALL6 = [(d, s) for d in range(3) for s in range(2)]


@functools.lru_cache(maxsize=None)
def cube(p=2, N=6):
    """(A, B, free mask) of the oracle: Poisson and Mass on the parametric cube, all faces Dirichlet"""
    mats = []
    for form in ("orc_form_poisson", "orc_form_mass"):
        orc, _ = make_pair(3, 1, p, [N] * 3, engine=False)
        for d, s in ALL6:
            orc.set_boundary_value(d, s, 0, 0.0)
        M, _ = orc.compute_system(form)
        mats.append(M.scipy().tocsr())
    nn = N + p
    i = np.arange(nn)
    edge = (i == 0) | (i == nn - 1)
    fixed = (edge[:, None, None] | edge[None, :, None] | edge[None, None, :]).reshape(-1)
    return mats[0], mats[1], ~fixed


def start_block(n, m):
    return np.random.default_rng(0).standard_normal((m, n)).T.copy()      # column j: the j-th draw of n numbers, as IGX.eigen writes them


def check(out, A, B, free, nev, label):
    lam_ref, _ = E.dense_reference(A, B, free, out["X"].shape[1])
    bound, rnorm = E.parlett_bounds(A, B, free, out["X"], out["lam"])
    err = np.abs(out["lam"] - lam_ref)
    defect = E.orthonormality_defect(B, out["X"])
    print("%s: %d iterations, reason %d, restarts %d; lambda %s; |theta - lambda| %s; Parlett bounds %s; |X^T B X - I| %.3e"
          % (label, out["iterations"], out["reason"], out["restarts"], np.array2string(out["lam"][:nev], precision=6), np.array2string(err[:nev], precision=2),
             np.array2string(bound[:nev], precision=2), defect))
    ok = bool(np.all(err[:nev] <= bound[:nev] + 64 * U * np.abs(lam_ref[:nev])))
    return ok, defect, rnorm


def test_the_loop_finds_the_cubes_lowest_pairs():
    A, B, free = cube()
    X0 = start_block(A.shape[0], 6)
    d = A.diagonal()
    for pc, T in (("none", None), ("jacobi", lambda r: r / d)):
        out = E.lobpcg(A, B, X0, 4, T=T, rtol=1e-8, maxit=200, fixed=~free)
        ok, defect, rnorm = check(out, A, B, free, 4, "cube p=2 6^3, pc=" + pc)
        assert out["reason"] == E.CONVERGED and out["nconverged"] == 4
        assert ok and defect <= ORTHO_TOL
        assert not out["X"][~free].any(), "a fixed row is not exactly zero"
        assert np.all(np.diff(out["lam"]) >= 0)
        assert np.allclose(out["resid"], rnorm, rtol=1e-6, atol=1e-12)
        assert out["history"].shape == (out["iterations"] + 1, 6) and np.array_equal(out["history"][-1], out["resid"])
        assert out["actions"] == 2 * 6 * (out["iterations"] + 1)
        # the triple second eigenvalue: the subspace, not the vectors
        lam_ref, V = E.dense_reference(A, B, free, 4)
        assert abs(lam_ref[1] - lam_ref[3]) <= 1e-9 * lam_ref[1] and lam_ref[1] - lam_ref[0] > 1.0
        angle = E.largest_principal_angle(B, out["X"][:, 1:4], V[:, 1:4])
        print("  largest principal angle of the triple eigenvalue's subspace: %.3e" % angle)
        assert angle <= 1e-5      # sin(angle) <= |r| / gap (Davis-Kahan): |r| <= 1e-8 |A x|, the gap to the next eigenvalue is O(10)


def test_identity_mass():
    A, _, free = cube()
    out = E.lobpcg(A, None, start_block(A.shape[0], 6), 4, rtol=1e-8, maxit=300, fixed=~free)
    ok, defect, _ = check(out, A, None, free, 4, "cube p=2 6^3, B = I")
    assert out["reason"] == E.CONVERGED and ok and defect <= ORTHO_TOL and not out["X"][~free].any()
    assert out["actions"] == 6 * (out["iterations"] + 1)


def test_a_stale_theta_is_caught():
    """after three iterations the residual the loop reports must be the residual of the pair it returns"""
    A, B, free = cube()
    X0 = start_block(A.shape[0], 6)
    good = E.lobpcg(A, B, X0, 4, maxit=3, fixed=~free)
    bad = E.lobpcg(A, B, X0, 4, maxit=3, fixed=~free, wrong="stale_theta")
    for out, right in ((good, True), (bad, False)):
        _, rnorm = E.parlett_bounds(A, B, free, out["X"], out["lam"])
        dev = np.abs(out["resid"] - rnorm).max() / rnorm.max()
        print("%s loop: reported residuals deviate from the recomputed ones by %.3e" % ("right" if right else "stale-theta", dev))
        assert out["reason"] == E.DIVERGED_ITS and out["iterations"] == 3
        assert (dev <= 1e-10) == right


def test_w_not_passed_through_b_is_caught():
    A, B, free = cube()
    X0 = start_block(A.shape[0], 6)
    bad = E.lobpcg(A, B, X0, 4, maxit=5, fixed=~free, wrong="w_not_b")
    good = E.lobpcg(A, B, X0, 4, maxit=5, fixed=~free)
    print("defect of X^T B X - I after 5 iterations: right loop %.3e, W-not-through-B loop %.3e" % (E.orthonormality_defect(B, good["X"]), E.orthonormality_defect(B, bad["X"])))
    assert E.orthonormality_defect(B, good["X"]) <= ORTHO_TOL < E.orthonormality_defect(B, bad["X"])


def test_p_kept_on_an_indefinite_gram_matrix_is_caught():
    """A preconditioner of rank m -- the projector on six fixed directions Z -- puts every W into span Z, and P = W C_W with it: once P is
    present [W P] has 12 columns in a space of 6 and G_B cannot be positive definite, while [X W] can.  The loop drops P, counts the
    restart and goes on (every iteration: it is a Rayleigh-Ritz iteration on the fixed span [X Z], which keeps X B-orthonormal and never
    raises a Ritz value past rounding); the loop that keeps P breaks down in the first iteration that has one."""
    A, B, free = cube()
    n = A.shape[0]
    X0 = start_block(n, 6)
    Z = np.zeros((n, 6))
    Z[np.flatnonzero(free), :] = np.linalg.qr(np.random.default_rng(1).standard_normal((int(free.sum()), 6)))[0]
    proj = lambda r: Z @ (Z.T @ r)
    good = E.lobpcg(A, B, X0, 4, T=proj, maxit=10, fixed=~free)
    bad = E.lobpcg(A, B, X0, 4, T=proj, maxit=10, fixed=~free, wrong="keep_p")
    first = E.lobpcg(A, B, X0, 4, T=proj, maxit=1, fixed=~free)
    defect = E.orthonormality_defect(B, good["X"])
    print("rank-6 preconditioner: right loop reason %d after %d iterations, %d restarts, |X^T B X - I| %.3e, sum of Ritz values %.6f (after one iteration %.6f); "
          "P-kept loop: reason %d after %d iterations" % (good["reason"], good["iterations"], good["restarts"], defect, good["lam"].sum(), first["lam"].sum(), bad["reason"], bad["iterations"]))
    assert good["reason"] == E.DIVERGED_ITS and good["iterations"] == 10 and good["restarts"] == 9
    assert defect <= ORTHO_TOL and good["lam"].sum() <= first["lam"].sum() * (1 + 64 * U) and not good["X"][~free].any()
    assert bad["reason"] == E.DIVERGED_BREAKDOWN and bad["iterations"] == 1 and bad["restarts"] == 0


def test_two_equal_start_columns_break_down_at_once():
    A, B, free = cube()
    X0 = start_block(A.shape[0], 6)
    X0[:, 3] = X0[:, 1]
    out = E.lobpcg(A, B, X0, 4, fixed=~free)
    print("two equal columns: reason %d, restarts %d, %d iterations" % (out["reason"], out["restarts"], out["iterations"]))
    assert out["reason"] == E.DIVERGED_BREAKDOWN and out["iterations"] == 0      # G_B of the start block is singular and there is no P to drop
