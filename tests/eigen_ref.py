"""A numpy restatement of IGXEigenSolve's loop (include/petiga_amd.h, steps 0-7) on matrices or callables: LOBPCG with a block of m columns
for the nev lowest pairs of A x = lambda B x, S = [X W P], the Gram matrices symmetrised and scaled by 1 / sqrt(diag G_B), the m lowest
pairs of the dense definite pencil (scipy.linalg.eigh in place of the library's long-double solver), P dropped once when G_B is not
positive definite, no locking.  `wrong` switches one of three mistakes on, for the tests that must catch them:
  "keep_p"       P is never dropped: an indefinite G_B with P present is a breakdown
  "stale_theta"  the residual is formed with the Ritz values of the iteration before
  "w_not_b"      G_B takes W where it needs B W
Also here: the bounds and measures the CPU and GPU tests share (Parlett's residual bound, the B-orthonormality defect, principal angles)."""
import numpy as np
import scipy.linalg as sla

CONVERGED, DIVERGED_ITS, DIVERGED_BREAKDOWN, DIVERGED_NAN = 1, -1, -2, -3


def _apply(op, V):
    if op is None:
        return V
    if callable(op):
        return np.column_stack([op(V[:, j]) for j in range(V.shape[1])])
    return np.asarray(op @ V)


def rayleigh_ritz(GA, GB, m):
    """(status, C [q, m], theta [m]); status 0, 1 (G_B not positive definite, or its diagonal not positive) or 2 (an entry not finite)"""
    if not (np.all(np.isfinite(GA)) and np.all(np.isfinite(GB))):
        return 2, None, None
    b = np.diag(GB)
    if not np.all(b > 0):
        return 1, None, None
    d = 1.0 / np.sqrt(b)
    A = 0.5 * (GA + GA.T) * d[:, None] * d[None, :]
    B = 0.5 * (GB + GB.T) * d[:, None] * d[None, :]
    try:
        lam, U = sla.eigh(A, B)
    except (np.linalg.LinAlgError, sla.LinAlgError):
        return 1, None, None
    return 0, d[:, None] * U[:, :m], lam[:m]


def lobpcg(A, B, X0, nev, T=None, rtol=1e-8, atol=0.0, maxit=200, fixed=None, wrong=None):
    """X0 [n, m].  Returns dict(X, lam, resid, iterations, reason, nconverged, restarts, actions, history [iterations + 1, m])."""
    X = np.array(X0, dtype=np.float64)
    n, m = X.shape
    if fixed is not None:
        X[fixed, :] = 0.0
    actions = [0]

    def act(V):
        actions[0] += V.shape[1] * (1 if B is None else 2)
        return _apply(A, V), _apply(B, V)

    its, reason, restarts, nconv = 0, 0, 0, 0
    theta, rn, hist = np.zeros(m), np.zeros(m), []
    AX, BX = act(X)
    status, C, th = rayleigh_ritz(X.T @ AX, X.T @ BX, m)
    if status:
        reason = DIVERGED_NAN if status == 2 else DIVERGED_BREAKDOWN
    else:
        X, AX, BX, theta = X @ C, AX @ C, BX @ C, th
    stale = theta.copy()
    P = AP = BP = None
    while not reason:
        R = AX - (stale if wrong == "stale_theta" else theta)[None, :] * BX
        rn = np.sqrt(np.sum(R * R, axis=0))
        an = np.sqrt(np.sum(AX * AX, axis=0))
        hist.append(rn.copy())
        nconv = int(np.count_nonzero(rn[:nev] <= np.maximum(rtol * an[:nev], atol)))
        if np.any(np.isnan(rn)):
            reason = DIVERGED_NAN
            break
        if nconv == nev:
            reason = CONVERGED
            break
        if its >= maxit:
            reason = DIVERGED_ITS
            break
        W = R if T is None else np.column_stack([T(R[:, j]) for j in range(m)])
        AW, BW = act(W)
        have_p = P is not None
        S = np.hstack([X, W, P] if have_p else [X, W])
        AS = np.hstack([AX, AW, AP] if have_p else [AX, AW])
        BS = np.hstack([BX, W if wrong == "w_not_b" else BW, BP] if have_p else [BX, W if wrong == "w_not_b" else BW])
        GA, GB = S.T @ AS, S.T @ BS
        status, C, th = rayleigh_ritz(GA, GB, m)
        if status == 1 and have_p and wrong != "keep_p":
            have_p = False
            restarts += 1
            status, C, th = rayleigh_ritz(GA[:2 * m, :2 * m], GB[:2 * m, :2 * m], m)
        if status:
            reason = DIVERGED_NAN if status == 2 else DIVERGED_BREAKDOWN
            break
        CX, CWP = C[:m], C[m:]
        WP, AWP, BWP = (np.hstack([W, P]), np.hstack([AW, AP]), np.hstack([BW, BP])) if have_p else (W, AW, BW)
        P, AP, BP = WP @ CWP, AWP @ CWP, BWP @ CWP
        X, AX, BX = X @ CX + P, AX @ CX + AP, BX @ CX + BP
        stale, theta = theta, th
        its += 1
    return dict(X=X, lam=theta.copy(), resid=rn.copy(), iterations=its, reason=reason, nconverged=nconv, restarts=restarts, actions=actions[0],
                history=np.array(hist).reshape(-1, m))


def dense_reference(A, B, free, k):
    """(the k lowest eigenvalues, their B-orthonormal vectors [n, k]) of the pencil on the free rows, by scipy.linalg.eigh"""
    A = np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)
    idx = np.flatnonzero(free)
    Af = A[np.ix_(idx, idx)]
    if B is None:
        lam, U = sla.eigh(0.5 * (Af + Af.T))
    else:
        B = np.asarray(B.todense()) if hasattr(B, "todense") else np.asarray(B)
        Bf = B[np.ix_(idx, idx)]
        lam, U = sla.eigh(0.5 * (Af + Af.T), 0.5 * (Bf + Bf.T))
    V = np.zeros((A.shape[0], k))
    V[idx, :] = U[:, :k]
    return lam[:k], V


def parlett_bounds(A, B, free, X, lam):
    """|B^-1/2 r_k| / |B^1/2 x_k| for r_k = A x_k - lam_k B x_k on the free rows: for a definite pencil some eigenvalue lies within that
    distance of lam_k (Parlett, The Symmetric Eigenvalue Problem, 15.9); in sorted order where the cut falls in a spectral gap.
    Also returns |r_k|_2, the residual norms the solve reports."""
    idx = np.flatnonzero(free)
    out, norms = [], []
    Bf = None
    if B is not None:
        Bd = np.asarray(B.todense()) if hasattr(B, "todense") else np.asarray(B)
        Bf = Bd[np.ix_(idx, idx)]
        L = np.linalg.cholesky(0.5 * (Bf + Bf.T))
    for k in range(X.shape[1]):
        x = X[:, k]
        bx = x if B is None else np.asarray(B @ x).ravel()
        r = (np.asarray(A @ x).ravel() - lam[k] * bx)[idx]
        norms.append(np.linalg.norm(r))
        if B is None:
            out.append(np.linalg.norm(r) / np.linalg.norm(x[idx]))
        else:
            y = sla.solve_triangular(L, r, lower=True)      # |B^-1/2 r|^2 = r^T B^-1 r = |L^-1 r|^2
            out.append(np.linalg.norm(y) / np.sqrt(x[idx] @ (Bf @ x[idx])))
    return np.array(out), np.array(norms)


def orthonormality_defect(B, X):
    """max |X^T B X - I|"""
    BX = X if B is None else np.asarray(B @ X)
    return float(np.abs(X.T @ BX - np.eye(X.shape[1])).max())


def largest_principal_angle(B, U, V):
    """between span U and span V (same number of B-orthonormal columns), in the B inner product, by its SINE -- the largest singular value
    of (I - V V^T B) U in the B norm -- because the cosine of a small angle rounds to 1: acos cannot see an angle below 1e-8"""
    BU = U if B is None else np.asarray(B @ U)
    D = U - V @ (V.T @ BU)
    BD = D if B is None else np.asarray(B @ D)
    G = D.T @ BD
    s2 = np.linalg.eigvalsh(0.5 * (G + G.T)).max()
    return float(np.arcsin(min(1.0, np.sqrt(max(s2, 0.0)))))
