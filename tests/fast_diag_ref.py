"""numpy / scipy restatement of fast diagonalisation (Sangalli and Tani 2016), independent of the library: the 1-D mass and stiffness
matrices from the knots (scipy.interpolate.BSpline, numpy's Gauss-Legendre rule), scipy.linalg.eigh for the generalised eigenpairs,
einsum for the six contractions.  Nodes are ordered with axis 0 fastest, fields interleaved: index = node * dof + field."""
import numpy as np
import scipy.linalg as sla
from scipy.interpolate import BSpline


def axis_functions(U, p, periodic):
    """(number of global functions nnp, list of (span index k, u0, u1)): element k carries the functions k - p .. k, wrapped modulo nnp"""
    U = np.asarray(U, dtype=float)
    m = len(U) - 1
    n = m - p - 1
    spans = [(k, U[k], U[k + 1]) for k in range(p, n + 1) if U[k + 1] > U[k]]
    nnp = n + 1
    if periodic:
        s = int(np.sum(U[n + 1:] == U[n + 1]))
        nnp = n - (p - s)
    return nnp, spans


def axis_matrices(U, p, nqp=None, periodic=False):
    """M[i, j] = int N_i N_j, K[i, j] = int N_i' N_j' over the axis, by the Gauss-Legendre rule with nqp points per element (default p + 1);
    count[i] = number of elements that hold function i"""
    U = np.asarray(U, dtype=float)
    nqp = p + 1 if nqp is None else nqp
    nnp, spans = axis_functions(U, p, periodic)
    nfun = len(U) - p - 1
    B = BSpline(U, np.eye(nfun), p, extrapolate=False)
    dB = B.derivative()
    x, w = np.polynomial.legendre.leggauss(nqp)
    M, K, count = np.zeros((nnp, nnp)), np.zeros((nnp, nnp)), np.zeros(nnp)
    for k, u0, u1 in spans:
        J = (u1 - u0) / 2
        pts = (x + 1) * J + u0
        idx = np.arange(k - p, k + 1)
        N, dN = B(pts)[:, idx], dB(pts)[:, idx]
        g = idx % nnp
        np.add.at(count, g, 1.0)
        np.add.at(M, (g[:, None], g[None, :]), np.einsum("q,qa,qb->ab", w * J, N, N))
        np.add.at(K, (g[:, None], g[None, :]), np.einsum("q,qa,qb->ab", w * J, dN, dN))
    return M, K, count


class FastDiagRef:
    """Z = P R as the library defines it.  axes: [(M, K, count)] * 3; fixed[d][side]: set of fields fixed on that face."""

    def __init__(self, axes, dof, fixed, alpha, beta, zero_tol=1e-12):
        self.axes, self.dof, self.alpha, self.beta = axes, dof, alpha, beta
        self.n = [a[0].shape[0] for a in axes]
        self.rng, self.eig = [], []
        for f in range(dof):
            rng, eig = [], []
            for d in range(3):
                lo, hi = int(f in fixed[d][0]), int(f in fixed[d][1])
                sl = slice(lo, self.n[d] - hi)
                lam, V = sla.eigh(axes[d][1][sl, sl], axes[d][0][sl, sl])
                rng.append(sl)
                eig.append((lam, V))
            self.rng.append(rng)
            self.eig.append(eig)
        dens = [self.denominators(f) for f in range(dof)]
        dmax = max(np.abs(d).max() for d in dens)
        self.recip, self.nzeroed = [], 0
        for den in dens:
            zero = np.abs(den) <= zero_tol * dmax
            self.nzeroed += int(zero.sum())
            self.recip.append(np.where(zero, 0.0, 1.0 / np.where(zero, 1.0, den)))

    def denominators(self, f):
        (l0, _), (l1, _), (l2, _) = self.eig[f]
        return self.alpha + self.beta[2] * l2[:, None, None] + self.beta[1] * l1[None, :, None] + self.beta[0] * l0[None, None, :]

    def count(self):
        return self.axes[2][2][:, None, None] * self.axes[1][2][None, :, None] * self.axes[0][2][None, None, :]

    def free_mask(self):
        """[n2, n1, n0, dof] True on the free dofs"""
        mask = np.zeros(self.n[::-1] + [self.dof], dtype=bool)
        for f in range(self.dof):
            r0, r1, r2 = self.rng[f]
            mask[r2, r1, r0, f] = True
        return mask.reshape(-1)

    def apply(self, R):
        R = np.asarray(R, dtype=float).reshape(self.n[::-1] + [self.dof])
        Z = R / self.count()[..., None]
        for f in range(self.dof):
            r0, r1, r2 = self.rng[f]
            (_, V0), (_, V1), (_, V2) = self.eig[f]
            T = np.einsum("kji,kc,jb,ia->cba", R[r2, r1, r0, f], V2, V1, V0, optimize=True) * self.recip[f]
            Z[r2, r1, r0, f] = np.einsum("cba,kc,jb,ia->kji", T, V2, V1, V0, optimize=True)
        return Z.reshape(-1)


def fixed_faces(dof, faces):
    """faces: iterable of (axis, side, field) -> fixed[d][side] = set of fields"""
    fixed = [[set(), set()] for _ in range(3)]
    for d, s, f in faces:
        fixed[d][s].add(f)
    return fixed


def pcg(op, prec, b, rtol=1e-10, maxit=None):
    """preconditioned CG, the loop of tests/test_gpu_matrix_diagonal.py with the stop criterion |r| <= rtol |b|; returns (x, iterations)"""
    x = np.zeros_like(b)
    r = b - op(x)
    z = prec(r)
    p = z.copy()
    rz, norm0, its = r @ z, np.linalg.norm(b), 0
    maxit = b.size if maxit is None else maxit
    while np.linalg.norm(r) > rtol * norm0 and its < maxit:
        Ap = op(p)
        a = rz / (p @ Ap)
        x += a * p
        r -= a * Ap
        z = prec(r)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        its += 1
    return x, its
