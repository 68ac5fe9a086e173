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


def axis_count(U, p, periodic=False):
    """count[i] = number of elements that hold function i (axis_matrices' third result, without the matrices)"""
    nnp, spans = axis_functions(U, p, periodic)
    count = np.zeros(nnp)
    for k, _, _ in spans:
        np.add.at(count, np.arange(k - p, k + 1) % nnp, 1.0)
    return count


U_ROUND = 2.0 ** -53


class ExactApplyRef:
    """Z = P R evaluated from the engine's OWN tables, so that the device half is judged apart from the host eigen-solver.
    tables[f][d] = (first, m, Lambda [m], U [m, m]) as IGXFastDiagGetAxis hands them back; counts[d] = elements per function.
    What the engine fixes in double is formed in double, in its order: s_d = beta_d Lambda_d, the denominators ((alpha + s0) + s1) + s2,
    thresh = 1e-12 dmax with dmax = max over the fields of ((alpha + max|s0|) + max|s1|) + max|s2|; a mode with |den| <= thresh is zeroed.
    Everything else -- three forward contractions, the reciprocal of the double denominator, three backward contractions, R / count in the
    fixed rows -- runs in np.longdouble.  apply() returns (Z_ref, S), both [n2 n1 n0 dof] flat; S is the same chain on |R|, |U|, |1 / den|:
    the sum of the absolute values of all terms of an entry."""

    def __init__(self, tables, n, dof, counts, alpha, beta):
        self.tables, self.n, self.dof, self.counts, self.alpha, self.beta = tables, list(n), dof, counts, float(alpha), [float(b) for b in beta]
        self.s = [[np.float64(self.beta[d]) * np.asarray(tables[f][d][2], dtype=np.float64) for d in range(3)] for f in range(dof)]
        dmax = 0.0
        for f in range(dof):
            v = np.float64(self.alpha)
            for d in range(3):
                v = v + (np.abs(self.s[f][d]).max() if self.s[f][d].size else 0.0)
            dmax = max(dmax, float(v))
        self.thresh = 1e-12 * dmax
        self.recip, self.nzeroed = [], 0
        for f in range(dof):
            s0, s1, s2 = self.s[f]
            den = ((np.float64(self.alpha) + s0[None, None, :]) + s1[None, :, None]) + s2[:, None, None]
            zero = np.abs(den) <= self.thresh
            self.nzeroed += int(zero.sum())
            self.recip.append(np.where(zero, np.longdouble(0), np.longdouble(1) / np.where(zero, 1.0, den).astype(np.longdouble)))

    def free_mask(self):
        mask = np.zeros(self.n[::-1] + [self.dof], dtype=bool)
        for f in range(self.dof):
            (a0, m0, _, _), (a1, m1, _, _), (a2, m2, _, _) = self.tables[f]
            mask[a2:a2 + m2, a1:a1 + m1, a0:a0 + m0, f] = True
        return mask.reshape(-1)

    @staticmethod
    def _chain(A, mats, recip):
        """[k2, k1, k0] -> modes -> nodes; mats = (U0, U1, U2) with U[node, mode]; grid axis d is numpy axis 2 - d"""
        for d in range(3):
            A = np.moveaxis(np.tensordot(A, mats[d], axes=([2 - d], [0])), -1, 2 - d)
        A = A * recip
        for d in (2, 1, 0):
            A = np.moveaxis(np.tensordot(A, mats[d], axes=([2 - d], [1])), -1, 2 - d)
        return A

    def apply(self, R):
        ld = np.longdouble
        R = np.asarray(R, dtype=np.float64).reshape(self.n[::-1] + [self.dof]).astype(ld)
        c0, c1, c2 = (np.asarray(c, dtype=ld) for c in self.counts)
        count = (c2[:, None, None] * c1[None, :, None] * c0[None, None, :])[..., None]
        Z, S = R / count, np.abs(R) / count
        for f in range(self.dof):
            (a0, m0, _, U0), (a1, m1, _, U1), (a2, m2, _, U2) = self.tables[f]
            if m0 * m1 * m2 == 0:
                continue
            box = (slice(a2, a2 + m2), slice(a1, a1 + m1), slice(a0, a0 + m0), f)
            mats = [np.asarray(U, dtype=np.float64).astype(ld) for U in (U0, U1, U2)]
            Z[box] = self._chain(R[box], mats, self.recip[f])
            S[box] = self._chain(np.abs(R[box]), [np.abs(U) for U in mats], np.abs(self.recip[f]))
        return Z.reshape(-1), S.reshape(-1)

    def rounding_constant(self):
        """c of |Z - Z_ref| <= c u S / (1 - c u): a contraction of length m on FMA hardware commits at most m roundings per entry (six
        contractions: 2 (n0 + n1 + n2)), the double denominator, its reciprocal and the scaling at most 8 more; any summation order"""
        return 2 * sum(self.n) + 8

    def ratio(self, Z, Z_ref, S):
        """worst |Z - Z_ref| / (u S) over the entries with S > 0, and whether Z is exactly 0 wherever S = 0"""
        Z = np.asarray(Z, dtype=np.float64).astype(np.longdouble)
        pos = S > 0
        r = float((np.abs(Z - Z_ref)[pos] / (U_ROUND * S[pos])).max()) if pos.any() else 0.0
        return r, bool(np.all(Z[~pos] == 0))

    def holds(self, Z, Z_ref, S):
        c = self.rounding_constant()
        r, zeros = self.ratio(Z, Z_ref, S)
        return zeros and r <= c / (1 - c * U_ROUND)


def engine_tables(eng, dof):
    return [[eng.fast_diag_get_axis(d, f) for d in range(3)] for f in range(dof)]


def uniform_knots(p, N, periodic=False):
    """the knot vector IGAAxisInitUniform makes on [0, 1] with continuity p - 1"""
    m = 2 * (p + 1) + (N - 1) - 1
    n = m - p - 1
    U = np.zeros(m + 1)
    U[m - p:] = 1.0
    U[p + 1:p + N] = np.arange(1, N) / N
    if periodic:
        C = p - 1
        for k in range(C + 1):
            U[C - k] = U[p] - U[m - p] + U[n - k]
            U[m - C + k] = U[m - p] - U[p] + U[p + 1 + k]
    return U


def exact_case(p, N, dof=1, faces=(), alpha=0.0, beta=(1.0, 1.0, 1.0), periodic=(False, False, False), knots=(None, None, None), nqp=(None, None, None)):
    """(engine after IGXFastDiagSetUp, ExactApplyRef of its tables, the nzeroed SetUp returned); host work only.
    faces: (axis, side, field); knots[d]: a knot vector in place of the uniform one of N[d] elements."""
    import petiga_amd as P
    eng = P.IGX(3, dof)
    counts = []
    for d in range(3):
        U = uniform_knots(p[d], N[d], periodic[d]) if knots[d] is None else np.asarray(knots[d], dtype=float)
        eng.axis_knots(d, p[d], U, periodic=periodic[d])
        if nqp[d]:
            eng.set_quadrature(d, nqp[d])
        counts.append(axis_count(U, p[d], periodic[d]))
    eng.setup()
    for d, s, f in faces:
        eng.set_boundary_value(d, s, f, 0.0)
    nz = eng.fast_diag_setup(alpha, list(beta))
    n = eng.sizes()["node_sizes"]
    assert [len(c) for c in counts] == list(n)
    return eng, ExactApplyRef(engine_tables(eng, dof), n, dof, counts, alpha, beta), nz


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
