"""A long double reference that evaluates AT THE QUADRATURE POINTS, for the passes whose coefficient depends on a state that varies.

tensor_ref.py covers the forms that are sums of Kronecker products of 1-D matrices; a coefficient such as lambda e^u(q) at a varying
state is not one.  Here the 1-D ingredients are dense collocation tables B[r][q, a] (value, first and second derivative of global basis
function a at global point q, from the points, weights and Jacobians the kernels use), and every quantity is built from three
operations on them: at() interpolates a field or one of its derivatives at all points, test() sums a point field against every test
function, pair_entries() sums it against pairs of them.  No element loop and no element-local numbering: a kernel that reads another
lane's, point's or element's interpolated state does not agree with it.

The bound S is the same sums with every factor replaced by its absolute value, every interpolated quantity by its abs-sum
(sum_b |N_b| |U_b|), and a coefficient that depends nonlinearly on the state by |coefficient| plus its first-order sensitivity times the
state's abs-sum (e^u -> e^u (1 + uabs)): S bounds any order of summation, it is not fitted to an implementation.  The comparison is
that of tensor_ref.py: |E - R| <= c u S, with c = C_ID on the identity geometry and C_MAP on an affine map
(test_pointwise_reference.py calibrates both on the CPU oracle).  3-D, one field; identity geometry or an affine map x = A g + b
(constant NURBS weights included: the rational basis is then the B-spline basis); curved_ref.py is the same reference on a general
NURBS map, where the Jacobian, the map's second derivatives and W vary from point to point.

Dirichlet semantics are TensorRef's (fixed / multiplicity, the last face wins): the state takes the boundary value at a fixed node, the
direction X and the rate V take 0 there; a fixed Function row is m (U - v), a fixed action row m X (S = m |X|: a kernel that adds X
once per element rounds it), a fixed matrix row the exact integer m on the diagonal.
"""
import numpy as np

import tensor_ref as T

LD = T.LD
Z = (0, 0, 0)
E1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
E2 = [(2, 0, 0), (0, 2, 0), (0, 0, 2)]


def collocation(axis, basis, evaluate=T.bspline_1d_d2):
    """(B [3, nel * nqp, nnp], w [nel * nqp]) of one axis: B[r][q, a] the r-th derivative of global function a at global point q
    (indices wrapped on a periodic axis), w[q] = weight * detJac."""
    nel, nen, nqp, nnp = basis["nel"], basis["nen"], basis["nqp"], axis["nnp"]
    B = np.zeros((3, nel * nqp, nnp), dtype=LD)
    w = np.zeros(nel * nqp, dtype=LD)
    for e in range(nel):
        idx = (basis["offset"][e] + np.arange(nen)) % nnp
        Ns = evaluate(axis["U"], axis["p"], int(axis["span"][e]), basis["point"][e])
        q = slice(e * nqp, (e + 1) * nqp)
        for r in range(3):
            for a in range(nen):
                B[r, q, idx[a]] += Ns[r][:, a]
        w[q] = np.asarray(basis["weight"][e], dtype=LD) * LD(basis["detJac"][e])
    return B, w


class PointwiseRef:
    """orc: the oracle of the discretisation (3-D, dof = 1); A: the affine map's matrix (None: identity); bcs: {(axis, side, 0): value}."""

    def __init__(self, orc, A=None, bcs=None):
        assert orc.dim == 3 and orc.dof == 1
        self.tref = T.reference(orc, 3, T.poisson(3), A=A, bcs=bcs, driver="system")       # index helpers, fix-up, the grad-grad part
        self.B, self.w = zip(*[collocation(orc.axis(i), orc.basis(i)) for i in range(3)])
        self.n = [b.shape[2] for b in self.B]
        self.size = int(np.prod(self.n))
        self.W = np.einsum("k,j,i->kji", self.w[2], self.w[1], self.w[0])
        if A is None:
            Ainv, det = np.eye(3), 1.0
        else:
            Ainv, det = np.linalg.inv(np.asarray(A, dtype=float)), float(np.linalg.det(A))
        self.det, self.deta = LD(det), LD(abs(det))
        self.G = Ainv @ Ainv.T * det                        # parametric coefficient of d_k N_a d_l u: TensorRef.K of Poisson
        self.Ga = np.abs(Ainv) @ np.abs(Ainv).T * abs(det)
        self.mapped = A is not None
        idx = np.arange(self.size)
        self.fx, self.v = self.tref.fixed(idx) if bcs else (np.zeros(self.size, dtype=bool), np.zeros(self.size))
        self.mult = self.tref.multiplicity(idx)

    # -- the three operations
    def _tabs(self, r, absolute):
        return [np.abs(self.B[d][r[d]]) if absolute else self.B[d][r[d]] for d in range(3)]

    def at(self, U, r, absolute=False):
        """[q2, q1, q0]: the derivative of per-axis orders r of the field U (axis 0 fastest) at all points; absolute: sum |B| |U|."""
        B = self._tabs(r, absolute)
        Ug = np.asarray(U, dtype=LD).reshape(self.n[2], self.n[1], self.n[0])
        if absolute:
            Ug = np.abs(Ug)
        t = np.einsum("ia,cba->cbi", B[0], Ug)
        t = np.einsum("jb,cbi->cji", B[1], t)
        return np.einsum("kc,cji->kji", B[2], t)

    def test(self, G, r, absolute=False):
        """[n]: sum_q G_q N^(r)_a(q) for every node a (the point field G already carries its weights)."""
        B = self._tabs(r, absolute)
        t = np.einsum("ia,kji->kja", B[0], np.asarray(G, dtype=LD))
        t = np.einsum("jb,kja->kba", B[1], t)
        return np.einsum("kc,kba->cba", B[2], t).reshape(-1)

    def pair_tensor(self, G, r, s, absolute=False):
        """[i2, j2, i1, j1, i0, j0]: sum_q G_q N^(r)_i(q) N^(s)_j(q)."""
        Br, Bs = self._tabs(r, absolute), self._tabs(s, absolute)
        t = np.einsum("qa,qb,kjq->kjab", Br[0], Bs[0], np.asarray(G, dtype=LD))
        t = np.einsum("qa,qb,kqcd->kabcd", Br[1], Bs[1], t)
        return np.einsum("qa,qb,qcdef->abcdef", Br[2], Bs[2], t)

    def pair_entries(self, G, r, s, rows, cols, absolute=False):
        """sum_q G_q N^(r)_i(q) N^(s)_j(q) at the global (row, col) pairs."""
        ti, _ = self.tref.split(rows)
        tj, _ = self.tref.split(cols)
        return self.pair_tensor(G, r, s, absolute)[ti[2], tj[2], ti[1], tj[1], ti[0], tj[0]]

    # -- Dirichlet
    def _state(self, U):
        return np.where(self.fx, self.v, np.asarray(U, dtype=np.float64))

    def _direction(self, X):
        return np.where(self.fx, 0.0, np.asarray(X, dtype=np.float64))

    def _fix_function(self, R, S, U):
        fx = self.fx
        R[fx] = self.mult[fx] * (LD(1) * np.asarray(U)[fx] - LD(1) * self.v[fx])
        S[fx] = self.mult[fx] * (np.abs(np.asarray(U)[fx]) + np.abs(self.v[fx]))
        return R, S

    def _fix_action(self, R, S, X):
        fx = self.fx
        R[fx] = self.mult[fx] * (LD(1) * np.asarray(X)[fx])
        S[fx] = self.mult[fx] * np.abs(np.asarray(X)[fx])
        return R, S

    def _gradgrad(self, D):
        """sum_q W G[k, l] d_k N_a d_l D and its bound, for a field D."""
        R, S = np.zeros(self.size, dtype=LD), np.zeros(self.size, dtype=LD)
        for k in range(3):
            for l in range(3):
                if self.Ga[k, l] == 0:
                    continue
                R += LD(self.G[k, l]) * self.test(self.W * self.at(D, E1[l]), E1[k])
                S += LD(self.Ga[k, l]) * self.test(self.W * self.at(D, E1[l], True), E1[k], True)
        return R, S

    # -- Bratu (oracle/igaforms.c: orc_form_bratu_*)
    def _bratu_exp(self, lam, Uf):
        """(lambda e^u det, its bound lambda e^u (1 + uabs) |det|) at the points."""
        u, ua = self.at(Uf, Z), self.at(Uf, Z, True)
        eu = LD(lam) * np.exp(u)
        return eu * self.det, np.abs(eu) * (1 + ua) * self.deta

    def bratu_function(self, lam, U, V=None):
        """(R, S) of every row of the Function (V None) or IFunction: F_a = [N_a v] + grad N_a . grad u - N_a lambda e^u."""
        Uf = self._state(U)
        eu, eua = self._bratu_exp(lam, Uf)
        R, S = self._gradgrad(Uf)
        R -= self.test(self.W * eu, Z)
        S += self.test(self.W * eua, Z, True)
        if V is not None:
            Vf = self._direction(V)
            R += self.test(self.W * self.det * self.at(Vf, Z), Z)
            S += self.test(self.W * self.deta * self.at(Vf, Z, True), Z, True)
        return self._fix_function(R, S, U)

    def bratu_action(self, lam, U, X, shift=0.0):
        """(R, S) of every row of the (I)Jacobian at the state U times X."""
        Uf, Xf = self._state(U), self._direction(X)
        eu, eua = self._bratu_exp(lam, Uf)
        R, S = self._gradgrad(Xf)
        R += self.test(self.W * (LD(shift) * self.det - eu) * self.at(Xf, Z), Z)
        S += self.test(self.W * (abs(LD(shift)) * self.deta + eua) * self.at(Xf, Z, True), Z, True)
        return self._fix_action(R, S, X)

    def bratu_entries(self, lam, U, rows, cols, shift=0.0, permute=None):
        """(R, S) of the (I)Jacobian at the state U at the global entries: the grad-grad part from TensorRef, the mass part from
        pair_entries with G = W (shift - lambda e^u).  permute: a map of the point field lambda e^u (the teeth test's wrong kernel)."""
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        eu, eua = self._bratu_exp(lam, self._state(U))
        if permute is not None:
            eu = permute(eu)
        R, S = self.tref._tensor(rows, cols)
        R = R + self.pair_entries(self.W * (LD(shift) * self.det - eu), Z, Z, rows, cols)
        S = S + self.pair_entries(self.W * (abs(LD(shift)) * self.deta + eua), Z, Z, rows, cols, True)
        fr, fc = self.fx[rows], self.fx[cols]
        R[fc & ~fr] = 0
        S[fc & ~fr] = 0
        R[fr] = np.where(rows[fr] == cols[fr], self.mult[rows[fr]], 0)
        S[fr] = 0
        return R, S

    # -- Cahn-Hilliard (orc_form_ch_residual / orc_form_ch_tangent), identity geometry
    def _ch(self, ctx, Uf):
        """The coefficients at the points and the absolute sums their bounds need.  ctx: (theta, alpha, cbar, L0, lambda, tau)."""
        assert not self.mapped, "Cahn-Hilliard: identity geometry only here; curved_ref.CurvedRef has it on a mapped geometry, the map's Hessian included"
        theta, alpha, _, L0, lam, _ = ctx
        scale = LD(L0) * LD(L0) / LD(lam) if L0 > 0 else 3 * LD(alpha)
        h = LD(0.5) / LD(theta)
        c, ca = self.at(Uf, Z), self.at(Uf, Z, True)
        g = 1 / (c * (1 - c))
        k = dict(c=c, ca=ca, M=c * (1 - c), dM=1 - 2 * c)
        k["dmu"] = (h * g - 2) * scale
        k["d2mu"] = -h * (1 - 2 * c) * g * g * scale
        d3mu = h * (2 * g * g + 2 * (1 - 2 * c) ** 2 * g ** 3) * scale
        k["lap"] = sum(self.at(Uf, e) for e in E2)
        k["lapa"] = sum(self.at(Uf, e, True) for e in E2)
        M, dM, dmu, d2mu, lapa = k["M"], k["dM"], k["dmu"], k["d2mu"], k["lapa"]
        # |d/dc| of M dmu, term by term, and of dM dmu + M d2mu
        k["sMdmu"] = np.abs(dM * dmu) + np.abs(M * d2mu)
        k["sk2"] = 2 * np.abs(dmu) + 2 * np.abs(dM * d2mu) + np.abs(M * d3mu)
        k["t1"] = M * dmu + dM * k["lap"]
        k["t1a"] = np.abs(M * dmu) + np.abs(dM) * lapa + (k["sMdmu"] + 2 * lapa) * ca
        k["Ma"] = np.abs(M) + np.abs(dM) * ca
        k["dMa"] = np.abs(dM) + 2 * ca
        return k

    def ch_ifunction(self, ctx, U, V):
        """(R, S) of every row of the IFunction: R_a = N_a c_t + grad N_a . (M dmu + dM lap c) grad c + lap N_a M lap c."""
        Uf, Vf = self._state(U), self._direction(V)
        k = self._ch(ctx, Uf)
        W = self.W
        R = self.test(W * self.at(Vf, Z), Z)
        S = self.test(W * self.at(Vf, Z, True), Z, True)
        for e in E1:
            R += self.test(W * k["t1"] * self.at(Uf, e), e)
            S += self.test(W * k["t1a"] * self.at(Uf, e, True), e, True)
        for e in E2:
            R += self.test(W * k["M"] * k["lap"], e)
            S += self.test(W * k["Ma"] * k["lapa"], e, True)
        return self._fix_function(R, S, U)

    def ch_action(self, ctx, shift, U, X):
        """(R, S) of every row of the IJacobian (the Tangent) at the state U times X."""
        Uf, Xf = self._state(U), self._direction(X)
        k = self._ch(ctx, Uf)
        W, M, dM, dmu, d2mu, lap, lapa, ca = self.W, k["M"], k["dM"], k["dmu"], k["d2mu"], k["lap"], k["lapa"], k["ca"]
        x, xa = self.at(Xf, Z), self.at(Xf, Z, True)
        lx = sum(self.at(Xf, e) for e in E2)
        lxa = sum(self.at(Xf, e, True) for e in E2)
        k2 = dM * dmu + M * d2mu - 2 * lap
        k2a = k["sMdmu"] + 2 * lapa + k["sk2"] * ca
        t2 = k2 * x + dM * lx
        t2a = k2a * xa + k["dMa"] * lxa
        R = self.test(W * LD(shift) * x, Z)
        S = self.test(W * abs(LD(shift)) * xa, Z, True)
        for e in E1:
            R += self.test(W * (k["t1"] * self.at(Xf, e) + t2 * self.at(Uf, e)), e)
            S += self.test(W * (k["t1a"] * self.at(Xf, e, True) + t2a * self.at(Uf, e, True)), e, True)
        for e in E2:
            R += self.test(W * (dM * lap * x + M * lx), e)
            S += self.test(W * (k["dMa"] * lapa * xa + k["Ma"] * lxa), e, True)
        return self._fix_action(R, S, X)


def compare_rows(Y, R, S, c, ref=None, what="vector"):
    """compare_entrywise for a whole vector: every row, |Y_i - R_i| <= c u S_i."""
    Y = np.asarray(Y)
    assert Y.shape == R.shape == S.shape, (Y.shape, R.shape, S.shape)
    return T.compare_entrywise((np.arange(Y.size), Y), R, S, c, ref, what)


def colouring(tabs, dof=1):
    """Colours of the global columns such that no row couples with two columns of one colour: each axis's nodes coloured greedily on
    couple @ couple (two nodes conflict when one row couples with both), the product over the axes, times dof.
    Returns (colour of every global index, number of colours, colours per axis)."""
    cols, counts = [], []
    for t in tabs:
        cp = t.couple.astype(np.int64)
        conflict = (cp @ cp.T) > 0
        col = -np.ones(t.nnp, dtype=np.int64)
        for a in range(t.nnp):
            used = set(col[np.flatnonzero(conflict[a])].tolist())
            k = 0
            while k in used:
                k += 1
            col[a] = k
        cols.append(col)
        counts.append(int(col.max()) + 1)
    # colour of node (i0, i1, i2) = c0[i0] + n0c * (c1[i1] + n1c * c2[i2]), axis 0 fastest
    grid = np.zeros([len(c) for c in cols[::-1]], dtype=np.int64)
    stride = 1
    for d, (col, cnt) in enumerate(zip(cols, counts)):
        shape = [1] * len(cols)
        shape[len(cols) - 1 - d] = len(col)
        grid = grid + stride * col.reshape(shape)
        stride *= cnt
    colour = (grid.reshape(-1)[:, None] * dof + np.arange(dof)[None, :]).reshape(-1)
    return colour, stride * dof, counts
