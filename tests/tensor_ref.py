"""An entry-wise reference for the forms that are sums of Kronecker products of 1-D matrices.

On the identity geometry and on an affine map X = A u + b every built-in form the engine assembles at a constant state (Poisson,
Poisson_f, mass, elasticity, elasticity_f, Bratu at U = c) integrates, term by term, a product of one 1-D factor per axis: the element
set is a Cartesian product and every quadrature term factorises.  So is the sum of the ABSOLUTE values of the terms, S: any order of
summing the same products -- sum-factorised phases, MFMA accumulation trees, LDS adds -- stays within a small multiple of u*S of the
exact value (u = 2^-53).  This module evaluates, at arbitrary global (row, col) pairs, the exact value R of the discrete operation (the
1-D tables in long double, from the points, weights and Jacobians the kernels use) and the bound S, and compares a matrix with them
entry by entry: |E - R| <= c * u * S, with S = 0 meaning exactly zero.  On a curved map no term factorises: curved_ref.py evaluates
the same forms at the quadrature points of a general NURBS geometry.

Indices are the engine's global natural numbering: node * dof + field, node = i0 + n0 * (i1 + n1 * i2) (axis 0 fastest).
"""
import numpy as np

U_RND = 2.0 ** -53
# c of |E - R| <= c u S: 4x the worst ratio of the CPU oracle (test_tensor_reference.py), rounded up to a power of two
C_ID = 128
C_MAP = 256
LD = np.longdouble


def bspline_1d(U, p, k, x, dtype=LD):
    """Cox-de Boor in long double (dtype=object: in the arithmetic of the given objects, Fractions say): values and first derivatives
    of the p + 1 functions of span k at the points x -> two [nx, p+1]."""
    U = np.asarray(U, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    N = [np.ones_like(x)]
    for d in range(1, p + 1):
        old, N = N, []
        for j in range(d + 1):
            i = k - d + j
            t = np.zeros_like(x)
            if j > 0 and U[i + d] != U[i]:
                t = t + (x - U[i]) / (U[i + d] - U[i]) * old[j - 1]
            if j < d and U[i + d + 1] != U[i + 1]:
                t = t + (U[i + d + 1] - x) / (U[i + d + 1] - U[i + 1]) * old[j]
            N.append(t)
        if d == p:
            dN = []
            for j in range(p + 1):
                i = k - p + j
                t = np.zeros_like(x)
                if p > 0 and j > 0 and U[i + p] != U[i]:
                    t = t + p * old[j - 1] / (U[i + p] - U[i])
                if p > 0 and j < p and U[i + p + 1] != U[i + 1]:
                    t = t - p * old[j] / (U[i + p + 1] - U[i + 1])
                dN.append(t)
    if p == 0:
        dN = [np.zeros_like(x)]
    return np.stack(N, axis=-1), np.stack(dN, axis=-1)


def bspline_1d_d2(U, p, k, x, dtype=LD):
    """bspline_1d with the second derivatives: the derivative recurrence applied to the first derivatives of the p functions of
    degree p - 1 on the same span -> three [nx, p+1]."""
    N0, N1 = bspline_1d(U, p, k, x, dtype)
    U = np.asarray(U, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    if p < 2:
        return N0, N1, np.zeros_like(N0)
    _, L1 = bspline_1d(U, p - 1, k, x, dtype)               # function j of degree p - 1 on span k has knot index k - p + 1 + j
    N2 = []
    for j in range(p + 1):
        i = k - p + j
        t = np.zeros_like(x)
        if j > 0 and U[i + p] != U[i]:
            t = t + p * L1[:, j - 1] / (U[i + p] - U[i])
        if j < p and U[i + p + 1] != U[i + 1]:
            t = t - p * L1[:, j] / (U[i + p + 1] - U[i + 1])
        N2.append(t)
    return N0, N1, np.stack(N2, axis=-1)


class AxisTables:
    """The assembled 1-D tables of one axis over the elements [e0, e1) (a rank's box), node indices wrapped on a periodic axis.
    axis / basis: the dicts of OracleIGA.axis(i) / .basis(i) -- the doubles (points, weights, Jacobians) the kernels use."""

    def __init__(self, axis, basis, e0=0, e1=None, evaluate=bspline_1d):
        p, U, nnp, per = axis["p"], axis["U"], axis["nnp"], axis["periodic"]
        nel, nen = basis["nel"], basis["nen"]
        e1 = nel if e1 is None else e1
        self.p, self.nnp, self.periodic, self.nel, self.e0, self.e1 = p, nnp, per, nel, e0, e1
        self.P = np.zeros((2, 2, nnp, nnp), dtype=LD)          # P[r, s][a, b] = sum_e sum_q wJ N^(r)_a N^(s)_b
        self.Pabs = np.zeros_like(self.P)
        self.I0 = np.zeros(nnp, dtype=LD)                       # integral of N_a
        self.I1abs = np.zeros(nnp, dtype=LD)                    # integral of |N'_a|
        self.T01 = np.zeros(nnp, dtype=LD)                      # integral of N_a * sum_b |N'_b|
        self.T11 = np.zeros(nnp, dtype=LD)                      # integral of |N'_a| * sum_b |N'_b|
        self.count = np.zeros(nnp, dtype=np.int64)              # elements of the range on which N_a is supported
        self.area = np.zeros(nnp, dtype=LD)                     # sum of 2 detJac / nen over those elements (a boundary load's face area)
        self.couple = np.zeros((nnp, nnp), dtype=bool)          # 1-D coupling over the WHOLE axis (the matrix pattern)
        for e in range(nel):
            idx = (basis["offset"][e] + np.arange(nen)) % nnp
            self.couple[np.ix_(idx, idx)] = True
            if not e0 <= e < e1:
                continue
            k = int(axis["span"][e])
            N0, N1 = evaluate(U, p, k, basis["point"][e])
            wJ = np.asarray(basis["weight"][e], dtype=LD) * LD(basis["detJac"][e])
            Ns = (N0, N1)
            for r in range(2):
                for s in range(2):
                    blk = np.einsum("q,qa,qb->ab", wJ, Ns[r], Ns[s])
                    np.add.at(self.P[r, s], np.ix_(idx, idx), blk)
                    np.add.at(self.Pabs[r, s], np.ix_(idx, idx), np.einsum("q,qa,qb->ab", np.abs(wJ), np.abs(Ns[r]), np.abs(Ns[s])))
            s1 = np.abs(N1).sum(axis=1)
            np.add.at(self.I0, idx, wJ @ N0)
            np.add.at(self.I1abs, idx, wJ @ np.abs(N1))
            np.add.at(self.T01, idx, (wJ * s1) @ np.abs(N0))
            np.add.at(self.T11, idx, (wJ * s1) @ np.abs(N1))
            np.add.at(self.count, idx, 1)
            np.add.at(self.area, idx, LD(2.0 * basis["detJac"][e] / nen))
        self.box_nodes = np.flatnonzero(self.count)


def axis_tables(orc, dim, box=None):
    """AxisTables of every axis of an oracle (box: per-axis (start, width) of a rank's elements)."""
    out = []
    for i in range(dim):
        e0, e1 = (0, None) if box is None else (box[i][0], box[i][0] + box[i][1])
        out.append(AxisTables(orc.axis(i), orc.basis(i), e0, e1))
    return out


# ---- forms: per field pair (f, g) a physical grad-grad coefficient C[f][g][k][l] (of d_k N_a d_l N_b) and a mass coefficient M[f][g]
# (of N_a N_b); Mabs the coefficient of the bound; per field a load Fl[f] (of N_a) with its bound Flabs[f], and for a state form the
# magnitude of the state, whose gradient is zero only in exact arithmetic.
class Form:
    def __init__(self, dim, dof, C=None, M=None, Mabs=None, Fl=None, Flabs=None, state=0.0):
        self.dim, self.dof = dim, dof
        self.C = np.zeros((dof, dof, dim, dim)) if C is None else np.asarray(C, dtype=float)
        self.M = np.zeros((dof, dof)) if M is None else np.asarray(M, dtype=float)
        self.Mabs = np.abs(self.M) if Mabs is None else np.asarray(Mabs, dtype=float)
        self.Fl = np.zeros(dof) if Fl is None else np.asarray(Fl, dtype=float)
        self.Flabs = np.abs(self.Fl) if Flabs is None else np.asarray(Flabs, dtype=float)
        self.state = abs(state)


def poisson(dim, f=1.0):
    return Form(dim, 1, C=np.eye(dim)[None, None], Fl=[f])


def poisson_f(dim):
    """test/IGAFixTable.c (System2): f = -2 dim"""
    return poisson(dim, -2.0 * dim)


def mass(dim, dof):
    return Form(dim, dof, M=np.eye(dof), Fl=np.ones(dof))


def elasticity(lam, mu, f=None):
    """orc_form_elasticity term by term, including the reference's mu * (Na_z Nb_z + Na_x Nb_x mu) in block (1, 1)
    (demo/Elasticity3D.c:37, kept as written); f: the body force of elasticity_f (None: F = 0)."""
    C = np.zeros((3, 3, 3, 3))
    l2 = lam + 2 * mu
    C[0, 0] = np.diag([l2, mu, mu])
    C[1, 1] = np.diag([mu * mu, l2, mu])
    C[2, 2] = np.diag([mu, mu, l2])
    for f_, g_ in ((0, 1), (0, 2), (1, 2)):      # K(a,f,b,g) = lam d_f N_a d_g N_b + mu d_g N_a d_f N_b, its mirror the other way
        C[f_, g_, f_, g_] = lam
        C[f_, g_, g_, f_] = mu
        C[g_, f_, f_, g_] = mu
        C[g_, f_, g_, f_] = lam
    return Form(3, 3, C=C, Fl=np.zeros(3) if f is None else f)


def bratu(dim, lam, c, shift=0.0, v=0.0):
    """Bratu at the constant state U = c, V = v: K = grad N . grad N + (shift - lam e^c) N N, F = (v - lam e^c) N (the Function and
    Jacobian drivers: shift = v = 0)."""
    le = lam * np.exp(c)
    return Form(dim, 1, C=np.eye(dim)[None, None], M=[[shift - le]], Mabs=[[abs(shift) + abs(le)]],
                Fl=[v - le], Flabs=[abs(v) + abs(le)], state=c)


def affine_map(dim, seed=0):
    """A non-diagonal A with det > 0 and condition number <= 4, |b| <= 1."""
    rng = np.random.default_rng(seed)
    while True:
        A = np.eye(dim) + rng.uniform(-0.45, 0.45, size=(dim, dim))
        if np.linalg.det(A) > 0 and np.linalg.cond(A) <= 4.0 and np.abs(A[~np.eye(dim, dtype=bool)]).min(initial=1) > 0.05:
            break
    b = rng.uniform(-1, 1, size=dim)
    b *= min(1.0, 1.0 / np.linalg.norm(b))
    return A, b


def affine_geometry(orc, dim, A, b):
    """Control points X = A g + b at the Greville points g of the oracle's axes ([n2][n1][n0] flattened, axis 0 fastest)."""
    from petiga_amd.geometry import greville
    g = [greville(orc.axis(i)["U"], orc.axis(i)["p"]) for i in range(dim)]
    mesh = np.meshgrid(*g[::-1], indexing="ij")[::-1]
    u = np.stack([m.reshape(-1) for m in mesh], axis=-1)
    return u @ np.asarray(A).T + np.asarray(b)


class TensorRef:
    """R and S of an assembled form at global entries.  tabs: AxisTables per axis; A: the affine map's matrix (None: identity);
    bcs: {(axis, side, field): value} of the Dirichlet faces, loads: {(axis, side, field): value} of the boundary loads;
    driver: "system" (System / Jacobian fix-up: a fixed row is its multiplicity on the diagonal, F_k = mult v_k, free F loses K v),
    "function" (the state is already c everywhere: F_k = mult (c - v_k)) or "matrix" (Matrix / Vector: no fix-up)."""

    def __init__(self, tabs, form, A=None, bcs=None, loads=None, driver="system"):
        fixup = driver != "matrix"
        self.driver = driver
        self.tabs, self.form, self.dim, self.dof = tabs, form, form.dim, form.dof
        assert len(tabs) == self.dim
        self.n = [t.nnp for t in tabs]
        dim = self.dim
        if A is None:
            Ainv, det = np.eye(dim), 1.0
        else:
            A = np.asarray(A, dtype=float)
            Ainv, det = np.linalg.inv(A), float(np.linalg.det(A))
        self.det = det
        # parametric coefficients of d_i N_a d_j N_b: Ainv C Ainv^T, and |Ainv| |C| |Ainv|^T for the bound
        self.K = np.einsum("ik,fgkl,jl->fgij", Ainv, form.C, Ainv) * det
        self.KS = np.einsum("ik,fgkl,jl->fgij", np.abs(Ainv), np.abs(form.C), np.abs(Ainv)) * abs(det)
        self.H = np.abs(Ainv) @ np.abs(Ainv).T * abs(det)
        self.bcs = dict(bcs or {}) if fixup else {}
        self.loads = dict(loads or {}) if fixup else {}

    # -- index helpers
    def split(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        node, f = idx // self.dof, idx % self.dof
        out = []
        for d in range(self.dim):
            out.append(node % self.n[d])
            node = node // self.n[d]
        return out, f

    def fixed(self, idx):
        """(fixed?, value) per global index: the value of the last face in the order (axis, side) that fixes it -- the precedence of
        the reference's BuildFix at edges and corners."""
        tri, f = self.split(idx)
        fx = np.zeros(np.shape(idx), dtype=bool)
        v = np.zeros(np.shape(idx))
        for d in range(self.dim):
            if self.tabs[d].periodic:
                continue
            for side in range(2):
                end = 0 if side == 0 else self.n[d] - 1
                for fld in range(self.dof):
                    if (d, side, fld) in self.bcs:
                        m = (tri[d] == end) & (f == fld)
                        fx |= m
                        v[m] = self.bcs[(d, side, fld)]
        return fx, v

    def multiplicity(self, idx):
        tri, _ = self.split(idx)
        m = np.ones(np.shape(idx), dtype=np.int64)
        for d in range(self.dim):
            m *= self.tabs[d].count[tri[d]]
        return m

    # -- the tensor (no fix-up)
    def _tensor(self, rows, cols):
        ti, fr = self.split(rows)
        tj, fc = self.split(cols)
        dim = self.dim
        P = [self.tabs[d].P[:, :, ti[d], tj[d]] for d in range(dim)]          # [2, 2, n]
        Pa = [self.tabs[d].Pabs[:, :, ti[d], tj[d]] for d in range(dim)]
        R = np.zeros(len(ti[0]), dtype=LD)
        S = np.zeros(len(ti[0]), dtype=LD)
        Kc, KSc = self.K[fr, fc], self.KS[fr, fc]               # [n, dim, dim]
        for i in range(dim):
            for j in range(dim):
                pr, ps = np.ones_like(R), np.ones_like(S)
                for d in range(dim):
                    r, s = int(d == i), int(d == j)
                    pr = pr * P[d][r, s]
                    ps = ps * Pa[d][r, s]
                R += LD(1) * Kc[:, i, j] * pr
                S += LD(1) * KSc[:, i, j] * ps
        m, ma = self.form.M[fr, fc] * self.det, self.form.Mabs[fr, fc] * abs(self.det)
        if np.any(m) or np.any(ma):
            pr, ps = np.ones_like(R), np.ones_like(S)
            for d in range(dim):
                pr = pr * P[d][0, 0]
                ps = ps * Pa[d][0, 0]
            R += LD(1) * m * pr
            S += LD(1) * ma * ps
        return R, S

    def coupled(self, rows, cols):
        ti, _ = self.split(rows)
        tj, _ = self.split(cols)
        ok = np.ones(len(ti[0]), dtype=bool)
        for d in range(self.dim):
            ok &= self.tabs[d].couple[ti[d], tj[d]]
        return ok

    def entries(self, rows, cols):
        """(R, S) of the assembled (and fixed-up) matrix at the global entries (rows, cols)."""
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        R, S = self._tensor(rows, cols)
        if self.bcs:
            fr, _ = self.fixed(rows)
            fc, _ = self.fixed(cols)
            R[fc & ~fr] = 0
            S[fc & ~fr] = 0
            R[fr] = np.where(rows[fr] == cols[fr], self.multiplicity(rows[fr]), 0)
            S[fr] = 0
        return R, S

    def stencil(self, rows):
        """The global columns of every row's full pattern, padded: (cols [n, w], valid [n, w])."""
        rows = np.asarray(rows, dtype=np.int64)
        ti, _ = self.split(rows)
        cols = np.zeros((len(rows), 1), dtype=np.int64)
        valid = np.ones((len(rows), 1), dtype=bool)
        stride = 1
        for d in range(self.dim):
            c = self.tabs[d].couple[ti[d]]                       # [n, nnp]
            w = int(c.sum(axis=1).max()) if len(rows) else 1
            order = np.argsort(~c, axis=1, kind="stable")[:, :w]
            ok = np.take_along_axis(c, order, axis=1)
            cols = (cols[:, :, None] + stride * order[:, None, :]).reshape(len(rows), -1)
            valid = (valid[:, :, None] & ok[:, None, :]).reshape(len(rows), -1)
            stride *= self.n[d]
        out = (cols[:, :, None] * self.dof + np.arange(self.dof)).reshape(len(rows), -1)
        return out, np.repeat(valid, self.dof, axis=1)

    def action(self, X, rows=None):
        """(R, S) of the rows of the assembled (and fixed-up) matrix times X: R_i = sum_j R_ij X_j and S_i = sum_j S_ij |X_j| over the
        row's stencil -- the sum of the absolute values of the terms a matrix-free kernel adds (Pabs takes the absolute value inside
        the point sum).  A fixed row is m X_i, which a kernel that adds X_i once per element rounds: S_i = m |X_i|."""
        X = np.asarray(X, dtype=np.float64)
        rows = np.arange(X.size, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
        cols, valid = self.stencil(rows)
        rr, cc = np.nonzero(valid)
        Re, Se = self.entries(rows[rr], cols[rr, cc])
        Xc = X[cols[rr, cc]]
        R, S = np.zeros(rows.size, dtype=LD), np.zeros(rows.size, dtype=LD)
        np.add.at(R, rr, Re * Xc)
        np.add.at(S, rr, Se * np.abs(Xc))
        if self.bcs:
            fx, _ = self.fixed(rows)
            m = self.multiplicity(rows[fx])
            R[fx] = m * (LD(1) * X[rows[fx]])
            S[fx] = m * np.abs(X[rows[fx]])
        return R, S

    def vector(self, rows):
        """(R, S) of the assembled (and fixed-up) right-hand side / residual at the global rows."""
        rows = np.asarray(rows, dtype=np.int64)
        ti, f = self.split(rows)
        tab = self.tabs
        dim = self.dim
        I = np.ones(len(rows), dtype=LD)
        for d in range(dim):
            I = I * tab[d].I0[ti[d]]
        R = LD(1) * self.form.Fl[f] * self.det * I
        S = LD(1) * self.form.Flabs[f] * abs(self.det) * I
        if self.form.state:                                       # sum |d_x N_a| |c| sum_b |d_x N_b| per point (H = |Ainv| |Ainv|^T)
            G = np.zeros_like(S)
            for i in range(dim):
                for j in range(dim):
                    t = np.ones_like(S)
                    for d in range(dim):
                        if d == i == j:
                            t = t * tab[d].T11[ti[d]]
                        elif d == j:
                            t = t * tab[d].I1abs[ti[d]]
                        elif d == i:
                            t = t * tab[d].T01[ti[d]]
                        else:
                            t = t * tab[d].I0[ti[d]]
                    G += LD(self.H[i, j]) * t
            S += LD(self.form.state) * G
        for (d, side, fld), val in self.loads.items():            # a boundary load: val * face area on every face node (AddFlux)
            if tab[d].periodic:
                continue
            end = 0 if side == 0 else self.n[d] - 1
            a = np.ones_like(S)
            for k in range(dim):
                if k != d:
                    a = a * tab[k].area[ti[k]]
            m = (ti[d] == end) & (f == fld) & (tab[d].count[ti[d]] > 0)
            R[m] += LD(val) * a[m]
            S[m] += LD(abs(val)) * a[m]
        if self.bcs and self.driver == "function":
            fx, v = self.fixed(rows)
            R[fx] = self.multiplicity(rows[fx]) * (LD(self.form.state) - LD(1) * v[fx])
            S[fx] = self.multiplicity(rows[fx]) * (self.form.state + np.abs(v[fx]))
        elif self.bcs:
            fx, v = self.fixed(rows)
            free = np.flatnonzero(~fx)
            if free.size:
                cols, valid = self.stencil(rows[free])
                fc, vc = self.fixed(cols.reshape(-1))
                fc = fc.reshape(cols.shape) & valid
                if fc.any():
                    rr, cc = np.nonzero(fc)
                    K, KS = self._tensor(rows[free][rr], cols[rr, cc])
                    vv = vc.reshape(cols.shape)[rr, cc]
                    corr = np.zeros(free.size, dtype=LD)
                    corrS = np.zeros(free.size, dtype=LD)
                    np.add.at(corr, rr, K * vv)
                    np.add.at(corrS, rr, KS * np.abs(vv))
                    R[free] -= corr
                    S[free] += corrS
            mult = self.multiplicity(rows[fx])
            R[fx] = mult * LD(1) * v[fx]
            S[fx] = mult * np.abs(v[fx])
        return R, S


def compare_entrywise(E, R, S, c, ref=None, what="matrix", pattern=True):
    """E: (rows, cols, vals) of the engine (or (rows, vals) of a vector); R, S at the same entries.  |E - R| <= c u S entry by entry,
    S = 0 meaning exactly zero.  Returns the worst ratio |E - R| / (u S).  With ref, the pattern is checked too: no duplicate entry,
    every entry coupled, and every row's whole stencil present (pattern=False: E is a part of a matrix, ref only names the entries)."""
    if len(E) == 3:
        rows, cols, vals = E
    else:
        (rows, vals), cols = E, None
    rows = np.asarray(rows, dtype=np.int64)
    if cols is not None:
        cols = np.asarray(cols, dtype=np.int64)
    if ref is not None and cols is not None and pattern:
        nmax = int(max(rows.max(initial=0), cols.max(initial=0))) + 1
        key = rows * nmax + cols
        assert np.unique(key).size == key.size, "%s: duplicate entries" % what
        cp = ref.coupled(rows, cols)
        assert cp.all(), "%s: %d entries outside the pattern, first (%d, %d)" % (what, (~cp).sum(), rows[~cp][0], cols[~cp][0])
        ur, cnt = np.unique(rows, return_counts=True)
        _, valid = ref.stencil(ur)
        want = valid.sum(axis=1)
        bad = np.flatnonzero(cnt != want)
        assert bad.size == 0, "%s: row %d has %d entries, its stencil %d" % (what, ur[bad[0]], cnt[bad[0]], want[bad[0]])
    err = np.abs(np.asarray(vals, dtype=LD) - R)
    zero = S == 0
    if zero.any():
        nz = np.flatnonzero(zero & (err != 0))
        if nz.size:
            k = nz[0]
            raise AssertionError("%s: entry %s must be exactly %r, is %r%s" % (what, _where(ref, rows[k], None if cols is None else cols[k]),
                                                                                float(R[k]), float(np.asarray(vals)[k]),
                                                                                "" if nz.size == 1 else " (and %d more)" % (nz.size - 1)))
    ratio = np.zeros(err.shape, dtype=LD)
    ratio[~zero] = err[~zero] / (LD(U_RND) * S[~zero])
    if ratio.size == 0:
        return 0.0
    k = int(np.argmax(ratio))
    worst = float(ratio[k])
    assert worst <= c, "%s: entry %s = %r, reference %r, |E - R| = %.3g = %.1f u S (S = %.3g, c = %g)" % (
        what, _where(ref, rows[k], None if cols is None else cols[k]), float(np.asarray(vals)[k]), float(R[k]), float(err[k]), worst,
        float(S[k]), c)
    return worst


def _where(ref, r, c):
    if ref is None:
        return "(%d, %d)" % (r, c) if c is not None else "%d" % r
    (ti, fr) = ref.split(np.array([r]))
    s = "node (%s) field %d" % (", ".join(str(int(t[0])) for t in ti), int(fr[0]))
    if c is not None:
        (tj, fc) = ref.split(np.array([c]))
        s = "row %s / col node (%s) field %d" % (s, ", ".join(str(int(t[0])) for t in tj), int(fc[0]))
    return s


def matrix_coo(A):
    """(rows, cols, vals) of an oracle CSR matrix."""
    rows = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.rowptr))
    return rows, A.colidx.astype(np.int64), A.val.copy()


# ---- one discretisation set up identically in the CPU oracle and (optionally) the engine, with its reference
USER_X = np.array([-0.93, -0.41, 0.08, 0.66])
USER_W = np.array([0.31, 0.62, 0.71, 0.36])


def graded_knots(p, n, ratio, C=None, seed=None):
    """An open knot vector on [0, 1] with n spans growing geometrically by ratio from the first to the last (seed: random spans
    instead); C: the continuity of every interior knot (repeated p - C times)."""
    if seed is not None:
        h = 0.5 + np.random.default_rng(seed).random(n)
    else:
        h = ratio ** (np.arange(n) / max(n - 1, 1))
    x = np.concatenate([[0.0], np.cumsum(h) / h.sum()])
    x[-1] = 1.0
    rep = 1 if C is None else p - C
    return np.concatenate([[0.0] * p, [x[0]], np.repeat(x[1:-1], rep), [x[-1]], [1.0] * p])


def setup_case(dim, dof, p, N, knots=None, C=None, periodic=None, rule=None, nqp=None, geometry=None, box=None, bcs=None, loads=None,
               engine=False, seed=0):
    """Returns (oracle, engine or None, A of the affine map or None).  rule: None / "lobatto" / "reduced" / "user"; geometry: None /
    "affine" / "rational" (the affine map with constant weights 1.7); box: (size, rank) of a partition."""
    from common import make_pair
    ls = lambda v, d=None: (list(v) if isinstance(v, (list, tuple)) else [v] * dim) if v is not None else [d] * dim
    orc, eng = make_pair(dim, dof, ls(p), ls(N), C=C, periodic=periodic, knots=knots, nqp=nqp, engine=engine)
    objs = [g for g in (orc, eng) if g is not None]
    if rule is not None or box is not None:
        for g in objs:
            for i in range(dim):
                if rule in ("lobatto", "reduced"):
                    g.set_rule_type(i, rule)
                    if nqp is not None:
                        g.set_quadrature(i, ls(nqp)[i])
                elif rule == "user":
                    q = ls(nqp, 4)[i]
                    g.set_rule(i, USER_X[:q], USER_W[:q])
            if box is not None:
                if g is orc:
                    g.set_partition(*box)
                else:
                    g.set_comm(*box)
            g.setup()
    A = None
    if geometry is not None:
        A, b = affine_map(dim, seed)
        X = affine_geometry(orc, dim, A, b)
        W = np.full(len(X), 1.7) if geometry == "rational" else None
        for g in objs:
            g.set_geometry(X, W)
    for g in objs:
        for (d, s, f), v in (bcs or {}).items():
            g.set_boundary_value(d, s, f, v)
        for (d, s, f), v in (loads or {}).items():
            g.set_boundary_load(d, s, f, v)
    return orc, eng, A


def reference(orc, dim, form, A=None, bcs=None, loads=None, driver="system"):
    r = orc.ranges()
    box = list(zip(r["elem_start"], r["elem_width"]))
    return TensorRef(axis_tables(orc, dim, box), form, A=A, bcs=bcs, loads=loads, driver=driver)
