"""A long double restatement of the probe's contract (IGXProbe, include/petiga_amd.h): the value and the derivatives up to order 3 of a
discrete field at arbitrary parametric points, dim 1..3, any degree, B-spline or rational basis, identity or mapped geometry.

  span        IGA_FindSpan's rule per axis: U[k] <= u < U[k+1]; the upper end of the axis belongs to the last non-empty span, so an
              interior knot is evaluated from the right and a repeated knot never yields an empty span.
  1-D rows    N, N', N'', N''' of the p + 1 functions of the span by the Cox-de Boor triangle and the derivative recurrence
              N^(r)_{i,d} = d (N^(r-1)_{i,d-1} / (U[i+d] - U[i]) - N^(r-1)_{i+1,d-1} / (U[i+d+1] - U[i+1]))   (tensor_ref.py stops at r = 2).
  sums        the distinct parametric partials d^s of sum_a c_a N_a, c = w (the weight W), w X_m (the map) and w U_f (a field).
  chain       on the sums: the quotient rule (y = A / W differentiated three times), then with E = J^-1, g = grad_x f, h = hess_x f:
                f_a = g_l x^l_a;  f_ab = h_lm x^l_a x^m_b + g_l x^l_ab;
                f_abc = t_lmn x^l_a x^m_b x^n_c + h_lm (x^l_ab x^m_c + x^l_ac x^m_b + x^l_bc x^m_a) + g_l x^l_abc
              solved for g, h, t in turn.  Physical derivatives when the geometry has nsd = dim, parametric otherwise.

Every output entry comes back as R with its magnitude sum S in the (v, a, d) convention of curved_ref.py (curved_ref.Q): an interpolated
sum has a = sum |d^s N_a| |c_a| and d = 0, products and functions propagate a and the first-order sensitivity d, S = a + d.  The check is
|E - R| <= c u S with c = tensor_ref.C_ID on the identity geometry and tensor_ref.C_MAP on a map for orders 0..2, and C3 below for order
3 on a map.

C3.  Nobody had measured an order-3 ratio on a map.  tests/test_probe_reference.py measures the CPU oracle's own double precision
tabulation (orc.element: shape[3]) against this reference over its cases (dof 1 and 3, 2-D and 3-D, affine / polynomial warp / NURBS):
the worst ratio |E - R| / (u S) is WORST3 below; C3 = max(C_MAP, 4 x WORST3 rounded up to a power of two), the factor 4 for a device
summation order that differs from the oracle's.  The oracle defines the constant, the engine never does.

Coefficients are in the engine's natural numbering: node * dof + field, node = i0 + nn0 * (i1 + nn1 * i2), nn = nnp (a periodic axis
wraps the functions onto its nnp nodes); the control net (X [grid, nsd], W [grid] or None) lives on the geometry grid, len(U) - p - 1
functions per axis, not wrapped.

wrong: one of the perturbed references of the teeth tests -- "left" (a knot evaluated from the left), "weights" (W ignored), "transpose"
(the inverse map transposed), "mixed3" (the mixed third partial d_0 d_0 d_1 dropped), "endspan" (the upper end sent to the empty span
behind it, where every function vanishes).
"""
import itertools

import numpy as np

import curved_ref as CR
import tensor_ref as T

LD = T.LD
Q = CR.Q
ZERO = CR.ZERO
U_RND = T.U_RND
C_ID, C_MAP = T.C_ID, T.C_MAP
WORST3 = 0.02              # the oracle's worst order-3 ratio on a map over the cases of test_probe_reference.py: measured 0.0186 (S carries the
                           # sensitivities of the quotient rule and of the inverse map, which the oracle's rounding comes nowhere near)
C3 = max(C_MAP, 0.125)     # 4 x WORST3 = 0.08, rounded up to a power of two: 0.125; C_MAP = 256 is the larger and stands


def bound(der, mapped):
    return (C3 if der == 3 else C_MAP) if mapped else C_ID


def find_span(U, p, u, wrong=None):
    """IGA_FindSpan for an array of points."""
    U, u = np.asarray(U, dtype=np.float64), np.asarray(u, dtype=np.float64)
    n = len(U) - p - 2                                       # the last function; the axis is [U[p], U[n+1]]
    assert np.all((u >= U[p]) & (u <= U[n + 1]))
    if wrong == "left":                                      # U[k] < u <= U[k+1]
        k = np.searchsorted(U, u, side="left") - 1
        return np.clip(k, p, n)
    k = np.searchsorted(U, u, side="right") - 1
    if wrong == "endspan":
        return k                                             # u = U[n+1] lands behind the last function
    end = u >= U[n + 1]
    k = np.where(end, n, k)
    while True:                                              # the last non-empty span
        empty = end & (k > p) & (U[k] == U[np.minimum(k + 1, len(U) - 1)])
        if not empty.any():
            return k
        k = np.where(empty, k - 1, k)


def rows_1d(U, p, k, x, nder=3):
    """[nder + 1] arrays [nx, p + 1]: the derivatives 0..nder of the functions k - p .. k at the points x of span k, long double."""
    U = np.asarray(U, dtype=LD)
    x = np.asarray(x, dtype=LD)
    V = [[np.ones_like(x)]]                                  # V[d][j]: function j of degree d on the span, knot index k - d + j
    for d in range(1, p + 1):
        old, new = V[-1], []
        for j in range(d + 1):
            i = k - d + j
            t = np.zeros_like(x)
            if j > 0 and U[i + d] != U[i]:
                t = t + (x - U[i]) / (U[i + d] - U[i]) * old[j - 1]
            if j < d and U[i + d + 1] != U[i + 1]:
                t = t + (U[i + d + 1] - x) / (U[i + d + 1] - U[i + 1]) * old[j]
            new.append(t)
        V.append(new)
    out, D = [np.stack(V[p], axis=-1)], V                    # D[d]: the current derivative order of the degree-d functions
    for r in range(1, nder + 1):
        nxt = [None] * (p + 1)
        for d in range(r, p + 1):
            row = []
            for j in range(d + 1):
                i = k - d + j
                t = np.zeros_like(x)
                if j > 0 and U[i + d] != U[i]:
                    t = t + d * D[d - 1][j - 1] / (U[i + d] - U[i])
                if j < d and U[i + d + 1] != U[i + 1]:
                    t = t - d * D[d - 1][j] / (U[i + d + 1] - U[i + 1])
                row.append(t)
            nxt[d] = row
        D = nxt
        out.append(np.stack(D[p], axis=-1) if p >= r else np.zeros((len(x), p + 1), dtype=LD))
    return out


def _inverse(J):
    """E = J^-1 by cofactors for [dim][dim] lists of arrays: (E, det)."""
    n = len(J)
    if n == 1:
        return [[1 / J[0][0]]], J[0][0]
    if n == 2:
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        return [[J[1][1] / det, -J[0][1] / det], [-J[1][0] / det, J[0][0] / det]], det
    cof = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for m in range(3):
            a, b = [k for k in range(3) if k != m], [k for k in range(3) if k != i]
            cof[i][m] = (-1) ** (i + m) * (J[a[0]][b[0]] * J[a[1]][b[1]] - J[a[0]][b[1]] * J[a[1]][b[0]])
    det = sum(J[0][i] * cof[i][0] for i in range(3))
    return [[cof[i][m] / det for m in range(3)] for i in range(3)], det


def _key(*axes):
    """the multi-index (k0, k1, k2) of the partial along the given axes"""
    return tuple(sum(1 for a in axes if a == d) for d in range(3))


class ProbeRef:
    """axes: per axis a dict with p, U, nnp (OracleIGA.axis(i)); X [grid, nsd], W [grid] or None: the control net as given to
    set_geometry (None: identity)."""

    def __init__(self, axes, dof, X=None, W=None, wrong=None):
        self.axes, self.dim, self.dof, self.wrong = axes, len(axes), dof, wrong
        self.n = [len(a["U"]) - a["p"] - 1 for a in axes]                   # the geometry grid
        self.nn = [a["nnp"] for a in axes]
        self.grid = int(np.prod(self.n))
        self.nsd = 0 if X is None else np.asarray(X).reshape(self.grid, -1).shape[1]
        self.X = None if X is None else np.asarray(X, dtype=LD).reshape(self.grid, self.nsd)
        self.W = None if (W is None or wrong == "weights") else np.asarray(W, dtype=LD).reshape(self.grid)
        self.mapped = self.nsd == self.dim and self.nsd > 0

    # -- location and rows
    def locate(self, pts):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, self.dim)
        return [find_span(self.axes[d]["U"], self.axes[d]["p"], pts[:, d], self.wrong) for d in range(self.dim)]

    def _rows(self, pts, nder):
        """per axis: span [npts], tables [nder + 1][npts, p + 1]"""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, self.dim)
        spans, tabs = self.locate(pts), []
        for d in range(self.dim):
            ax, k = self.axes[d], spans[d]
            p = ax["p"]
            tab = [np.zeros((len(pts), p + 1), dtype=LD) for _ in range(nder + 1)]
            for kk in np.unique(k):
                sel = np.flatnonzero(k == kk)
                if kk > len(ax["U"]) - p - 2:                # "endspan": an empty span, every function vanishes
                    continue
                r = rows_1d(ax["U"], p, int(kk), pts[sel, d], nder)
                for o in range(nder + 1):
                    tab[o][sel] = r[o]
            tabs.append(tab)
        return spans, tabs

    def _sum(self, spans, tabs, coef, s):
        """Q [npts]: sum_a coef_a prod_d N^(s_d)_{a_d} over the functions of each point's span; coef(idx per axis [npts, p_d + 1]) ->
        [npts, (p2+1), (p1+1), (p0+1)] (trailing axes only up to dim)."""
        dim = self.dim
        idx = [np.minimum(spans[d][:, None] - self.axes[d]["p"] + np.arange(self.axes[d]["p"] + 1)[None, :], self.n[d] - 1) for d in range(dim)]
        c = coef(idx)
        letters = "ijk"[:dim]
        sub = "n" + letters[::-1] + "," + ",".join("n" + l for l in letters) + "->n"
        B = [tabs[d][s[d]] for d in range(dim)]
        v = np.einsum(sub, c, *B)
        a = np.einsum(sub, np.abs(c), *[np.abs(b) for b in B])
        return Q(v, a, 0)

    def _grid_coef(self, Y):
        """coefficients on the geometry grid"""
        def f(idx):
            g = idx[0][:, None, None, :] if self.dim == 3 else (idx[0][:, None, :] if self.dim == 2 else idx[0])
            if self.dim >= 2:
                g = g + self.n[0] * (idx[1][:, None, :, None] if self.dim == 3 else idx[1][:, :, None])
            if self.dim == 3:
                g = g + self.n[0] * self.n[1] * idx[2][:, :, None, None]
            return Y[g]
        return f

    def _node_of_grid(self):
        g = [np.arange(self.n[d]) % self.nn[d] for d in range(self.dim)]
        out, stride = np.zeros([self.n[d] for d in range(self.dim)][::-1], dtype=np.int64), 1
        for d in range(self.dim):
            shape = [1] * self.dim
            shape[self.dim - 1 - d] = self.n[d]
            out = out + stride * g[d].reshape(shape)
            stride *= self.nn[d]
        return out.reshape(-1)

    def _partials(self, spans, tabs, Y, der):
        """{multi-index: Q} of the distinct partials of order <= der of sum_a Y_a N_a (Y on the grid)"""
        out = {}
        for s in itertools.product(range(der + 1), repeat=3):
            if sum(s) <= der and all(s[d] == 0 for d in range(self.dim, 3)):
                if self.wrong == "mixed3" and s == (2, 1, 0):
                    out[s] = ZERO
                else:
                    out[s] = self._sum(spans, tabs, self._grid_coef(Y), s)
        return out

    def _quot(self, A, Wd, invW, der):
        """the quotient rule on the sums: the partials of A / W"""
        dim, y = self.dim, {}
        y[_key()] = A[_key()] * invW
        if der >= 1:
            for a in range(dim):
                y[_key(a)] = (A[_key(a)] - y[_key()] * Wd[_key(a)]) * invW
        if der >= 2:
            for a in range(dim):
                for b in range(a, dim):
                    y[_key(a, b)] = (A[_key(a, b)] - y[_key()] * Wd[_key(a, b)] - y[_key(a)] * Wd[_key(b)] - y[_key(b)] * Wd[_key(a)]) * invW
        if der >= 3:
            for a in range(dim):
                for b in range(a, dim):
                    for c in range(b, dim):
                        y[_key(a, b, c)] = (A[_key(a, b, c)] - y[_key()] * Wd[_key(a, b, c)]
                                            - y[_key(a)] * Wd[_key(b, c)] - y[_key(b)] * Wd[_key(a, c)] - y[_key(c)] * Wd[_key(a, b)]
                                            - y[_key(b, c)] * Wd[_key(a)] - y[_key(a, c)] * Wd[_key(b)] - y[_key(a, b)] * Wd[_key(c)]) * invW
        return y

    def _geometry(self, spans, tabs, der):
        """(Wd, invW, x partials per component) at the points, to order der"""
        ones = np.ones(self.grid, dtype=LD)
        Wd = invW = None
        if self.W is not None:
            Wd = self._partials(spans, tabs, self.W, der)
            invW = Wd[_key()].recip()
        xs = []
        if self.X is not None:
            for m in range(self.nsd):
                A = self._partials(spans, tabs, self.X[:, m] * (ones if self.W is None else self.W), der)
                xs.append(A if self.W is None else self._quot(A, Wd, invW, der))
        return Wd, invW, xs

    def geom_map(self, pts):
        """(R, S) [npts, nsd] (no geometry: the points themselves, S = |u|)"""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, self.dim)
        if self.X is None:
            return pts.astype(LD), np.abs(pts).astype(LD)
        spans, tabs = self._rows(pts, 0)
        _, _, xs = self._geometry(spans, tabs, 0)
        one = np.ones(len(pts), dtype=LD)
        return np.stack([x[_key()].v * one for x in xs], axis=-1), np.stack([x[_key()].s * one for x in xs], axis=-1)

    def evaluate(self, coef, pts, der):
        """(R, S) [npts, dof, dim, ...]: derivative der of every field of the coefficient vector (natural numbering) at the points"""
        dim, dof = self.dim, self.dof
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, dim)
        npts = len(pts)
        coef = np.asarray(coef, dtype=LD).reshape(-1, dof)[self._node_of_grid()]           # on the geometry grid
        spans, tabs = self._rows(pts, der)
        chain = self.mapped and der > 0
        Wd, invW, xs = self._geometry(spans, tabs, der if chain else 0) if (self.W is not None or chain) else (None, None, [])
        if self.W is not None and not chain and der > 0:
            Wd = self._partials(spans, tabs, self.W, der)
        if chain:
            J = [[xs[m][_key(i)] for i in range(dim)] for m in range(dim)]                  # J[m][i] = d_i x_m
            one = np.ones(npts, dtype=LD)
            Jv = [[J[m][i].v * one for i in range(dim)] for m in range(dim)]
            Js = np.array([[J[m][i].s * one for i in range(dim)] for m in range(dim)])
            Ev, _ = _inverse(Jv)
            Ev = np.array(Ev)
            if self.wrong == "transpose":
                Ev = Ev.transpose(1, 0, 2)
            Ea = np.abs(Ev)
            Ed = np.einsum("in...,nj...,jm...->im...", Ea, Js, Ea)
            E = [[Q(Ev[i, m], Ea[i, m], Ed[i, m]) for m in range(dim)] for i in range(dim)]  # E[a][i] = du_a / dx_i
        shape = (npts, dof) + (dim,) * der
        R, S = np.zeros(shape, dtype=LD), np.zeros(shape, dtype=LD)
        wgrid = np.ones(self.grid, dtype=LD) if self.W is None else self.W
        for f in range(dof):
            F = self._partials(spans, tabs, coef[:, f] * wgrid, der)
            if self.W is not None:
                F = self._quot(F, Wd, invW, der)
            if der == 0:
                res = {(): F[_key()]}
            elif not chain:
                res = {ix: F[_key(*ix)] for ix in itertools.product(range(dim), repeat=der)}
            else:
                rng = range(dim)
                g = [sum((F[_key(a)] * E[a][i] for a in rng), ZERO) for i in rng]
                res = {(i,): g[i] for i in rng}
                if der >= 2:
                    r2 = {(a, b): F[_key(a, b)] - sum((g[l] * xs[l][_key(a, b)] for l in rng), ZERO) for a in rng for b in rng}
                    h = {(i, j): sum((r2[a, b] * E[a][i] * E[b][j] for a in rng for b in rng), ZERO) for i in rng for j in rng}
                    res = h
                if der >= 3:
                    r3 = {}
                    for a, b, c in itertools.product(rng, repeat=3):
                        t = F[_key(a, b, c)] - sum((g[l] * xs[l][_key(a, b, c)] for l in rng), ZERO)
                        for l in rng:
                            for m in rng:
                                t = t - h[l, m] * (xs[l][_key(a, b)] * xs[m][_key(c)] + xs[l][_key(a, c)] * xs[m][_key(b)] + xs[l][_key(b, c)] * xs[m][_key(a)])
                        r3[a, b, c] = t
                    res = {(i, j, k): sum((r3[a, b, c] * E[a][i] * E[b][j] * E[c][k] for a, b, c in itertools.product(rng, repeat=3)), ZERO)
                           for i, j, k in itertools.product(rng, repeat=3)}
            for ix, q in res.items():
                R[(slice(None), f) + ix] = q.v
                S[(slice(None), f) + ix] = q.s
        return R, S


def compare(E, R, S, c, what="probe"):
    """|E - R| <= c u S entry by entry (S = 0: exactly R); returns the worst ratio."""
    E, R, S = np.asarray(E, dtype=LD), np.asarray(R, dtype=LD), np.asarray(S, dtype=LD)
    assert E.shape == R.shape == S.shape, (what, E.shape, R.shape, S.shape)
    assert np.all(np.isfinite(E.astype(np.float64))), "%s: a non-finite entry" % what
    err = np.abs(E - R)
    zero = S == 0
    assert not np.any(err[zero] != 0), "%s: an entry with S = 0 is not exact" % what
    ratio = np.zeros(err.shape, dtype=LD)
    ratio[~zero] = err[~zero] / (LD(U_RND) * S[~zero])
    if ratio.size == 0:
        return 0.0
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[k])
    assert worst <= c, "%s: entry %s = %r, reference %r, |E - R| = %.3g = %.1f u S (S = %.3g, c = %g)" % (
        what, k, float(E[k]), float(R[k]), float(err[k]), worst, float(S[k]), c)
    return worst


GEOMETRIES = ("identity", "affine", "warp", "nurbs")


def geometry(orc, dim, kind, seed=3):
    """(X, W) of the four geometries of the probe's tests on the oracle's geometry grid: None, an affine map (tensor_ref.affine_map), the
    polynomial warp and the NURBS map with varying weights (common.warped_geometry, as the curved-map tests use them)."""
    from common import warped_geometry
    if kind == "identity":
        return None, None
    if kind == "affine":
        A, b = T.affine_map(dim, seed)
        return T.affine_geometry(orc, dim, A, b), None
    return warped_geometry(orc, dim, seed=seed, rational=(kind == "nurbs"))


def axes_of(orc):
    return [orc.axis(i) for i in range(orc.dim)]


def oracle_at_element(orc, ID, coef, der):
    """(points [nqp, dim], E [nqp, dof, dim, ...]): the oracle's own double precision tabulation of element ID (shape[der]) applied to the
    coefficients (natural numbering; one rank, no periodic axis: the ghosted-local node index is the node)."""
    el = orc.element(list(ID))
    Ue = np.asarray(coef, dtype=np.float64).reshape(-1, orc.dof)[el["mapping"]]
    sh = el["shape%d" % der]
    return el["point"], np.moveaxis(np.tensordot(sh, Ue, axes=([1], [0])), -1, 1)
