"""A long double reference on a GENERAL NURBS map: the control net (X, W) given to set_geometry, curved, with varying rational weights.

tensor_ref.py and pointwise_ref.py stop at an affine map, where the Jacobian is the same at every point, the map's second derivatives
vanish and W is constant: a kernel that reads another point's or element's metric, drops dW / W from the quotient rule or the map's
Hessian from the second-derivative chain, or gathers its control points one node off on a uniform Greville grid agrees with them.  Here
the geometry is evaluated at the quadrature points from the collocation tables of pointwise_ref.py (no element loop, no element-local
numbering): W, X W and their parametric derivatives up to order 2 are interpolated, x, J, det J, J^-1 (by cofactors) and the map's second
derivatives follow by the quotient rule, all in long double.  3-D, any dof, B-spline (W None) or rational basis.  The tables live on the
GEOMETRY GRID: a periodic axis wraps the basis functions but not the control net (its wrapped copies carry control points and weights of
their own), so every sum runs over the unwrapped functions and rows and columns are folded onto the nodes at the end.

POINT COEFFICIENTS.  Every physical feature of the basis function R_a = w_a N_a / W is linear in the parametric derivatives of N_a:

    feature_a(q) = w_a sum_s c_s(q) d^s N_a(q),        s over the ten multi-indices of order <= 2 (S10),

with, writing r_i, r_ij for the parametric derivatives of R_a / w_a, E = J^-1 (E[i][m] = d xi_i / d x_m) and H[m][ij] = d_ij x_m,

    value      1/W
    r_i        d_i N / W - N d_i W / W^2
    r_ij       d_ij N / W - (d_i N d_j W + d_j N d_i W) / W^2 + N (2 d_i W d_j W / W^3 - d_ij W / W^2)
    grad_x m   sum_i E[i][m] r_i
    hess_x kl  sum_ij E[i][k] E[j][l] (r_ij - sum_m H[m][ij] grad_x m)           (lap_x: its trace)

The coefficient fields (self.val, self.grad[m], self.lap: lists of ten point fields) are built once; every form is then
the three operations of pointwise_ref.py with them as the point field: interp() (at), rows() (test), pairs() (pair_tensor, on the pattern of the matrix).

THE BOUND S.  Every point quantity is a triple Q = (v, a, d): the value, the sum of the absolute values of its terms, and a first-order
sensitivity, both in the units in which S is measured.  |E - R| <= c u S with S built from a + d.
    an interpolated sum      v = sum B Y,  a = sum |B| |Y|,  d = 0          (summed in any order it is within ~u a of v)
    x + y                    a = a_x + a_y,  d = d_x + d_y
    x y                      a = a_x a_y,    d = d_x a_y + a_x d_y           (first order: d_x d_y is dropped)
    f(x)                     a = |f(v)|,     d = |f'(v)| (a_x + d_x)         (e^u, 1 / W, c (1 - c), ...: as _bratu_exp and _ch of
                                                                              pointwise_ref.py treat the state)
    E = J^-1                 a = |E|,        d = |E| (a_J + d_J) |E|         (dE = -E dJ E with absolute values)
    det J                    a = |det|,      d = |det| sum_im |E[i][m]| (a_J + d_J)[m][i]          (d det = det tr(E dJ))
So J^-1 J^-T det enters S as |J^-1| |J^-1|^T |det|, as Ga of PointwiseRef, plus the rounding of the interpolated sums
sum |d N_a| |X_a w_a| and sum |d N_a| |w_a| carried through the quotient rule and the inverse: J = sum d N_a X_a cancels from O(1 / h)
terms, which the plain bound does not see.  S bounds any order of summation; nothing in it is fitted to a kernel.

Dirichlet semantics are TensorRef's (fixed / multiplicity, the last face wins), as in pointwise_ref.py.  Boundary loads on a curved face
are out of scope.  A rank's element box (oracle.ranges()) restricts the point sums, as tensor_ref.reference does.
"""
import numpy as np

import pointwise_ref as PW
import tensor_ref as T

LD = T.LD
Z = (0, 0, 0)
E1 = PW.E1
S10 = [Z] + E1 + [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2)]
IDX = {s: k for k, s in enumerate(S10)}


def _plus(s, t):
    return tuple(a + b for a, b in zip(s, t))


class Q:
    """(v, a, d) of the module docstring; scalars and point fields."""
    __slots__ = ("v", "a", "d")

    def __init__(self, v, a=None, d=0):
        self.v = v if isinstance(v, np.ndarray) else LD(v)
        self.a = np.abs(self.v) if a is None else a
        self.d = d

    @property
    def s(self):
        return self.a + self.d

    def zero(self):
        return np.ndim(self.a) == 0 and self.a == 0 and np.ndim(self.d) == 0 and self.d == 0

    def __neg__(self):
        return Q(-self.v, self.a, self.d)

    def __add__(self, o):
        o = _q(o)
        return Q(self.v + o.v, self.a + o.a, self.d + o.d)

    def __sub__(self, o):
        o = _q(o)
        return Q(self.v - o.v, self.a + o.a, self.d + o.d)

    def __mul__(self, o):
        o = _q(o)
        if self.zero() or o.zero():
            return ZERO
        return Q(self.v * o.v, self.a * o.a, self.d * o.a + self.a * o.d)

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return _q(o) - self

    def fn(self, f, df):
        return Q(f(self.v), np.abs(f(self.v)), np.abs(df(self.v)) * self.s)

    def recip(self):
        return self.fn(lambda v: 1 / v, lambda v: 1 / (v * v))


def _q(o):
    return o if isinstance(o, Q) else Q(o)


ZERO = Q(0)


def _unit(s, q):
    out = [ZERO] * 10
    out[IDX[s]] = q
    return out


def _vsum(*vs):
    return [sum((v[k] for v in vs[1:]), vs[0][k]) for k in range(10)]


def _vscale(q, v):
    return [q * x for x in v]


class CurvedRef:
    """orc: the oracle of the discretisation (3-D); X [grid, 3], W [grid] or None: the control net as given to set_geometry;
    bcs: {(axis, side, field): value}.  wrong: one of the wrong kernels of the teeth tests ("point": the metric of the neighbouring point
    along axis 0, "element": one element's metric used for the element after it, "dW": dW / W dropped, "hess": the map's second
    derivatives dropped)."""

    def __init__(self, orc, X, W=None, bcs=None, wrong=None):
        assert orc.dim == 3
        axes = [orc.axis(i) for i in range(3)]
        self.dof, self.wrong = orc.dof, wrong
        self.tref = T.reference(orc, 3, T.Form(3, orc.dof), bcs=bcs, driver="system")          # index helpers and the Dirichlet fix-up
        # the geometry grid: len(U) - p - 1 functions per axis, not wrapped
        tabs = [PW.collocation(dict(axes[i], nnp=len(axes[i]["U"]) - axes[i]["p"] - 1), _untrimmed(orc.basis(i))) for i in range(3)]
        self.nqp = [orc.basis(i)["nqp"] for i in range(3)]
        w, self.B = [], []
        r = orc.ranges()
        for i in range(3):                                     # the rank's element box: no point outside it contributes, none is kept
            box = slice(r["elem_start"][i] * self.nqp[i], (r["elem_start"][i] + r["elem_width"][i]) * self.nqp[i])
            self.B.append(tabs[i][0][:, box, :])
            w.append(tabs[i][1][box])
        self.Wq = np.einsum("k,j,i->kji", w[2], w[1], w[0])
        self.n = [b.shape[2] for b in self.B]                  # the geometry grid ...
        self.grid = int(np.prod(self.n))
        nn = [a["nnp"] for a in axes]                          # ... and the nodes its functions fold onto
        g = [np.arange(self.n[i]) % nn[i] for i in range(3)]
        self.gmap = (g[0][None, None, :] + nn[0] * (g[1][None, :, None] + nn[1] * g[2][:, None, None])).reshape(-1)
        self.nodes = int(np.prod(nn))
        self.size = self.nodes * self.dof
        self.rational = W is not None
        self.wn = np.ones(self.grid, dtype=LD) if W is None else np.asarray(W, dtype=LD).reshape(-1)
        assert self.wn.size == self.grid
        assert np.all(self.wn > 0)
        idx = np.arange(self.size)
        self.fx, self.v = self.tref.fixed(idx) if bcs else (np.zeros(self.size, dtype=bool), np.zeros(self.size))
        self.mult = self.tref.multiplicity(idx)
        self._M = {}
        self._pattern([a["p"] for a in axes])
        self._geometry(np.asarray(X, dtype=LD).reshape(self.grid, 3))

    # -- the three operations
    def _tabs(self, r, absolute):
        return [np.abs(self.B[d][r[d]]) if absolute else self.B[d][r[d]] for d in range(3)]

    def at(self, Y, r, absolute=False):
        """pointwise_ref.PointwiseRef.at: [q2, q1, q0], the parametric derivative r of sum_a Y_a N_a at all points (Y on the grid)."""
        B = self._tabs(r, absolute)
        Yg = np.asarray(Y, dtype=LD).reshape(self.n[2], self.n[1], self.n[0])
        if absolute:
            Yg = np.abs(Yg)
        t = np.einsum("ia,cba->cbi", B[0], Yg)
        t = np.einsum("jb,cbi->cji", B[1], t)
        return np.einsum("kc,cji->kji", B[2], t)

    def interp(self, Y, r):
        return Q(self.at(Y, r), self.at(Y, r, True))

    def test(self, G, r, absolute=False):
        """PointwiseRef.test: [grid], sum_q G_q d^r N_a(q)."""
        B = self._tabs(r, absolute)
        t = np.einsum("ia,kji->kja", B[0], np.asarray(G, dtype=LD))
        t = np.einsum("jb,kja->kba", B[1], t)
        return np.einsum("kc,kba->cba", B[2], t).reshape(-1)

    def _pattern(self, p):
        """The pairs of grid functions that can share an element of the box, |a - b| <= p per axis, and the node pair each folds onto."""
        self.pa, self.pb = [], []
        for d in range(3):
            live = np.any(self.B[d][0] != 0, axis=0)            # the functions with a point of the box in their support
            a, b = np.nonzero((np.abs(np.arange(self.n[d])[:, None] - np.arange(self.n[d])[None, :]) <= p[d]) & live[:, None] & live[None, :])
            self.pa.append(a)
            self.pb.append(b)
        flat = lambda t: (t[0][:, None, None] + self.n[0] * (t[1][None, :, None] + self.n[1] * t[2][None, None, :])).reshape(-1)
        ga, gb = flat(self.pa), flat(self.pb)                  # [L0, L1, L2] flattened: axis 2 fastest
        self.pw = self.wn[ga] * self.wn[gb]
        key = self.gmap[ga].astype(np.int64) * self.nodes + self.gmap[gb]
        self.pkey, self.pinv = np.unique(key, return_inverse=True)

    def _pairs(self, d, r, s, absolute):
        key = (d, r, s, absolute)
        if key not in self._M:
            Br = np.abs(self.B[d][r]) if absolute else self.B[d][r]
            Bs = np.abs(self.B[d][s]) if absolute else self.B[d][s]
            self._M[key] = Br[:, self.pa[d]] * Bs[:, self.pb[d]]
        return self._M[key]

    def pair_band(self, G, r, s, absolute=False):
        """PointwiseRef.pair_tensor on the pattern: sum_q G_q d^r N_i(q) d^s N_j(q) for the pairs of _pattern, [L0 L1 L2] flattened
        (one matrix product per axis)."""
        k, j, i = G.shape
        t = G.reshape(k * j, i) @ self._pairs(0, r[0], s[0], absolute)                        # [k j, L0]
        t = t.reshape(k, j, -1).transpose(0, 2, 1).reshape(-1, j) @ self._pairs(1, r[1], s[1], absolute)   # [k L0, L1]
        return (t.reshape(k, -1).T @ self._pairs(2, r[2], s[2], absolute)).reshape(-1)        # [L0 L1, L2]

    # -- geometry at the points and the point coefficients
    def _geometry(self, X):
        wn = self.wn
        if self.rational:
            Wd = {s: self.interp(wn, s) for s in S10}
            invW = Wd[Z].recip()
        else:
            Wd = {s: ZERO for s in S10}
            Wd[Z] = invW = Q(1)
        P = {s: [self.interp(X[:, m] * wn, s) for m in range(3)] for s in S10}
        x = [P[Z][m] * invW for m in range(3)]
        J = [[(P[E1[i]][m] - x[m] * Wd[E1[i]]) * invW for i in range(3)] for m in range(3)]      # J[m][i] = d_i x_m
        H = [{(i, j): (P[_plus(E1[i], E1[j])][m] - J[m][i] * Wd[E1[j]] - J[m][j] * Wd[E1[i]] - x[m] * Wd[_plus(E1[i], E1[j])]) * invW
              for i in range(3) for j in range(3)} for m in range(3)]
        Jv = np.array([[J[m][i].v for i in range(3)] for m in range(3)])
        Js = np.array([[J[m][i].s * np.ones_like(J[m][i].v) for i in range(3)] for m in range(3)])
        cof = np.empty_like(Jv)                                # cof[i][m]: the cofactor of J[m][i], E = cof / det
        for i in range(3):
            for m in range(3):
                a, b = [k for k in range(3) if k != m], [k for k in range(3) if k != i]
                cof[i, m] = (-1) ** (i + m) * (Jv[a[0], b[0]] * Jv[a[1], b[1]] - Jv[a[0], b[1]] * Jv[a[1], b[0]])
        det = sum(Jv[0, i] * cof[i, 0] for i in range(3))
        Ev = cof / det
        self.x, self.detv = np.array([c.v for c in x]), det
        self.xq, self.J = x, J                                 # (as Q: face_ref.py forms the normal of a face from the columns of J)
        if self.wrong in ("point", "element"):                 # the metric (J^-1, det J, the map's Hessian) of another point
            nq = self.nqp[0]
            if self.wrong == "point":
                src = np.arange(det.shape[2]) + np.where(np.arange(det.shape[2]) % nq == nq - 1, -1, 1)
            else:
                src = np.arange(det.shape[2])
                src[2 * nq:3 * nq] -= nq                       # element 2 along axis 0 reads element 1
            Ev, Js, det = Ev[..., src], Js[..., src], det[..., src]
            H = [{k: Q(h.v[..., src], h.a[..., src], h.d[..., src]) for k, h in Hm.items()} for Hm in H]
        Ea = np.abs(Ev)
        Ed = np.einsum("in...,nj...,jm...->im...", Ea, Js, Ea)
        E = [[Q(Ev[i, m], Ea[i, m], Ed[i, m]) for m in range(3)] for i in range(3)]
        self.det = Q(det, np.abs(det), np.abs(det) * np.einsum("im...,mi...->...", Ea, Js))
        if self.wrong == "hess":
            H = [{k: ZERO for k in Hm} for Hm in H]
        Wb = {s: ZERO for s in S10} if self.wrong == "dW" else Wd          # the W derivatives of the basis's quotient rule
        iW2 = invW * invW
        self.val = _unit(Z, invW)
        rp = [_vsum(_unit(E1[i], invW), _unit(Z, -(Wb[E1[i]] * iW2))) for i in range(3)]
        self.grad = [_vsum(*[_vscale(E[i][m], rp[i]) for i in range(3)]) for m in range(3)]
        self._second = (E, H, Wb, invW)

    @property
    def lap(self):
        """The coefficients of the physical Laplacian: the trace of hess_x (built when a second-order form first asks)."""
        if self._second is not None:
            E, H, Wb, invW = self._second
            iW2, lap = invW * invW, None
            for i in range(3):
                for j in range(i, 3):                          # (t_ij = t_ji: the pairs i < j count twice)
                    ei, ej = E1[i], E1[j]
                    t = _vsum(_unit(_plus(ei, ej), invW), _unit(ei, -(Wb[ej] * iW2)), _unit(ej, -(Wb[ei] * iW2)),
                              _unit(Z, 2 * Wb[ei] * Wb[ej] * iW2 * invW - Wb[_plus(ei, ej)] * iW2),
                              *[_vscale(-H[m][i, j], self.grad[m]) for m in range(3)])
                    c = sum((E[i][k] * E[j][k] for k in range(1, 3)), E[i][0] * E[j][0]) * (1 if i == j else 2)
                    lap = _vscale(c, t) if lap is None else _vsum(lap, _vscale(c, t))
            self._lap, self._second = lap, None
        return self._lap

    # -- fields, rows, matrices from the coefficients
    def field(self, F, Y):
        """The feature F of sum_a Y_a R_a at the points, a Q."""
        Yw = np.asarray(Y, dtype=LD)[self.gmap] * self.wn
        return sum((F[k] * self.interp(Yw, S10[k]) for k in range(10) if not F[k].zero()), ZERO)

    def rows(self, terms):
        """(R, S) [nodes]: sum over the terms (F, G) of sum_q Wq G_q feature F of R_a(q)."""
        R, S = np.zeros(self.grid, dtype=LD), np.zeros(self.grid, dtype=LD)
        for k in range(10):
            g = sum((F[k] * G for F, G in terms if not F[k].zero()), ZERO)
            if g.zero():
                continue
            R += self.test(self.Wq * g.v, S10[k])
            S += self.test(self.Wq * g.s, S10[k], True)
        return self._fold(self.wn * R), self._fold(self.wn * S)

    def _fold(self, A):
        """Rows of the grid summed onto their nodes."""
        if self.grid == self.nodes:
            return A
        out = np.zeros(self.nodes, dtype=LD)
        np.add.at(out, self.gmap, A)
        return out

    def pairs(self, terms):
        """(R, S) on the node pairs self.pkey (row node * nodes + col node, sorted): sum over the terms (F1, F2, G) of
        sum_q Wq G_q F1 of R_i(q) F2 of R_j(q)."""
        R, S = np.zeros(self.pw.size, dtype=LD), np.zeros(self.pw.size, dtype=LD)
        for k in range(10):
            for l in range(10):
                g = sum((F1[k] * F2[l] * G for F1, F2, G in terms if not (F1[k].zero() or F2[l].zero())), ZERO)
                if g.zero():
                    continue
                R += self.pair_band(self.Wq * g.v, S10[k], S10[l])
                S += self.pair_band(self.Wq * g.s, S10[k], S10[l], True)
        out = np.zeros((2, self.pkey.size), dtype=LD)
        np.add.at(out[0], self.pinv, self.pw * R)
        np.add.at(out[1], self.pinv, self.pw * S)
        return out[0], out[1]

    def _matrix(self, blocks):
        """Entries from {(f, g): (R, S) on the node pairs}."""
        rn, cn = self.pkey // self.nodes, self.pkey % self.nodes
        rows = np.concatenate([rn * self.dof + f for f, g in blocks])
        cols = np.concatenate([cn * self.dof + g for f, g in blocks])
        return Entries(self.size, rows, cols, np.concatenate([b[0] for b in blocks.values()]), np.concatenate([b[1] for b in blocks.values()]))

    # -- linear forms: tensor_ref.Form (C, M, Fl), any dof
    def linear(self, form, driver="system"):
        """(K: Entries, F, FS [size]) of System ("system": with the Dirichlet fix-up) or Matrix / Vector ("matrix")."""
        dof, nn = self.dof, self.nodes
        F, FS = np.zeros((nn, dof), dtype=LD), np.zeros((nn, dof), dtype=LD)
        blocks, done = {}, {}
        swap = np.argsort((self.pkey % nn) * nn + self.pkey // nn)          # the node pairs transposed
        for f in range(dof):
            for g in range(dof):
                Cfg, Mfg = form.C[f, g], form.M[f, g]
                if not (np.any(Cfg) or Mfg):
                    continue
                key = (Cfg.tobytes(), float(Mfg), float(form.Mabs[f, g]))
                tkey = (np.ascontiguousarray(Cfg.T).tobytes(), float(Mfg), float(form.Mabs[f, g]))
                if key in done:
                    blocks[f, g] = done[key]
                elif tkey in done:                             # the block of the mirrored pair: its transpose
                    blocks[f, g] = (done[tkey][0][swap], done[tkey][1][swap])
                else:
                    terms = [(self.grad[k], self.grad[l], Q(Cfg[k, l]) * self.det) for k in range(3) for l in range(3) if Cfg[k, l]]
                    if Mfg or form.Mabs[f, g]:
                        terms.append((self.val, self.val, Q(Mfg, form.Mabs[f, g]) * self.det))
                    blocks[f, g] = done[key] = self.pairs(terms)
            if form.Fl[f] or form.Flabs[f]:
                F[:, f], FS[:, f] = self.rows([(self.val, Q(form.Fl[f], form.Flabs[f]) * self.det)])
        K, F, FS = self._matrix(blocks), F.reshape(-1), FS.reshape(-1)
        if driver == "system" and self.fx.any():
            fx, v = self.fx, self.v
            corr, corrS = K.fixed_columns(fx, v)
            F[~fx] -= corr[~fx]
            FS[~fx] += corrS[~fx]
            F[fx] = self.mult[fx] * (LD(1) * v[fx])
            FS[fx] = self.mult[fx] * np.abs(v[fx])
        if driver == "system":
            K.fix(self.fx, self.mult)
        return K, F, FS

    # -- Dirichlet, one field (pointwise_ref.PointwiseRef)
    def _state(self, U):
        return np.where(self.fx, self.v, np.asarray(U, dtype=np.float64))

    def _direction(self, X):
        return np.where(self.fx, 0.0, np.asarray(X, dtype=np.float64))

    _fix_function = PW.PointwiseRef._fix_function
    _fix_action = PW.PointwiseRef._fix_action

    # -- Bratu (oracle/igaforms.c: orc_form_bratu_*)
    def _bratu_exp(self, lam, Uf):
        return self.field(self.val, Uf).fn(lambda u: LD(lam) * np.exp(u), lambda u: LD(lam) * np.exp(u))

    def bratu_function(self, lam, U, V=None):
        """(R, S) of every row of the Function (V None) or IFunction: F_a = [R_a v] + grad R_a . grad u - R_a lambda e^u."""
        assert self.dof == 1
        Uf = self._state(U)
        terms = [(self.grad[m], self.field(self.grad[m], Uf) * self.det) for m in range(3)]
        terms.append((self.val, -(self._bratu_exp(lam, Uf) * self.det)))
        if V is not None:
            terms.append((self.val, self.field(self.val, self._direction(V)) * self.det))
        return self._fix_function(*self.rows(terms), U)

    def bratu_action(self, lam, U, X, shift=0.0):
        """(R, S) of every row of the (I)Jacobian at the state U times X."""
        assert self.dof == 1
        Uf, Xf = self._state(U), self._direction(X)
        terms = [(self.grad[m], self.field(self.grad[m], Xf) * self.det) for m in range(3)]
        terms.append((self.val, (Q(shift) - self._bratu_exp(lam, Uf)) * self.field(self.val, Xf) * self.det))
        return self._fix_action(*self.rows(terms), X)

    def bratu_matrix(self, lam, U, shift=0.0):
        """The (I)Jacobian at the state U, fixed up: Entries."""
        assert self.dof == 1
        terms = [(self.grad[m], self.grad[m], self.det) for m in range(3)]
        terms.append((self.val, self.val, (Q(shift) - self._bratu_exp(lam, self._state(U))) * self.det))
        return self._matrix({(0, 0): self.pairs(terms)}).fix(self.fx, self.mult)

    # -- Cahn-Hilliard (orc_form_ch_residual / orc_form_ch_tangent) with the physical gradient and Laplacian
    def _ch(self, ctx, Uf):
        theta, alpha, _, L0, lam, _ = ctx
        scale = LD(L0) * LD(L0) / LD(lam) if L0 > 0 else 3 * LD(alpha)
        h = LD(0.5) / LD(theta)
        g = lambda c: 1 / (c * (1 - c))
        dmu = lambda c: (h * g(c) - 2) * scale
        d2mu = lambda c: -h * (1 - 2 * c) * g(c) ** 2 * scale
        d3mu = lambda c: h * (2 * g(c) ** 2 + 2 * (1 - 2 * c) ** 2 * g(c) ** 3) * scale
        c = self.field(self.val, Uf)
        k = dict(M=c.fn(lambda c: c * (1 - c), lambda c: 1 - 2 * c), dM=c.fn(lambda c: 1 - 2 * c, lambda c: -2 + 0 * c),
                 dmu=c.fn(dmu, d2mu), d2mu=c.fn(d2mu, d3mu), lap=self.field(self.lap, Uf),
                 grad=[self.field(self.grad[m], Uf) for m in range(3)])
        k["t1"] = k["M"] * k["dmu"] + k["dM"] * k["lap"]
        return k

    def ch_ifunction(self, ctx, U, V):
        """(R, S) of every row of the IFunction: R_a c_t + grad R_a . (M dmu + dM lap c) grad c + lap R_a M lap c."""
        assert self.dof == 1
        Uf, Vf = self._state(U), self._direction(V)
        k = self._ch(ctx, Uf)
        terms = [(self.val, self.field(self.val, Vf) * self.det)]
        terms += [(self.grad[m], k["t1"] * k["grad"][m] * self.det) for m in range(3)]
        terms.append((self.lap, k["M"] * k["lap"] * self.det))
        return self._fix_function(*self.rows(terms), U)

    def ch_action(self, ctx, shift, U, X):
        """(R, S) of every row of the IJacobian (the Tangent) at the state U times X."""
        assert self.dof == 1
        Uf, Xf = self._state(U), self._direction(X)
        k = self._ch(ctx, Uf)
        x, lx = self.field(self.val, Xf), self.field(self.lap, Xf)
        t2 = (k["dM"] * k["dmu"] + k["M"] * k["d2mu"] - 2 * k["lap"]) * x + k["dM"] * lx
        terms = [(self.val, Q(shift) * x * self.det)]
        terms += [(self.grad[m], (k["t1"] * self.field(self.grad[m], Xf) + t2 * k["grad"][m]) * self.det) for m in range(3)]
        terms.append((self.lap, (k["dM"] * k["lap"] * x + k["M"] * lx) * self.det))
        return self._fix_action(*self.rows(terms), X)


class Entries:
    """A matrix on its pattern: (R, S) of the entries (rows, cols), sorted; whatever is not stored is exactly zero."""

    def __init__(self, size, rows, cols, R, S):
        key = rows.astype(np.int64) * size + cols
        o = np.argsort(key)
        assert np.all(np.diff(key[o]) > 0)
        self.size, self.key, self.rows, self.cols, self.R, self.S = size, key[o], rows[o], cols[o], R[o], S[o]

    def at(self, rows, cols):
        """(R, S) at the global entries (rows, cols)."""
        key = np.asarray(rows, dtype=np.int64) * self.size + np.asarray(cols, dtype=np.int64)
        k = np.minimum(np.searchsorted(self.key, key), self.key.size - 1)
        hit = self.key[k] == key
        return np.where(hit, self.R[k], 0), np.where(hit, self.S[k], 0)

    def fix(self, fx, mult):
        """The Dirichlet fix-up of a matrix: a fixed row is its multiplicity on the diagonal, exactly; a fixed column is zero."""
        if fx.any():
            out = fx[self.rows] | fx[self.cols]
            self.R[out] = 0
            self.S[out] = 0
            d = fx[self.rows] & (self.rows == self.cols)
            assert d.sum() == (fx & (mult > 0)).sum()         # (a rank's box holds the diagonals of the rows its elements touch)
            self.R[d] = mult[self.rows[d]]
        return self

    def fixed_columns(self, fx, v):
        """(sum_j K_ij v_j, sum_j S_ij |v_j|) over the fixed columns j, for every row."""
        m = fx[self.cols]
        R, S = np.zeros(self.size, dtype=LD), np.zeros(self.size, dtype=LD)
        np.add.at(R, self.rows[m], self.R[m] * v[self.cols[m]])
        np.add.at(S, self.rows[m], self.S[m] * np.abs(v[self.cols[m]]))
        return R, S

    def action(self, X):
        """(R, S) of the matrix times X; a fixed row is m X_i with S = m |X_i| (its diagonal holds m exactly, S = 0 there)."""
        X = np.asarray(X, dtype=np.float64)
        Sd = np.where((self.S == 0) & (self.rows == self.cols), np.abs(self.R), self.S)
        R, S = np.zeros(self.size, dtype=LD), np.zeros(self.size, dtype=LD)
        np.add.at(R, self.rows, self.R * X[self.cols])
        np.add.at(S, self.rows, Sd * np.abs(X[self.cols]))
        return R, S


def _untrimmed(basis):
    """A reduced rule pads the points it trims (weight 0, point DBL_MAX): give them a point of their element; the weight keeps them out."""
    pt, wt = np.array(basis["point"], dtype=np.float64), np.asarray(basis["weight"])
    return dict(basis, point=np.where(wt == 0, pt[:, :1], pt))
