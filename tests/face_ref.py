"""A long double reference of the BOUNDARY-FORM passes: the interior pass of curved_ref.CurvedRef plus one pass per
visited face, on a general NURBS map, entry by entry and row by row with the bound S of curved_ref.py.

A FACE (axis, side) is the same tensor of collocation tables (pointwise_ref.collocation, no element loop, no element-local numbering)
with that axis's table replaced by ONE row: the value, first and second derivative of every global basis function at the end knot
(tensor_ref.bspline_1d_d2 on the end span), weight 1 and Jacobian factor 1.  FacePass is CurvedRef on those tables: W, X W and their
parametric derivatives are interpolated at the face points, x, J, J^-1 and the point coefficients of the basis follow as in
curved_ref.py.  From the columns of J at the face points, as Q triples (v, a, d):

    N      = J[:, t1] x J[:, t2],   (t1, t2) = (axis + 1, axis + 2) mod 3: the un-normalised normal, cyclic order
    detS   = |N|                                           d = sum_k |N_k| / |N| (a + d)_k: Q.fn for a function of a vector
    n      = +-N / detS   (- on side 0)                    d = sum_k |delta_mk - n_m n_k| / |N| (a + d)_k
    JW     = w detS       (w: the product of the other two axes' weights)
    x      = (sum X w N_a) / W
    h      = 2 / |G n|,   G[a][i] = E[a][i] / L_a          the norm as detS, the quotient as Q.fn; E = J^-1; L_a the element half-width, a
                                                           piecewise-constant point field from the oracle's basis(a)["detJac"] (on
                                                           the face axis: the end element's)
    alpha  = C / h

det of the pass is detS, so every form of CurvedRef (linear(), the Bratu terms) integrates its ordinary callback over the face
unchanged.  Nothing in S is fitted to a kernel.  An engine without set_geometry takes the kernels' no-geometry branch (n = +-e_axis,
detS = 1, G = diag(1 / L)); its reference is the same code on the Greville control net (common.greville), which is the identity map
exactly.

FaceRef sums the passes: Nitsche (mat / vec inside, bmat / bvec of forms.hpp's FormNitsche on the faces), BoundaryIntegral, a form without
a boundary branch integrated over the face by its ordinary callback (mass, Poisson), Bratu's Function and Jacobian at a varying state, and
two functionals per face (the area and int x . n dS) beside the volume.  Dirichlet semantics are TensorRef's: the passes of an element
are summed BEFORE the fix-up, so a fixed row holds the exact integer multiplicity of the interior pass on its diagonal (a face pass does
not add to it), fixed columns are zero, and b is lifted by the fixed columns of the sum of all passes.  A rank's element box
(oracle.ranges()) restricts the interior sums and selects which faces, and which part of them, the rank integrates.

3-D only, because the references are 3-D: the kernels' separate 2-D normal branch stays on the parity with the double-precision oracle
of test_boundary_forms.py and test_rtc_boundary_scalar.py.

wrong=: the wrong kernels of test_face_reference.py's teeth tests, one at a time: "normal" (the tangent pair of the next axis), "detS"
(detS of the neighbouring face point along axis t1), "h" (the face axis's L taken from the neighbouring element), "dW" (dW / W dropped
from the quotient rule of the basis on the face), "inward" (the face row's first derivative evaluated one knot span inward, at the end
element's other knot).
"""
import numpy as np

import curved_ref as CR
import tensor_ref as T
from common import greville

LD = T.LD
Q = CR.Q
Z, E1, S10 = CR.Z, CR.E1, CR.S10
# c of |E - R| <= c u S on the face cases: measured on the CPU oracle by test_face_reference.py (its docstring has the ratios); the worst
# is within C_MAP / 4, so no new constant
C_FACE = T.C_MAP


def _end(orc, axis, side):
    """(the end element, its span, the end knot) of a face."""
    ax = orc.axis(axis)
    e = 0 if side == 0 else ax["nel"] - 1
    k = int(ax["span"][e])
    return e, k, float(ax["U"][k] if side == 0 else ax["U"][k + 1])


class _FaceOracle:
    """The oracle of a discretisation with one axis reduced to the one-point, one-element rule of a face: what CurvedRef reads."""

    def __init__(self, orc, axis, side):
        self.orc, self.faxis, self.dim, self.dof = orc, axis, orc.dim, orc.dof
        self.e, self.k, self.u = _end(orc, axis, side)

    def axis(self, i):
        ax = self.orc.axis(i)
        return dict(ax, nel=1, span=np.array([self.k])) if i == self.faxis else ax

    def basis(self, i):
        b = self.orc.basis(i)
        if i != self.faxis:
            return b
        return dict(nel=1, nqp=1, nen=b["nen"], offset=b["offset"][self.e:self.e + 1], detJac=np.ones(1), weight=np.ones((1, 1)),
                    point=np.array([[self.u]]))

    def ranges(self):
        r = self.orc.ranges()
        r = dict(r, elem_start=list(r["elem_start"]), elem_width=list(r["elem_width"]))
        r["elem_start"][self.faxis], r["elem_width"][self.faxis] = 0, 1
        return r


def on_rank(orc, axis, side):
    """Does the rank's element box hold the face's end element?"""
    r = orc.ranges()
    return r["elem_start"][axis] <= _end(orc, axis, side)[0] < r["elem_start"][axis] + r["elem_width"][axis]


def _field(a, values):
    """A per-point 1-D array along axis a as a [q2, q1, q0] point field."""
    shape = [1, 1, 1]
    shape[2 - a] = -1
    return np.asarray(values, dtype=LD).reshape(shape)


def _norm(N):
    """|N| of a vector of Q: Q.fn for a function of several arguments, d = sum_k |d|N| / dN_k| (a_k + d_k) with d|N| / dN_k = N_k / |N|
    (squaring the a_k first, as N . N built from products would, bounds the same rounding a_k / |N_k| times too generously)."""
    v = np.sqrt(sum(c.v * c.v for c in N))
    return Q(v, v, sum(np.abs(c.v) / v * c.s for c in N))


def _unit(N, norm):
    """N / |N|, the same way: d n_m / dN_k = (delta_mk - n_m n_k) / |N|."""
    n = [c.v / norm.v for c in N]
    return [Q(n[m], np.abs(n[m]), sum(np.abs((m == k) - n[m] * n[k]) / norm.v * N[k].s for k in range(3))) for m in range(3)]


class FacePass(CR.CurvedRef):
    """One face's pass: CurvedRef on the face's tables, with det = detS and the normal, x and h of the module docstring."""

    def __init__(self, orc, X, W, axis, side, wrong=None):
        self.faxis, self.fside, self.fwrong, self.real = axis, side, wrong, orc
        CR.CurvedRef.__init__(self, _FaceOracle(orc, axis, side), X, W, wrong="dW" if wrong == "dW" else None)

    def _pattern(self, p):
        """At the end knot only the end function has a value, while its neighbours have derivatives: a function is live on the face when
        any row of its table is non-zero."""
        B = self.B[self.faxis]
        self.B[self.faxis] = np.broadcast_to(np.abs(B).sum(axis=0), B.shape)
        CR.CurvedRef._pattern(self, p)
        self.B[self.faxis] = B

    def _geometry(self, X):
        ax, side, orc = self.faxis, self.fside, self.real
        e, k, u = _end(orc, ax, side)
        assert self.B[ax].shape[1] == 1
        if self.fwrong == "inward":
            A = orc.axis(ax)
            idx = orc.basis(ax)["offset"][e] + np.arange(A["p"] + 1)
            self.B[ax][1, 0, idx] = T.bspline_1d_d2(A["U"], A["p"], k, np.array([A["U"][k + 1] if side == 0 else A["U"][k]]))[1][0]
        CR.CurvedRef._geometry(self, X)
        E, J = self._second[0], self.J                         # (self.xq, self.J: x and d x / d xi at the face points, as Q)
        t0 = ax + 1 if self.fwrong == "normal" else ax
        t1, t2 = (t0 + 1) % 3, (t0 + 2) % 3
        s, t = [J[m][t1] for m in range(3)], [J[m][t2] for m in range(3)]
        N = [s[1] * t[2] - s[2] * t[1], s[2] * t[0] - s[0] * t[2], s[0] * t[1] - s[1] * t[0]]
        detS = _norm(N)
        self.normal = _unit(N if side else [-c for c in N], detS)
        if self.fwrong == "detS":                              # detS of the neighbouring face point along axis t1
            nq, n = orc.basis(t1)["nqp"], detS.v.shape[2 - t1]
            src = np.arange(n) + np.where(np.arange(n) % nq == nq - 1, -1, 1)
            detS = Q(*(np.take(c * np.ones_like(detS.v), src, axis=2 - t1) for c in (detS.v, detS.a, detS.d)))
        self.det = self.detS = detS
        # h = 2 / |G n|
        r = orc.ranges()
        gn = []
        for a in range(3):
            L = orc.basis(a)["detJac"]
            if a == ax:
                en = e if self.fwrong != "h" else min(max(e + (1 if side == 0 else -1), 0), len(L) - 1)
                iL = Q(1 / LD(L[en]))
            else:
                box = L[r["elem_start"][a]:r["elem_start"][a] + r["elem_width"][a]]
                iL = Q(_field(a, np.repeat(1 / np.asarray(box, dtype=LD), orc.basis(a)["nqp"])))
            gn.append((E[a][0] * self.normal[0] + E[a][1] * self.normal[1] + E[a][2] * self.normal[2]) * iL)
        self.h = _norm(gn).fn(lambda v: 2 / v, lambda v: 2 / (v * v))

    # -- the face's integrands
    def nitsche(self, k):
        """(pairs (R, S) on self.pkey, rows (R, S)) of FormNitsche's bmat / bvec: -N_a d_n N_b - N_b d_n N_a + alpha N_a N_b and
        (-d_n N_a + alpha N_a) |x|^2, alpha = 5 (k + 1) / h."""
        alpha = Q(5 * (k + 1)) * self.h.recip()
        x, n, JW = self.xq, self.normal, self.detS
        g = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
        mat, vec = [(self.val, self.val, alpha * JW)], [(self.val, alpha * g * JW)]
        for m in range(3):
            mat += [(self.val, self.grad[m], -(n[m] * JW)), (self.grad[m], self.val, -(n[m] * JW))]
            vec.append((self.grad[m], -(n[m] * g * JW)))
        return self.pairs(mat), self.rows(vec)

    def integral(self, q):
        """(R, S) of sum_q w detS q over the face."""
        q = q * self.detS
        one = np.ones_like(self.Wq)
        return (self.Wq * q.v * one).sum(), (self.Wq * q.s * one).sum()

    def area(self):
        return self.integral(Q(1))

    def flux_of_x(self):
        """int x . n dS"""
        return self.integral(self.xq[0] * self.normal[0] + self.xq[1] * self.normal[1] + self.xq[2] * self.normal[2])


def _form(kind, dof):
    """The interior form and the form the face integrates by its ordinary callback (None: a boundary branch)."""
    if kind == "nitsche":
        return T.poisson_f(3), None
    if kind == "boundary_integral":
        return T.poisson(3, 0.0), None
    f = T.mass(3, dof) if kind == "mass" else T.poisson(3)
    return f, f


class FaceRef:
    """orc: the oracle (3-D); X, W: the control net given to set_geometry (X None: no geometry, the Greville net); bcs: {(axis, side,
    field): value}; faces: the visited (axis, side); wrong: see the module docstring."""

    def __init__(self, orc, X=None, W=None, bcs=None, faces=(), wrong=None):
        assert orc.dim == 3
        if X is None:
            g = [greville(orc.axis(i)["U"], orc.axis(i)["p"]) for i in range(3)]
            X = np.stack([m.reshape(-1) for m in np.meshgrid(*g[::-1], indexing="ij")[::-1]], axis=-1)
        self.interior = CR.CurvedRef(orc, X, W, bcs=bcs)
        self.tref, self.dof = self.interior.tref, orc.dof
        self.visited = sorted(set(faces))
        for a, s in self.visited:
            assert not orc.axis(a)["periodic"]
        self.faces = {f: FacePass(orc, X, W, f[0], f[1], wrong) for f in self.visited if on_rank(orc, *f)}

    @staticmethod
    def _add(K, Kf):
        R, S = Kf.at(K.rows, K.cols)
        assert np.count_nonzero(S) == np.count_nonzero(Kf.S)       # the face's pairs lie on the interior's pattern
        K.R += R
        K.S += S

    def _fix_system(self, K, F, FS, driver):
        I = self.interior
        if driver == "system" and I.fx.any():
            fx, v = I.fx, I.v
            corr, corrS = K.fixed_columns(fx, v)
            F[~fx] -= corr[~fx]
            FS[~fx] += corrS[~fx]
            F[fx] = I.mult[fx] * (LD(1) * v[fx])
            FS[fx] = I.mult[fx] * np.abs(v[fx])
        if driver == "system":
            K.fix(I.fx, I.mult)
        return K, F, FS

    def linear(self, kind, params=(), driver="system"):
        """(K: curved_ref.Entries, F, FS) of System ("system") or Matrix / Vector ("matrix") of "nitsche" (params: k),
        "boundary_integral", "mass" or "poisson"."""
        I = self.interior
        inside, onface = _form(kind, self.dof)
        K, F, FS = I.linear(inside, "matrix")
        for fp in self.faces.values():
            if onface is not None:
                Kf, Ff, FSf = fp.linear(onface, "matrix")
            elif kind == "nitsche":
                prs, (r, s) = fp.nitsche(params[0])
                Kf, Ff, FSf = fp._matrix({(0, 0): prs}), r, s
            else:
                Kf, (Ff, FSf) = None, fp.rows([(fp.val, fp.detS)])
            if Kf is not None:
                self._add(K, Kf)
            F += Ff
            FS += FSf
        return self._fix_system(K, F, FS, driver)

    # -- Bratu at a varying state: the ordinary callback at the face's interpolated state
    def _passes(self):
        return [self.interior] + list(self.faces.values())

    def bratu_function(self, lam, U):
        I = self.interior
        Uf = I._state(U)
        R, S = np.zeros(I.size, dtype=LD), np.zeros(I.size, dtype=LD)
        for r in self._passes():
            terms = [(r.grad[m], r.field(r.grad[m], Uf) * r.det) for m in range(3)]
            terms.append((r.val, -(r._bratu_exp(lam, Uf) * r.det)))
            a, b = r.rows(terms)
            R += a
            S += b
        return I._fix_function(R, S, U)

    def bratu_jacobian(self, lam, U):
        I = self.interior
        Uf = I._state(U)
        K = None
        for r in self._passes():
            terms = [(r.grad[m], r.grad[m], r.det) for m in range(3)]
            terms.append((r.val, r.val, -(r._bratu_exp(lam, Uf) * r.det)))
            Kr = r._matrix({(0, 0): r.pairs(terms)})
            if K is None:
                K = Kr
            else:
                self._add(K, Kr)
        return K.fix(I.fx, I.mult)

    # -- functionals
    def volume(self):
        I = self.interior
        return (I.Wq * I.det.v).sum(), (I.Wq * I.det.s).sum()

    def area(self):
        """(R, S) of the area of the visited faces (of their part in the rank's box)."""
        out = [fp.area() for fp in self.faces.values()]
        return sum(o[0] for o in out), sum(o[1] for o in out)

    def flux_of_x(self):
        out = [fp.flux_of_x() for fp in self.faces.values()]
        return sum(o[0] for o in out), sum(o[1] for o in out)
