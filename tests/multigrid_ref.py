"""numpy restatement of IGXMultigrid's cycle (include/petiga_amd.h), written from the header's statement on callables, as krylov_ref.py
restates IGXSolve: the estimate of lambda, the constants, Smooth and V.  Every product, quotient and sum is one numpy operation, so it
rounds on its own, as the sweeps of petiga_amd/csrc/multigrid.hpp do: on the same operators the two give the same bits.

A hierarchy is a Hierarchy of Levels, coarsest first.  A level holds callables: A(v) the action, dinv(v) = D^-1 v, and, above level 0,
restrict(r) = P^T r with the coarse fixed rows set to zero and prolong_add(e, x) = x + P e; level 0 holds coarse(b).
  dense_hierarchy      from matrices (scipy sparse or dense) and prolongation matrices: the diagonal as D, an exact coarse solve
  engine_callables     from a hierarchy of engines through the Python view: the engines' own actions, diagonals (point blocks), transfers
                       and coarse preconditioner, one host copy each way per call
wrong (the teeth of tests/test_multigrid_reference.py): "post-zero" the post-smoother starts from a zero guess, "unmasked" the coarse fixed
rows keep what the restriction put there, "stale-rho" rho_j is not updated from step to step."""
import numpy as np

import krylov_ref as K


class Level:
    def __init__(self, n, A, dinv, restrict=None, prolong_add=None, coarse=None, lam=None):
        self.n, self.A, self.dinv, self.restrict, self.prolong_add, self.coarse, self.lam = n, A, dinv, restrict, prolong_add, coarse, lam


class Hierarchy:
    def __init__(self, levels, degree=2, lo=0.1, hi=1.1, power_its=10, wrong=None):
        self.levels, self.degree, self.lo, self.hi, self.power_its, self.wrong = list(levels), int(degree), float(lo), float(hi), int(power_its), wrong
        self.trace = {}      # what the last cycle saw: ("restricted", l) the masked coarse right-hand side, ("correction", l) P e on level l

    def setup(self, lambdas=None, norm=np.linalg.norm):
        """lambda_l of every level above the coarsest: the host's own power iteration, or the figures given (IGXMultigridGetInfo's)"""
        for l, lv in enumerate(self.levels):
            if lambdas is not None:
                lv.lam = float(lambdas[l])
            elif l > 0 or lv.coarse is None:
                lv.lam = estimate_lambda(lv.A, lv.dinv, lv.n, self.power_its, norm)
        return self

    def apply(self, r):
        """z = B r: one V-cycle from a zero guess on the finest level"""
        return vcycle(self, len(self.levels) - 1, np.asarray(r, dtype=np.float64))


def start_vector(n):
    return np.sin(1.0 + np.arange(n, dtype=np.float64))


def estimate_lambda(A, dinv, n, its, norm=np.linalg.norm):
    """its steps of the power method on D^-1 A from v_i = sin(1 + i): per step z = D^-1 A v, lambda = |z| / |v|, v = (1 / |z|) z"""
    v, lam = start_vector(n), 0.0
    for _ in range(its):
        nv = norm(v)
        z = dinv(A(v))
        nz = norm(z)
        lam = nz / nv
        v = (1.0 / nz) * z
    return float(lam)


def constants(lam, lo, hi, degree, wrong=None):
    """(1 / theta, [rho_j rho_{j-1}], [2 rho_j / delta]) for j = 2 .. degree, in the header's order of operations"""
    theta = (hi + lo) * lam / 2
    delta = (hi - lo) * lam / 2
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = {}, {}
    for j in range(2, degree + 1):
        rn = 1.0 / (2 * sigma - rho)
        c1[j], c2[j] = rn * rho, 2 * rn / delta
        if wrong != "stale-rho":
            rho = rn
    return 1.0 / theta, c1, c2


def smooth(h, l, b, x=None):
    """Smooth(l, b, x, zero guess = x is None): (x, r, d), r the residual before the last step's correction d"""
    lv = h.levels[l]
    c, c1, c2 = constants(lv.lam, h.lo, h.hi, h.degree, h.wrong)
    r = b.copy() if x is None else b - lv.A(x)
    z = lv.dinv(r)
    d = c * z
    x = d.copy() if x is None else x + d
    for j in range(2, h.degree + 1):
        w = lv.A(d)
        r = r - w
        z = lv.dinv(r)
        d = c1[j] * d + c2[j] * z
        x = x + d
    return x, r, d


def vcycle(h, l, b):
    lv = h.levels[l]
    if l == 0:
        return lv.coarse(b)
    x, r, d = smooth(h, l, b)
    r = r - lv.A(d)
    bc = lv.restrict(r, mask=h.wrong != "unmasked")
    h.trace[("restricted", l - 1)] = bc.copy()
    e = vcycle(h, l - 1, bc)
    x2 = lv.prolong_add(e, x)
    h.trace[("correction", l)] = x2 - x
    if h.wrong == "post-zero":
        return smooth(h, l, b)[0]
    return smooth(h, l, b, x2)[0]


def fixed_mask(nodes, dof, fixed):
    """bool [n]: the rows of the Dirichlet faces; nodes = (n0, n1, n2) of the level, fixed = [(axis, side, field)], numbering [n2][n1][n0][dof]"""
    n0, n1, n2 = (list(nodes) + [1, 1])[:3]
    m = np.zeros((n2, n1, n0, dof), dtype=bool)
    for axis, side, field in fixed:
        idx = [slice(None)] * 3
        idx[2 - axis] = -1 if side else 0
        m[tuple(idx) + (field,)] = True
    return m.reshape(-1)


def dense_hierarchy(As, Ps, masks, **kw):
    """As[l]: the level's matrix (fixed rows included, as the oracle assembles them); Ps[l-1]: the prolongation from level l-1 to l;
    masks[l]: fixed_mask of level l.  D is the matrix' diagonal and the coarse solve a sparse LU."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    levels = []
    for l, A in enumerate(As):
        A = sp.csr_matrix(A)
        D = A.diagonal()
        lv = Level(A.shape[0], (lambda v, A=A: A @ v), (lambda v, D=D: v / D))
        if l == 0:
            lu = spla.splu(A.tocsc())
            lv.coarse = lambda b, lu=lu: lu.solve(b)
        else:
            P, mc = sp.csr_matrix(Ps[l - 1]), masks[l - 1]
            PT = P.T.tocsr()

            def restrict(r, mask=True, PT=PT, mc=mc):
                bc = PT @ r
                if mask:
                    bc[mc] = 0.0
                return bc
            lv.restrict, lv.prolong_add = restrict, (lambda e, x, P=P: x + P @ e)
        levels.append(lv)
    return Hierarchy(levels, **kw)


def engine_callables(engines, fixed, op="matrix", smoother="jacobi", coarse=None, states=None, a=0.0, t=0.0, **kw):
    """A Hierarchy on the engines' own operators (coarsest first), driven through the Python view.  fixed: [(axis, side, field)] of the
    Dirichlet faces; states: per level a dict of U / V Vecs; coarse: dict(pc=..., maxit=0) for one application of the engine's
    preconditioner, or dict(method=, pc=, rtol=, maxit=) for the host loop of krylov_ref on level 0's callables."""
    coarse = dict(coarse or dict(pc="jacobi", maxit=0))
    states = states or [dict() for _ in engines]
    levels, transfers = [], []
    for l, eng in enumerate(engines):
        st = dict(a=a, t=t, **states[l]) if op == "ijacobian" else dict(states[l])
        action, dinv = K.engine_callables(eng, op=op, pc=smoother, **st)
        lv = Level(eng.create_vec().n, action, dinv)
        if l == 0:
            if coarse.get("maxit", 0) == 0:
                lv.coarse = K.engine_callables(eng, op=op, pc=coarse["pc"], **st)[1]
            else:
                act0, prec0 = K.engine_callables(eng, op=op, pc=coarse["pc"], **st)
                loop = K.cg if coarse.get("method", "cg") == "cg" else K.bicgstab
                lv.coarse = lambda b, loop=loop, act0=act0, prec0=prec0: loop(act0, prec0, b, rtol=coarse["rtol"], maxit=coarse["maxit"])[0]
        else:
            tr = eng.transfer(engines[l - 1])
            transfers.append(tr)
            nodes = [tr.sizes(d)[1] for d in range(3)]
            mc = fixed_mask(nodes, eng.dof, fixed)
            vc, vf = engines[l - 1].create_vec(), eng.create_vec()

            def restrict(r, mask=True, tr=tr, vc=vc, vf=vf, mc=mc, eng=eng):
                tr.restrict(vf.set(r), vc)
                eng.synchronize()
                bc = vc.get().copy()
                if mask:
                    bc[mc] = 0.0
                return bc

            def prolong_add(e, x, tr=tr, vc=vc, vf=vf, eng=eng):
                tr.prolong(vc.set(e), vf.set(x), add=True)
                eng.synchronize()
                return vf.get().copy()
            lv.restrict, lv.prolong_add = restrict, prolong_add
        levels.append(lv)
    h = Hierarchy(levels, **kw)
    h.transfers = transfers
    return h
