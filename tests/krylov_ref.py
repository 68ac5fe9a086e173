"""numpy restatements of the two loops of IGXSolve (include/petiga_amd.h), written from the method's statement and independently of
krylov.hpp: preconditioned CG -- the loop of pcg() in tests/fast_diag_ref.py with an initial guess, atol, a history and the outcomes -- and
right-preconditioned BiCGStab in the order DESIGN.md 3.12 states (one test of |r| per iteration, no half-step exit).  `dot` is the inner product the loop uses: np.dot, or another summation
order to see what rounding alone moves.  Both return (x, info) with info = dict(iterations, reason, rnorm0, rnorm, bnorm, history)."""
import math

import numpy as np

from fast_diag_ref import pcg      # noqa: F401  (the loop cg() restates; tests/test_krylov_abi.py holds the two against each other)

CONVERGED_RTOL, CONVERGED_ATOL, DIVERGED_ITS, DIVERGED_BREAKDOWN, DIVERGED_NAN = 1, 2, -1, -2, -3


def _bad(d):
    return d == 0.0 or not np.isfinite(d)


def _stop(rnorm, bnorm, rtol, atol, its, maxit):
    if np.isnan(rnorm):
        return DIVERGED_NAN
    if rnorm <= max(rtol * bnorm, atol):
        return CONVERGED_RTOL if rnorm <= rtol * bnorm else CONVERGED_ATOL
    if its >= maxit:
        return DIVERGED_ITS
    return 0


def _info(its, reason, hist, bnorm):
    return dict(iterations=its, reason=reason, rnorm0=hist[0], rnorm=hist[-1], bnorm=bnorm, history=np.array(hist))


U_ROUND = 2.0 ** -53


def exact_dot(x, y):
    """the correctly rounded value of sum x_i y_i and sum |x_i y_i|: every product as rounded value + rounding error (Veltkamp / Dekker)"""
    def split(a):
        c = 134217729.0 * a
        hi = c - (c - a)
        return hi, a - hi
    p = x * y
    xh, xl = split(x)
    yh, yl = split(y)
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return math.fsum(np.concatenate([p, e])), math.fsum(np.abs(p))


def gamma(n):
    """gamma_n = n u / (1 - n u): the bound of a sum of n terms in any order"""
    return n * U_ROUND / (1.0 - n * U_ROUND)


def norm_bound(n, root):
    """|s - sqrt(exact)| of a computed 2-norm of length n: gamma_n on the sum of squares through the square root, one rounding for the
    library's sqrt and one for the reference's (the bound of tests/test_gpu_vec_algebra.py)"""
    return (gamma(n) / 2 + gamma(n) ** 2 + 2 * U_ROUND) * root


def dot_reversed(a, b):
    """the same products added from the far end, one by one in chunks: another summation order than np.dot's"""
    return float(np.sum((a * b)[::-1].reshape(-1)))


def dot_pairwise_chunks(a, b, chunk=37):
    """partial sums over chunks of 37 added in order: the shape of a slab reduction"""
    q = a * b
    return float(sum(float(np.sum(q[i:i + chunk])) for i in range(0, q.size, chunk)))


ORDERS = (("np.dot", np.dot), ("from the far end", dot_reversed), ("chunks", dot_pairwise_chunks))


def count_window(counts):
    """(lo, hi, m) of a loop's iteration counts in several summation orders: rounding alone moves the count between lo and hi, so another
    order is held to [lo - m, hi + m] with m = max(1, hi - lo)"""
    lo, hi = min(counts), max(counts)
    return lo, hi, max(1, hi - lo)


def head_deviation(hist, ref, first=1, last=5):
    """the largest relative deviation of entries first .. last of a history from the reference's (over the entries both have)"""
    m = min(len(hist), len(ref), last + 1)
    if m <= first:
        return 0.0
    h, r = np.asarray(hist[first:m]), np.asarray(ref[first:m])
    return float((np.abs(h - r) / np.abs(r)).max())


def corner_dofs(nodes, dof=1):
    """the dofs of the eight corner nodes of a box of nodes[0] x nodes[1] x nodes[2] nodes, axis 0 fastest, dof entries per node"""
    n0, n1, n2 = nodes
    at = [i + n0 * (j + n1 * k) for k in (0, n2 - 1) for j in (0, n1 - 1) for i in (0, n0 - 1)]
    return np.array([a * dof + f for a in at for f in range(dof)])


ALL6 = [(d, s) for d in range(3) for s in range(2)]
# the problems of tests/test_gpu_krylov_lengths.py that tests/test_krylov_abi.py also runs on the oracle's matrix:
# n -> (form, dof, p, N, Dirichlet values (axis, side, field, value)); identity geometry
SMALL_LENGTHS = {
    175: ("poisson", 1, 2, (5, 3, 3), [(d, s, 0, 0.0) for d, s in ALL6]),
    1025: ("poisson", 1, 2, (3, 3, 39), [(d, s, 0, 0.0) for d, s in ALL6]),
    1029: ("elasticity", 3, 2, (5, 5, 5), [(0, 0, 0, 0.0), (0, 0, 1, 0.0), (0, 0, 2, 0.0), (0, 1, 0, 0.0)]),
}


def x_true(n):
    """the fixed random solution of the length: b is the operator's action on it"""
    return np.random.default_rng(n).standard_normal(n)


def cg(op, prec, b, x0=None, rtol=1e-10, atol=0.0, maxit=None, dot=np.dot):
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=float)
    maxit = b.size if maxit is None else maxit
    bnorm = np.sqrt(dot(b, b))
    if bnorm == 0.0:
        return np.zeros_like(b), _info(0, CONVERGED_ATOL, [0.0], 0.0)
    r = b - op(x)
    z = prec(r)
    p = z.copy()
    rz, its = dot(r, z), 0
    hist = [np.sqrt(dot(r, r))]
    while True:
        reason = _stop(hist[-1], bnorm, rtol, atol, its, maxit)
        if reason:
            break
        if _bad(rz):
            reason = DIVERGED_BREAKDOWN
            break
        Ap = op(p)
        pAp = dot(p, Ap)
        if not (pAp > 0.0) or not np.isfinite(pAp):
            reason = DIVERGED_BREAKDOWN
            break
        a = rz / pAp
        x += a * p
        r -= a * Ap
        z = prec(r)
        rz, rz_old = dot(r, z), rz
        p = z + (rz / rz_old) * p
        its += 1
        hist.append(np.sqrt(dot(r, r)))
    return x, _info(its, reason, hist, bnorm)


def bicgstab(op, prec, b, x0=None, rtol=1e-10, atol=0.0, maxit=None, dot=np.dot):
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=float)
    maxit = b.size if maxit is None else maxit
    bnorm = np.sqrt(dot(b, b))
    if bnorm == 0.0:
        return np.zeros_like(b), _info(0, CONVERGED_ATOL, [0.0], 0.0)
    # 1
    r = b - op(x)
    rhat = r.copy()
    rho = alpha = omega = 1.0
    v, p = np.zeros_like(b), np.zeros_like(b)
    its = 0
    hist = [np.sqrt(dot(r, r))]
    while True:
        reason = _stop(hist[-1], bnorm, rtol, atol, its, maxit)
        if reason:
            break
        rho1 = dot(rhat, r)                       # 2.1
        if _bad(rho1) or _bad(omega):
            reason = DIVERGED_BREAKDOWN
            break
        beta = (rho1 / rho) * (alpha / omega)     # 2.2
        p = r + beta * (p - omega * v)            # 2.3
        y = prec(p)                               # 2.4
        v = op(y)                                 # 2.5
        rhatv = dot(rhat, v)
        if _bad(rhatv):
            reason = DIVERGED_BREAKDOWN
            break
        alpha = rho1 / rhatv                      # 2.6
        s = r - alpha * v                         # 2.7
        z = prec(s)                               # 2.8
        t = op(z)                                 # 2.9
        tt = dot(t, t)
        if _bad(tt):
            reason = DIVERGED_BREAKDOWN
            break
        omega = dot(t, s) / tt                    # 2.10
        x += alpha * y + omega * z                # 2.11
        r = s - omega * t                         # 2.12
        rho = rho1
        its += 1
        hist.append(np.sqrt(dot(r, r)))           # 2.13: the one test of |r|, at the top of the loop
    return x, _info(its, reason, hist, bnorm)


def engine_callables(eng, op="matrix", pc="none", a=0.0, t=0.0, V=None, U=None):
    """(op(v), prec(v)) on the host from the engine's own operators, one host copy each way per call, the way tests/test_gpu_fast_diag.py drives
    its CG: the action named by `op` at the state (a, V, t, U), and 1 / D of the matching diagonal, the inverted point blocks of the matching
    block diagonal, IGXFastDiagApply (the caller has run fast_diag_setup) or the identity."""
    Xv, Yv = eng.create_vec(), eng.create_vec()

    def action(v):
        Xv.set(v)
        if op == "matrix":
            eng.compute_matrix_action(Xv, Yv)
        elif op == "jacobian":
            eng.compute_jacobian_action(U, Xv, Yv)
        else:
            eng.compute_ijacobian_action(a, V, t, U, Xv, Yv)
        eng.synchronize()
        return Yv.get().copy()

    if pc == "none":
        return action, (lambda v: v.copy())
    if pc == "jacobi":
        Dv = eng.create_vec()
        if op == "matrix":
            eng.compute_matrix_diagonal(Dv)
        elif op == "jacobian":
            eng.compute_jacobian_diagonal(U, Dv)
        else:
            eng.compute_ijacobian_diagonal(a, V, t, U, Dv)
        eng.synchronize()
        D = Dv.get().copy()
        return action, (lambda v: v / D)
    if pc == "pbjacobi":
        B = [eng.create_vec() for _ in range(eng.dof)]
        if op == "matrix":
            eng.compute_matrix_block_diagonal(B)
        elif op == "jacobian":
            eng.compute_jacobian_block_diagonal(U, B)
        else:
            eng.compute_ijacobian_block_diagonal(a, V, t, U, B)
        eng.block_diagonal_invert(B)

        def blocks(v):
            eng.block_diagonal_apply(B, Xv.set(v), Yv)
            eng.synchronize()
            return Yv.get().copy()
        return action, blocks

    def fast_diag(v):
        eng.fast_diag_apply(Xv.set(v), Yv)
        eng.synchronize()
        return Yv.get().copy()
    return action, fast_diag
