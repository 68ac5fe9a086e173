"""IGXSolve on the GPU (include/petiga_amd.h; petiga_amd/csrc/krylov.hpp): CG and right-preconditioned BiCGStab on the matrix-free actions,
everything resident on the device.  The yardstick of every run is the host loop of tests/krylov_ref.py on the SAME engine operators (one
host copy each way per product, krylov_ref.engine_callables): the two differ by the summation order of their inner products alone.  The
reference of every solution is the CPU oracle's matrix of the same operator: spsolve, or the true residual |b - A_s x|.
  iteration counts   CG: within 1 of the host loop (another summation order moves a crossing of the threshold by one step at the most on
                     these cases: tests/test_krylov_abi.py runs the loops in two orders on the CPU).  BiCGStab: within BICG_MARGIN.
  history            |r_k| of the first min(k, 5) steps agrees with the host loop's to HISTORY_RTOL (rounding differences grow along the
                     recurrence, so only the head is pinned).
  true residual      |b - A_s x| <= max(2 rtol |b|, 8 x the host loop's own true residual)
  repeatability      two solves give the same bits in x and in the history
HISTORY_RTOL and BICG_MARGIN are measured: 8 x the largest relative deviation of the head and twice the largest deviation of the count seen
on these cases on an MI355X (DESIGN.md 3.12 holds the figures); every test prints what it sees before it asserts (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import krylov_ref as K
import oracle_api as O
from common import make_pair, warped_geometry
from test_gpu_matrix_action import CASES, CH, DT, EL, NS
from test_gpu_matrix_action import _pair as action_pair
from test_gpu_matrix_action import _reference as action_reference

pytestmark = pytest.mark.gpu

ALL6 = [(d, s) for d in range(3) for s in range(2)]
RTOL = 1e-10
HISTORY_RTOL = 8 * 2.3e-15      # measured: the largest relative deviation of a head entry on the CG cases below is 2.23e-15 (p = 3, fast diagonalisation)
BICG_MARGIN = 8                 # measured: NS-VMS 91 against the restatement's 95, Bratu 73 against 69: the largest deviation is 4


def _true_residual(A_s, b, x):
    return np.linalg.norm(b - A_s @ x)


def _solve(eng, rhs, x0=None, **kw):
    b, x = eng.create_vec().set(rhs), eng.create_vec()
    if x0 is not None:
        x.set(x0)
    info = eng.solve(b, x, history=True, **kw)
    return x.get().copy(), info


# ---- 1. the exact inverse
def test_poisson_with_its_exact_inverse_takes_two_iterations_at_the_most():
    import scipy.sparse.linalg as spla
    orc, eng = make_pair(3, 1, 3, [5, 4, 3])
    for g in (orc, eng):
        for d, s in ALL6:
            g.set_boundary_value(d, s, 0, 0.25)
    eng.set_form("poisson")
    A, bv = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, bv)
    eng.synchronize()
    rhs = bv.get().copy()
    A_o, b_o = orc.compute_system("orc_form_poisson")
    want = spla.spsolve(A_o.scipy().tocsc(), np.asarray(b_o))
    assert eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0]) == 0
    op, prec = K.engine_callables(eng, pc="fastdiag")
    x_ref, ref = K.cg(op, prec, rhs, rtol=RTOL)
    x, info = _solve(eng, rhs, pc="fastdiag", rtol=RTOL, maxit=20)
    e, e_ref = np.abs(x - want).max() / np.abs(want).max(), np.abs(x_ref - want).max() / np.abs(want).max()
    print("exact inverse: %d iterations (host loop %d), reason %d; max|x - spsolve| / max|x| = %.3e (host loop %.3e); %s"
          % (info["iterations"], ref["iterations"], info["reason"], e, e_ref, eng.kernel_name()))
    assert info["reason"] == K.CONVERGED_RTOL and info["iterations"] <= 2
    assert e <= max(8 * e_ref, 1e-13)
    assert eng.kernel_name().startswith("krylov(cg, pc=fastdiag, vec_sumfact") and eng.kernel_name().endswith("%d iterations)" % info["iterations"])


# ---- 2. NURBS-mapped Poisson
@functools.lru_cache(maxsize=None)
def _nurbs_poisson(p, N):
    """(engine, right-hand side, the oracle's matrix): the cases of tests/test_gpu_fast_diag.py's CG run; made once, never written to"""
    orc, eng = make_pair(3, 1, p, list(N))
    X, W = warped_geometry(orc, 3, seed=2, rational=True, amp=0.05)
    for g in (orc, eng):
        g.set_geometry(X, W)
        for d, s in ALL6:
            g.set_boundary_value(d, s, 0, 0.0)
    eng.set_form("poisson")
    A, b = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, b)
    eng.synchronize()
    rhs = b.get().copy()
    rhs.setflags(write=False)
    A_o, _ = orc.compute_system("orc_form_poisson")
    eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    return eng, rhs, A_o.scipy().tocsr()


def _against_the_host_loop(label, eng, rhs, A_s, loop, margin, rtol=RTOL, maxit=400, **kw):
    method = "cg" if loop is K.cg else "bicgstab"
    state = {k: kw[k] for k in ("a", "t", "V", "U") if k in kw}
    op, prec = K.engine_callables(eng, op=kw.get("op", "matrix"), pc=kw["pc"], **state)
    rhs = np.array(rhs)
    x_ref, ref = loop(op, prec, rhs, rtol=rtol, maxit=maxit)
    x, info = _solve(eng, rhs, method=method, rtol=rtol, maxit=maxit, **kw)
    name = eng.kernel_name()
    k, k_ref = info["iterations"], ref["iterations"]
    m = min(k, k_ref, 5)
    dev = np.abs(info["history"][:m + 1] - ref["history"][:m + 1]) / ref["history"][:m + 1]
    res, res_ref, bn = _true_residual(A_s, rhs, x), _true_residual(A_s, rhs, x_ref), np.linalg.norm(rhs)
    print("%s: %d iterations (host loop %d), reason %d; head of the history deviates by %.3e; true residual / |b| %.3e (host loop %.3e); %s"
          % (label, k, k_ref, info["reason"], dev.max(), res / bn, res_ref / bn, name))
    assert info["reason"] == K.CONVERGED_RTOL == ref["reason"]
    assert abs(k - k_ref) <= margin
    assert info["history"].size == k + 1 and info["rnorm"] == info["history"][-1] and info["rnorm0"] == info["history"][0] and info["rnorm"] <= rtol * info["bnorm"]
    assert abs(info["bnorm"] - bn) <= 1e-14 * bn
    if loop is K.cg:
        assert dev.max() <= HISTORY_RTOL
    assert res <= max(2 * rtol * bn, 8 * res_ref)
    assert name.startswith("krylov(%s, pc=%s, vec_sumfact" % (method, kw["pc"])) and name.endswith(", %d iterations)" % k), name
    return x, info


@pytest.mark.parametrize("pc", ["none", "jacobi", "fastdiag"])
@pytest.mark.parametrize("p,N", [(3, (5, 4, 3)), (2, (8, 8, 8))])
def test_cg_on_nurbs_mapped_poisson(p, N, pc):
    eng, rhs, A_s = _nurbs_poisson(p, N)
    x, info = _against_the_host_loop("p = %d %s, pc %s" % (p, N, pc), eng, rhs, A_s, K.cg, 1, pc=pc)
    x2, info2 = _solve(eng, rhs, pc=pc, rtol=RTOL, maxit=400)
    assert np.array_equal(x, x2) and np.array_equal(info["history"], info2["history"]), "two solves differ"


def test_initial_guess_and_timing():
    eng, rhs, A_s = _nurbs_poisson(2, (8, 8, 8))
    x, info = _solve(eng, rhs, pc="fastdiag", rtol=RTOL)
    eng.set_timing(True)
    x2, info2 = _solve(eng, rhs, x0=x, pc="fastdiag", rtol=1e-6)
    total, kernel, launches = eng.last_timing()
    eng.set_timing(False)
    print("restart from the solution: %d iterations, |r0| / |b| = %.3e; last solve %.3f ms, operators %.3f ms, %d launches" % (info2["iterations"], info2["rnorm0"] / info2["bnorm"], total, kernel, launches))
    assert info2["iterations"] == 0 and info2["reason"] == K.CONVERGED_RTOL and np.array_equal(x2, x)
    assert info2["rnorm0"] <= 1e-8 * info2["bnorm"]
    assert total > 0 and 0 < kernel <= total and launches >= 3


# ---- 3. elasticity, dof 3
@functools.lru_cache(maxsize=None)
def _elasticity():
    orc, eng = make_pair(3, 3, 2, [4, 3, 3])
    for g in (orc, eng):
        for f in range(3):
            g.set_boundary_value(0, 0, f, 0.0)
        g.set_boundary_value(0, 1, 0, 0.1)
    eng.set_form("elasticity", EL)
    A, b = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, b)
    eng.synchronize()
    rhs = b.get().copy()
    rhs.setflags(write=False)
    A_o, _ = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))
    return eng, rhs, A_o.scipy().tocsr()


@pytest.mark.parametrize("pc", ["pbjacobi", "jacobi"])
def test_cg_on_elasticity(pc):
    eng, rhs, A_s = _elasticity()
    assert rhs.size == 450
    _against_the_host_loop("elasticity p = 2 (4, 3, 3), pc %s" % pc, eng, rhs, A_s, K.cg, 1, pc=pc, maxit=450)


# ---- 4. BiCGStab on nonsymmetric operators
@functools.lru_cache(maxsize=None)
def _nonsymmetric(name):
    """(engine, state keywords, right-hand side, the oracle's Jacobian) of a case of tests/test_gpu_matrix_action.py"""
    form = CASES[name][0]
    orc, eng = action_pair(name)
    _, U, V = action_reference(name)[:3]
    if form == "bratu":
        A_o = orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(3.5), U)
        eng.set_form("bratu", (3.5,))
        state = dict(op="jacobian", U=eng.create_vec().set(U))
    else:
        A_o = orc.compute_ijacobian("orc_form_ns_tangent", O.NSVMSCtx(*NS), 2.0 / DT, V, 0.0, U)
        eng.set_form("nsvms", NS)
        state = dict(op="ijacobian", a=2.0 / DT, t=0.0, V=eng.create_vec().set(V), U=eng.create_vec().set(U))
    A_s = A_o.scipy().tocsr()
    rhs = np.random.default_rng(41).standard_normal(A_s.shape[0])
    rhs.setflags(write=False)
    return eng, state, rhs, A_s


@pytest.mark.parametrize("name,pc", [("nsvms-p2", "pbjacobi"), ("bratu-p3", "jacobi")])
def test_bicgstab_on_a_nonsymmetric_operator(name, pc):
    eng, state, rhs, A_s = _nonsymmetric(name)
    assert abs(A_s - A_s.T).max() > 1e-6 * abs(A_s).max() or name == "bratu-p3"
    x, info = _against_the_host_loop("%s, pc %s" % (name, pc), eng, rhs, A_s, K.bicgstab, BICG_MARGIN, rtol=1e-9, pc=pc, **state)
    x2, info2 = _solve(eng, rhs, method="bicgstab", rtol=1e-9, maxit=400, pc=pc, **state)
    assert np.array_equal(x, x2) and np.array_equal(info["history"], info2["history"]), "two solves differ"


# ---- 5. outcomes
def test_maxit_one_gives_the_host_loops_first_iterate():
    eng, rhs, A_s = _nurbs_poisson(3, (5, 4, 3))
    op, prec = K.engine_callables(eng, pc="jacobi")
    rhs = np.array(rhs)
    x_ref, ref = K.cg(op, prec, rhs, rtol=RTOL, maxit=1)
    x, info = _solve(eng, rhs, pc="jacobi", rtol=RTOL, maxit=1)
    assert info["reason"] == K.DIVERGED_ITS == ref["reason"] and info["iterations"] == 1 and info["history"].size == 2
    # x = alpha p with alpha = r.z / p.Ap and the same p and A p bit for bit (the same kernels on the same input).  Either loop's r.z
    # (positive terms) is within gamma_n of the exact value and its p.Ap within gamma_n sum|p_i Ap_i| / |p.Ap| (the dot product's bound of
    # tests/test_gpu_vec_algebra.py); the quotient and the product alpha p round once each on either side
    n, u = rhs.size, 2.0 ** -53
    p = prec(rhs)
    Ap = op(p)
    gamma = n * u / (1 - n * u)
    bound = (2 * gamma * (1 + np.abs(p * Ap).sum() / abs(p @ Ap)) + 4 * u) * np.abs(x_ref)
    print("first iterate: max|x - x_ref| / bound = %.3f" % (np.abs(x - x_ref) / np.maximum(bound, 1e-300)).max())
    assert np.all(np.abs(x - x_ref) <= bound)


def test_zero_right_hand_side():
    eng, rhs, _ = _nurbs_poisson(3, (5, 4, 3))
    for method in ("cg", "bicgstab"):
        x, info = _solve(eng, np.zeros(rhs.size), x0=np.ones(rhs.size), method=method, pc="jacobi")
        assert info["reason"] == K.CONVERGED_ATOL and info["iterations"] == 0 and not x.any() and info["rnorm"] == 0.0 and info["bnorm"] == 0.0


def test_refusals_and_a_covered_solve_after_them():
    import petiga_amd as P
    # Cahn-Hilliard's IJacobian: the action covers it, the diagonal does not, and its reason passes through
    orc, eng = action_pair("ch-p2")
    _, U, V = action_reference("ch-p2")[:3]
    eng.set_form("cahnhilliard", CH)
    state = dict(op="ijacobian", a=250.0, t=0.0, V=eng.create_vec().set(V), U=eng.create_vec().set(U))
    b, x = eng.create_vec().set(np.random.default_rng(3).standard_normal(U.size)), eng.create_vec()
    with pytest.raises(P.IGXError) as e:
        eng.solve(b, x, pc="jacobi", **state)
    assert e.value.code == 56 and "second-order" in str(e.value) and "Krylov solve" in str(e.value), str(e.value)
    with pytest.raises(P.IGXError) as e:
        eng.solve(b, x, pc="fastdiag", **state)
    assert e.value.code == 58 and "IGXFastDiagSetUp" in str(e.value)
    with pytest.raises(P.IGXError) as e:
        eng.solve(b, b, **state)
    assert e.value.code == 62
    with pytest.raises(P.IGXError) as e:
        eng.solve(b, x, op="ijacobian", a=250.0, U=state["U"])      # V missing
    assert e.value.code == 62
    with pytest.raises(P.IGXError) as e:
        eng.solve(b, x, pc="none", op="ijacobian", a=250.0, V=state["V"], U=x)
    assert e.value.code == 62
    _, other = make_pair(3, 1, 2, [4, 4, 4])
    with pytest.raises(P.IGXError) as e:
        eng.solve(b, other.create_vec(), **state)
    assert e.value.code == 62
    # the action itself is covered: an unpreconditioned solve runs (the operator is not SPD: whatever CG makes of it, it reports) ...
    info = eng.solve(b, x, method="bicgstab", pc="none", rtol=1e-6, maxit=300, **state)
    print("Cahn-Hilliard IJacobian, BiCGStab without a preconditioner: %d iterations, reason %d; %s" % (info["iterations"], info["reason"], eng.kernel_name()))
    assert eng.kernel_name().startswith("krylov(bicgstab, pc=none, vec_sumfact")
    info = eng.solve(b, x, method="cg", pc="none", rtol=1e-6, maxit=5, **state)
    assert info["reason"] in (K.CONVERGED_RTOL, K.DIVERGED_ITS, K.DIVERGED_BREAKDOWN)
    # ... and after a refused solve on the Poisson engine a covered one reports its own kernel
    eng, rhs, A_s = _nurbs_poisson(3, (5, 4, 3))
    bv, xv = eng.create_vec().set(np.array(rhs)), eng.create_vec()
    with pytest.raises(P.IGXError):
        eng.solve(bv, bv)
    eng.set_kernel(1)
    with pytest.raises(P.IGXError) as e:
        eng.solve(bv, xv)
    assert e.value.code == 56 and "Krylov solve" in str(e.value) and "IGXSetKernel" in str(e.value)
    eng.set_kernel(0)
    info = eng.solve(bv, xv, pc="jacobi", rtol=RTOL)
    assert info["reason"] == K.CONVERGED_RTOL and eng.kernel_name().startswith("krylov(cg, pc=jacobi, vec_sumfact")
