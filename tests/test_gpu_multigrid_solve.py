"""IGXMultigridSolve on the GPU (include/petiga_amd.h): IGXSolve's loop with the V-cycle as the preconditioner, by the rules of
tests/test_gpu_krylov_solve.py.  The yardstick of every run is the host loop -- krylov_ref's CG / BiCGStab with multigrid_ref's cycle on the
SAME engines' operators, lambda_l from IGXMultigridGetInfo -- from which the device differs by the summation order of its inner products
alone (the cycle itself is the same bits: tests/test_gpu_multigrid_cycle.py).  The reference of every solution is the CPU oracle's matrix.
  iteration counts   CG: within 1 of the host loop.  BiCGStab: within BICG_MARGIN.
  history            |r_k| of the first min(k, 5) steps agrees with the host loop's to HISTORY_RTOL
  true residual      |b - A_s x| <= max(2 rtol |b|, 8 x the host loop's own true residual)
  repeatability      two solves give the same bits in x and in the history
  the counts         the device run meets the count conditions of tests/test_multigrid_reference.py: flat in the mesh, at most half of Jacobi's
HISTORY_RTOL and BICG_MARGIN are measured on an MI355X: 8 x the largest relative deviation of a head entry and twice the largest deviation
of the count seen on these cases (DESIGN.md 3.19 holds the figures).  Every test prints what it sees before it asserts (run with -s).
Cases: Poisson on the parametric cube and on a NURBS map whose geometry on every level is geometry.refine of the coarsest net (p = 2 three
levels, p = 3 two levels; fast diagonalisation once as the coarse solve); elasticity (dof 3) with point blocks, 4^3 -> 8^3; the Bratu
Jacobian under BiCGStab with a state per level (the coarse one a coarse solution, the fine one its prolongation)."""
import ctypes as C
import functools

import numpy as np
import pytest

import krylov_ref as K
import multigrid_ref as M
import oracle_api as O
import transfer_ref as TR
from common import make_pair
from test_gpu_multigrid_cycle import ALL6, device_and_host, fixed_of, poisson_level

pytestmark = pytest.mark.gpu
RTOL = 1e-10
HISTORY_RTOL = 8 * 1.4e-13      # measured: the largest relative deviation of a head entry on the CG cases below is 1.389e-13 (p = 3, parametric cube; the others 8.4e-16 .. 1.2e-14)
BICG_MARGIN = 1                 # measured: the Bratu case takes 8 iterations on the device and in the host loop: twice the deviation seen is 0; one step is what a summation order moves (CG's rule)
FASTDIAG_X1 = dict(pc="fastdiag", maxit=0)


def _nets(p, Ns, seed=2, amp=0.05):
    """(X, W) per level of one NURBS map: a warped rational net on the coarsest knots, refined to every level by knot insertion"""
    from petiga_amd import geometry as G
    from common import warped_geometry
    orc, _ = make_pair(3, 1, p, list(Ns[0]), engine=False)
    X, W = warped_geometry(orc, 3, seed=seed, rational=True, amp=amp)
    shape = [Ns[0][d] + p for d in (2, 1, 0)]
    Pw = np.concatenate([X * W[:, None], W[:, None]], axis=1).reshape(shape + [4])
    knots = [TR.uniform_knots(p, Ns[0][d]) for d in range(3)]
    out = [(X, W)]
    for N in Ns[1:]:
        new = [np.setdiff1d(TR.uniform_knots(p, N[d]), knots[d]) for d in range(3)]
        knots, Pw = G.refine([p] * 3, knots, Pw, new)
        out.append(G.split_net(Pw))
    return out


@functools.lru_cache(maxsize=None)
def _poisson(p, Ns, nurbs):
    """(levels, right-hand side of the finest level, the oracle's matrix there)"""
    nets = _nets(p, Ns) if nurbs else [None] * len(Ns)
    levels = [poisson_level(p, N, geometry=g) for N, g in zip(Ns, nets)]
    orc, _ = make_pair(3, 1, p, list(Ns[-1]), engine=False)
    if nurbs:
        orc.set_geometry(*nets[-1])
    for d, s in ALL6:
        orc.set_boundary_value(d, s, 0, 0.0)
    A_o, _ = orc.compute_system("orc_form_poisson")
    fine = levels[-1]
    A, b = fine.create_mat(), fine.create_vec()
    fine.compute_system(A, b)
    fine.synchronize()
    rhs = b.get().copy()
    rhs.setflags(write=False)
    return levels, rhs, A_o.scipy().tocsr()


def _solve(mg, fine, rhs, x0=None, **kw):
    b, x = fine.create_vec().set(rhs), fine.create_vec()
    if x0 is not None:
        x.set(x0)
    info = mg.solve(b, x, history=True, **kw)
    return x.get().copy(), info


def _against_the_host_loop(label, mg, h, fine, rhs, A_s, loop, margin, rtol=RTOL, maxit=300, pin_history=True):
    method = "cg" if loop is K.cg else "bicgstab"
    rhs = np.array(rhs)
    x_ref, ref = loop(h.levels[-1].A, h.apply, rhs, rtol=rtol, maxit=maxit)
    x, info = _solve(mg, fine, rhs, method=method, rtol=rtol, maxit=maxit)
    name = fine.kernel_name()
    k, k_ref = info["iterations"], ref["iterations"]
    dev = K.head_deviation(info["history"], ref["history"])
    res, res_ref, bn = np.linalg.norm(rhs - A_s @ x), np.linalg.norm(rhs - A_s @ x_ref), np.linalg.norm(rhs)
    print("%s: %d iterations (host loop %d), reason %d; head of the history deviates by %.3e; true residual / |b| %.3e (host loop %.3e); %s"
          % (label, k, k_ref, info["reason"], dev, res / bn, res_ref / bn, name))
    assert info["reason"] == K.CONVERGED_RTOL == ref["reason"]
    assert abs(k - k_ref) <= margin
    assert info["history"].size == k + 1 and info["rnorm"] == info["history"][-1] and info["rnorm0"] == info["history"][0] and info["rnorm"] <= rtol * info["bnorm"]
    assert abs(info["bnorm"] - bn) <= 1e-14 * bn
    if pin_history:
        assert dev <= HISTORY_RTOL
    assert res <= max(2 * rtol * bn, 8 * res_ref)
    assert name.startswith("krylov(%s, pc=multigrid(%d levels, chebyshev-" % (method, len(h.levels))) and name.endswith(", %d iterations)" % k), name
    x2, info2 = _solve(mg, fine, rhs, method=method, rtol=rtol, maxit=maxit)
    assert np.array_equal(x, x2) and np.array_equal(info["history"], info2["history"]), "two solves differ"
    return info


@pytest.mark.parametrize("nurbs", [False, True], ids=["cube", "nurbs"])
@pytest.mark.parametrize("p,Ns", [(2, ((4, 4, 4), (8, 8, 8), (16, 16, 16))), (3, ((4, 4, 4), (8, 8, 8)))], ids=["p2", "p3"])
def test_cg_on_poisson(p, Ns, nurbs):
    levels, rhs, A_s = _poisson(p, Ns, nurbs)
    mg, h = device_and_host(levels, fixed_of(ALL6), FASTDIAG_X1)
    _against_the_host_loop("Poisson p = %d, %d levels, %s" % (p, len(Ns), "NURBS map" if nurbs else "parametric cube"), mg, h, levels[-1], rhs, A_s, K.cg, 1)
    mg.close()


def test_counts_are_flat_in_the_mesh_and_at_most_half_of_jacobi():
    """the count conditions of tests/test_multigrid_reference.py on the device: the parametric cube, all faces Dirichlet, a random right-hand
    side, fast diagonalisation (the exact inverse there) as the coarse solve"""
    counts = {}
    for p, Ns in ((2, ((4, 4, 4), (8, 8, 8))), (2, ((4, 4, 4), (8, 8, 8), (16, 16, 16))), (3, ((4, 4, 4), (8, 8, 8)))):
        levels, _, _ = _poisson(p, Ns, False)
        fine = levels[-1]
        levels[0].fast_diag_setup(0.0, [1.0, 1.0, 1.0])
        mg = fine.multigrid(levels[:-1], coarse=FASTDIAG_X1).setup()
        rhs = np.random.default_rng(0).standard_normal(fine.create_vec().n)
        _, info = _solve(mg, fine, rhs, rtol=RTOL, maxit=400)
        b, x = fine.create_vec().set(rhs), fine.create_vec()
        jac = fine.solve(b, x, pc="jacobi", rtol=RTOL, maxit=2000)
        print("p = %d, %d levels: MG-PCG %d iterations, Jacobi-PCG %d" % (p, len(Ns), info["iterations"], jac["iterations"]))
        assert info["reason"] == K.CONVERGED_RTOL == jac["reason"]
        counts[(p, len(Ns))] = (info["iterations"], jac["iterations"])
        mg.close()
    assert counts[(2, 3)][0] <= counts[(2, 2)][0] + 4
    for mg_its, jac_its in counts.values():
        assert 2 * mg_its <= jac_its


def test_cg_on_elasticity_with_point_blocks():
    from test_gpu_matrix_action import EL
    faces = [(0, 0), (0, 1)]
    Ns = ((4, 4, 4), (8, 8, 8))
    levels = [poisson_level(2, N, faces=faces, dof=3) for N in Ns]
    orc, _ = make_pair(3, 3, 2, list(Ns[-1]), engine=False)
    for d, s, f in fixed_of(faces, 3):
        orc.set_boundary_value(d, s, f, 0.0)
    A_s = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))[0].scipy().tocsr()
    for g in levels:
        g.set_form("elasticity", EL)
    mg, h = device_and_host(levels, fixed_of(faces, 3), dict(pc="pbjacobi", maxit=0), smoother="pbjacobi")
    rhs = np.random.default_rng(4).standard_normal(3000)
    _against_the_host_loop("elasticity p = 2, 4^3 -> 8^3, point blocks", mg, h, levels[-1], rhs, A_s, K.cg, 1)
    mg.close()


def test_bicgstab_on_the_bratu_jacobian_with_a_state_per_level():
    lam = 3.5
    Ns = ((4, 4, 4), (8, 8, 8))
    levels = [poisson_level(2, N) for N in Ns]
    for g in levels:
        g.set_form("bratu", (lam,))
    coarse, fine = levels
    Uc = coarse.create_vec()
    nl = coarse.solve_nonlinear(Uc, op="jacobian", method="cg", pc="jacobi", lin_rtol=1e-8, rtol=1e-10)
    assert nl["reason"] > 0, nl
    Uf = fine.create_vec()
    t = fine.transfer(coarse)
    t.prolong(Uc, Uf)
    fine.synchronize()
    t.close()
    assert np.abs(Uf.get()).max() > 1e-3
    orc, _ = make_pair(3, 1, 2, list(Ns[-1]), engine=False)
    for d, s in ALL6:
        orc.set_boundary_value(d, s, 0, 0.0)
    A_s = orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(lam), Uf.get()).scipy().tocsr()
    states = [dict(U=Uc), dict(U=Uf)]
    coarse.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    mg = fine.multigrid([coarse], op="jacobian", coarse=FASTDIAG_X1)
    for l, st in enumerate(states):
        mg.set_state(l, **st)
    mg.setup()
    h = M.engine_callables(levels, fixed_of(ALL6), op="jacobian", coarse=FASTDIAG_X1, states=states)
    h.setup(lambdas=[mg.info(l)["lambda_"] for l in range(2)])
    rhs = np.random.default_rng(41).standard_normal(fine.create_vec().n)
    _against_the_host_loop("Bratu Jacobian p = 2, 4^3 -> 8^3, BiCGStab", mg, h, fine, rhs, A_s, K.bicgstab, BICG_MARGIN, rtol=1e-9, pin_history=False)
    mg.close()


def test_zero_right_hand_side_and_maxit_zero():
    levels, rhs, _ = _poisson(3, ((4, 4, 4), (8, 8, 8)), False)
    fine = levels[-1]
    levels[0].fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    mg = fine.multigrid(levels[:-1], coarse=FASTDIAG_X1).setup()
    for method in ("cg", "bicgstab"):
        x, info = _solve(mg, fine, np.zeros(rhs.size), x0=np.ones(rhs.size), method=method)
        assert info["reason"] == K.CONVERGED_ATOL and info["iterations"] == 0 and not x.any() and info["rnorm"] == 0.0 and info["bnorm"] == 0.0
        x0 = 0.25 * np.ones(rhs.size)
        x, info = _solve(mg, fine, np.array(rhs), x0=x0, method=method, maxit=0)
        print("%s, maxit = 0: reason %d, |r0| = %.3e; %s" % (method, info["reason"], info["rnorm0"], fine.kernel_name()))
        assert info["reason"] == K.DIVERGED_ITS and info["iterations"] == 0 and info["history"].size == 1 and np.array_equal(x, x0)
        assert fine.kernel_name().startswith("krylov(%s, pc=multigrid(2 levels, chebyshev-jacobi 2, coarse fastdiag x1, vec_sumfact" % method)
        assert fine.kernel_name().endswith(", 0 iterations)")
    mg.close()
