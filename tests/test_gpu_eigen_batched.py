"""IGXEigenSolve with IGXSetBatchedActions(stiff, 1) on the GPU: three of the eight solves of tests/test_gpu_eigen.py -- the cube at p = 2
with fast diagonalisation, p = 3 on the NURBS map with Jacobi, Elasticity with the three-field Mass and the point blocks -- with the
operators applied through the block actions (one call on stiff and one on mass per block in place of m single actions each), held to
that file's assertions with that file's helpers: Parlett's bound against eigh of the oracle's matrices, B-orthonormality, the returned
residuals, exact zeros on the fixed rows, the host loop's iteration count within ITERATION_MARGIN, bit-repeatability.
  launches   the count written down from the loop (test_gpu_eigen.py: test_launches_equal_the_count_derived_from_the_loop) with the m (a + b)
             launches of the single actions replaced by A + B, the launches of one block call of m columns on stiff and on mass
  actions    info.actions counts columns: it equals the flag-off solve's
  flag off   after IGXSetBatchedActions(stiff, 0) the solve is bit for bit, name for name and launch for launch the solve of an IGX that
             never saw the setter (test_gpu_eigen.py's own engines: nothing there calls it)
The engines of the batched solves are this file's own (test_gpu_eigen.problem, made once more), so the other file's stay untouched.
Every test prints what it sees before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import eigen_ref as E
import test_gpu_eigen as GE

pytestmark = pytest.mark.gpu
U = GE.U
BLOCK = GE.BLOCK
SOLVES = [("cube", "fastdiag"), ("nurbs-p3", "jacobi"), ("elasticity", "pbjacobi")]


@functools.lru_cache(maxsize=None)
def problem(name):
    return GE.problem.__wrapped__(name)


def solve(name, pc, flag):
    stiff, mass, _, _, _ = problem(name)
    stiff.set_batched_actions(flag)
    try:
        out = stiff.eigen(GE.nev_of(name), mass=mass, block=BLOCK, pc=pc, rtol=1e-8, maxit=300, history=True)
        kname, (_, _, launches) = stiff.kernel_name(), stiff.last_timing()
    finally:
        stiff.set_batched_actions(0)
    out["Xh"] = GE.host_of(out)
    return out, kname, launches


@functools.lru_cache(maxsize=None)
def batched(name, pc):
    return solve(name, pc, 1)


@pytest.mark.parametrize("name,pc", SOLVES)
def test_lowest_pairs_against_eigh_of_the_oracle(name, pc):
    stiff, mass, A, B, free = problem(name)
    nev, m = GE.nev_of(name), BLOCK
    out, kname, _ = batched(name, pc)
    off = GE.device(name, pc)[0]
    X, lam, its = out["Xh"], out["lambda"], out["iterations"]
    lam_ref, _ = E.dense_reference(A, B, free, m + 1)
    bound, rnorm = E.parlett_bounds(A, B, free, X, lam)
    err = np.abs(lam - lam_ref[:m])
    defect = E.orthonormality_defect(B, X)
    ax = np.array([np.linalg.norm(A @ X[:, j]) for j in range(m)])
    resid_dev = float((np.abs(out["resid"] - rnorm) / ax).max())
    resid_tol = 8 * (its + 1) * (3 * m + 2) * U
    ref = E.lobpcg(A, B, GE.start_block(A.shape[0]), nev, T=GE.engine_T(stiff, pc, A), rtol=1e-8, maxit=300, fixed=~free)
    print("%s, pc=%s, batched: %d iterations (host loop %d, flag off %d), reason %s, restarts %d, %d actions (flag off %d); lambda %s; |theta - lambda| %s; "
          "Parlett bounds %s; |X^T B X - I| %.3e; resid against the recomputed one / |A x| %.3e (tolerance %.3e); lambda equal to the flag-off solve's bit for bit: %s; %s"
          % (name, pc, its, ref["iterations"], off["iterations"], out["reason_name"], out["restarts"], out["actions"], off["actions"], np.array2string(lam[:nev], precision=8),
             np.array2string(err[:nev], precision=2), np.array2string(bound[:nev], precision=2), defect, resid_dev, resid_tol, np.array_equal(lam, off["lambda"]), kname))
    assert out["reason"] == E.CONVERGED == ref["reason"] and out["nconverged"] == nev
    assert lam_ref[nev] - lam_ref[nev - 1] > 1e-3 * lam_ref[nev], "nev does not cut in a spectral gap"
    assert np.all(err[:nev] <= bound[:nev] + 64 * U * np.abs(lam_ref[:nev]))
    assert np.all(np.diff(lam) >= 0) and defect <= GE.ORTHO_TOL
    assert resid_dev <= resid_tol
    assert not X[~free].any(), "a fixed row is not exactly zero"
    assert out["history"].shape == (its + 1, m) and np.array_equal(out["history"][-1], out["resid"])
    assert np.all(out["resid"][:nev] <= 1e-8 * ax[:nev] * (1 + 1e-6))
    assert out["actions"] == 2 * m * (its + 1) and out["actions"] == off["actions"]
    assert abs(its - ref["iterations"]) <= GE.ITERATION_MARGIN
    assert kname.startswith("eigen(lobpcg, block %d, pc=%s, vec_sumfact(matrix action on a block: " % (m, pc)) and kname.endswith(", %d iterations)" % its), kname


@pytest.mark.parametrize("name,pc", SOLVES)
def test_a_batched_solve_is_bit_repeatable(name, pc):
    first = batched(name, pc)[0]
    again = solve(name, pc, 1)[0]
    assert np.array_equal(first["lambda"], again["lambda"]) and np.array_equal(first["history"], again["history"])
    assert np.array_equal(first["Xh"], again["Xh"]) and first["iterations"] == again["iterations"]


@pytest.mark.parametrize("name,pc", SOLVES)
def test_launches_equal_the_count_derived_from_the_loop(name, pc):
    """test_gpu_eigen.py's derivation with m (a + b) replaced by A + B, the launches of one block call of m columns on stiff and on mass:
      set-up and step 0   m z + D + (A + B) + 2 x 2 (two IGXVecMDot) + 3 IGXVecMAXPY
      every pass          2 (bv_resid, bv_record): its + 1 passes
      every iteration     m t + (A + B) + 2 x 2 + 6 IGXVecMAXPY"""
    stiff, mass, _, _, _ = problem(name)
    out, _, launches = batched(name, pc)
    m, its = BLOCK, out["iterations"]
    xs, ys = [stiff.create_vec() for _ in range(m)], [stiff.create_vec() for _ in range(m)]
    stiff.compute_matrix_action_block(xs, ys)
    a = stiff.last_timing()[2]
    mass.compute_matrix_action_block([mass.create_vec() for _ in range(m)], [mass.create_vec() for _ in range(m)])
    b = mass.last_timing()[2]
    c = stiff.coloring()
    assert a == b == c[0] * c[1] * c[2]
    D = t = 0
    if pc == "jacobi":
        stiff.compute_matrix_diagonal(ys[0])
        D, t = stiff.last_timing()[2], 1
    elif pc == "pbjacobi":
        cols = [stiff.create_vec() for _ in range(stiff.dof)]
        stiff.compute_matrix_block_diagonal(cols)
        D = stiff.last_timing()[2] + 1
        t = 1
    elif pc == "fastdiag":
        stiff.fast_diag_apply(xs[0], ys[0])
        t = stiff.last_timing()[2]
    count = m * 1 + D + (a + b) + 4 + 3 + 2 * (its + 1) + its * (m * t + (a + b) + 4 + 6)
    off = GE.device(name, pc)
    print("%s, pc=%s, batched: %d launches reported, %d derived (m = %d, its = %d, A = %d, B = %d, D = %d, t = %d); flag off: %d launches in %d iterations"
          % (name, pc, launches, count, m, its, a, b, D, t, off[2], off[0]["iterations"]))
    assert launches == count


@pytest.mark.parametrize("name,pc", SOLVES)
def test_flag_off_is_the_solve_of_an_igx_that_never_saw_the_setter(name, pc):
    batched(name, pc)                                       # the flag has been on, and is off again
    out, kname, launches = solve(name, pc, 0)
    never, kname0, launches0 = GE.device(name, pc)
    assert kname == kname0 and launches == launches0 and "on a block" not in kname
    assert out["iterations"] == never["iterations"] and out["actions"] == never["actions"]
    assert np.array_equal(out["lambda"], never["lambda"]) and np.array_equal(out["history"], never["history"]) and np.array_equal(out["Xh"], never["Xh"])
