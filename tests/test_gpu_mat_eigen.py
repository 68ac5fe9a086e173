"""IGXMatEigenSolve on the GPU (include/petiga_amd.h; the loop: eigen_loop in petiga_amd/csrc/solve_loops.hpp, shared with IGXEigenSolve; the
operators: IGXMatMultBlock) against scipy.linalg.eigh of the ORACLE's matrices on the free rows.  K and M are assembled by the engine.
  cases      the five of tests/test_gpu_eigen.py with its solves (cube with every pc, nurbs-p3 with Jacobi, periodic with fast
             diagonalisation, elasticity with point-block Jacobi, identity), and the two IGXEigenSolve refuses (asserted):
             membrane    dim 2, Poisson + Mass, p = 3, 6^2 elements, all four faces Dirichlet, nev 4, block 6, none and Jacobi
             rod         dim 1, p = 2, 12 elements, both ends fixed, nev 2, block 3 (3 m = 9 of 12 free rows), none
  per case   the checks of tests/test_gpu_eigen.py with the same derived bounds: Parlett's bound + 64 u lambda, nev in a spectral gap,
             max |X^T B X - I| <= 1e-10, the returned resid against the recomputed one within RESID_TOL, fixed rows exactly zero (the
             assembled K and M hold identity rows and zero columns there: asserted on the engine's own matrices)
  subspace   Davis-Kahan on the cube's triple eigenvalue
  iterations against tests/eigen_ref.py with Mat.mult as both operators and the engine's own T on the same start block.
             ITERATION_MARGIN = the largest deviation seen over the eleven solves on an MI355X plus one (both in profiles/mat_eigen.txt)
  also       bit-repeatable; a matrix-free IGXEigenSolve between two matrix solves with another pc; maxit = 0 and an unreachable rtol; two
             equal start columns; the launch count written down from the loop with L_A = the chunk count; M from the same IGX and from a
             second one give the same bits; fast diagonalisation on the membrane refused with the inner reason; the refusals that need
             vectors
Every test prints what it sees before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import eigen_ref as E
import mat_block_cases as MB
import test_gpu_eigen as GE
from common import make_pair

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
ARG_WRONG, ORDER, SUP = 62, 58, 56
ORTHO_TOL = 1e-10
ITERATION_MARGIN = 0 + 1      # measured on an MI355X (profiles/mat_eigen.txt): the largest |device - host loop| over the eleven solves below is 0 iterations
SOLVES = GE.SOLVES + [("membrane", "none"), ("membrane", "jacobi"), ("rod", "none")]


def shape(name):
    """(nev, block)"""
    return (MB.LOWDIM[name]["nev"], MB.LOWDIM[name]["block"]) if name in MB.LOWDIM else (GE.nev_of(name), GE.BLOCK)


def lowdim_engines(name):
    """(stiffness engine, mass engine) of the membrane or the rod, every face Dirichlet"""
    c = MB.LOWDIM[name]
    out = []
    for form in ("poisson", "mass"):
        _, eng = make_pair(c["dim"], 1, c["p"], list(c["N"]))
        for d in range(c["dim"]):
            for s in range(2):
                eng.set_boundary_value(d, s, 0, 0.0)
        eng.set_form(form)
        out.append(eng)
    return out


def assemble(eng):
    A = eng.create_mat()
    eng.compute_system(A, eng.create_vec())
    return A


@functools.lru_cache(maxsize=None)
def problem(name):
    """(stiffness engine, K, M or None, oracle A, oracle B or None, free mask): made once, never written to"""
    if name in MB.LOWDIM:
        stiff, mass = lowdim_engines(name)
        A, B, free, _ = MB.lowdim_oracle(name)
    else:
        stiff, mass, A, B, free = GE.problem(name)
    return stiff, assemble(stiff), assemble(mass) if mass is not None else None, A, B, free


def host_of(out):
    return np.column_stack([v.get() for v in out["X"]])


def start_block(n, m):
    return np.random.default_rng(0).standard_normal((m, n)).T.copy()


@functools.lru_cache(maxsize=None)
def device(name, pc):
    stiff, K, M, _, _, _ = problem(name)
    nev, m = shape(name)
    out = K.eigen(nev, mass=M, block=m, pc=pc, rtol=1e-8, maxit=300, history=True)
    name_, (_, _, launches) = stiff.kernel_name(), stiff.last_timing()
    out["Xh"] = host_of(out)
    out["Xh"].setflags(write=False)
    return out, name_, launches


def mat_operator(A):
    """x -> A x through Mat.mult, on vectors of the matrix's own IGX"""
    if A is None:
        return None
    x_, y_ = A.iga.create_vec(), A.iga.create_vec()

    def op(x):
        A.mult(x_.set(x), y_)
        return y_.get().copy()
    return op


def engine_T(stiff, K, pc):
    """the preconditioner of the host loop, read out of K as the solve reads it; the engine's own kernels apply it"""
    if pc == "none":
        return None
    r_, z_ = stiff.create_vec(), stiff.create_vec()
    if pc == "jacobi":
        d_ = stiff.create_vec()
        K.diagonal(d_)
        d = d_.get().copy()
        return lambda r: r / d
    if pc == "fastdiag":
        def T(r):
            stiff.fast_diag_apply(r_.set(r), z_)
            return z_.get().copy()
        return T
    cols = [stiff.create_vec() for _ in range(K.bs)]
    K.block_diagonal(cols)
    stiff.block_diagonal_invert(cols)

    def T(r):
        stiff.block_diagonal_apply(cols, r_.set(r), z_)
        return z_.get().copy()
    return T


@pytest.mark.parametrize("name,pc", SOLVES)
def test_lowest_pairs_against_eigh_of_the_oracle(name, pc):
    stiff, K, M, A, B, free = problem(name)
    nev, m = shape(name)
    out, kname, _ = device(name, pc)
    X, lam, its = out["Xh"], out["lambda"], out["iterations"]
    lam_ref, V = E.dense_reference(A, B, free, m + 1)
    bound, rnorm = E.parlett_bounds(A, B, free, X, lam)
    err = np.abs(lam - lam_ref[:m])
    defect = E.orthonormality_defect(B, X)
    ax = np.array([np.linalg.norm(A @ X[:, j]) for j in range(m)])
    resid_dev = float((np.abs(out["resid"] - rnorm) / ax).max())
    resid_tol = 8 * (its + 1) * (3 * m + 2) * U
    ref = E.lobpcg(mat_operator(K), mat_operator(M), start_block(A.shape[0], m), nev, T=engine_T(stiff, K, pc), rtol=1e-8, maxit=300, fixed=~free)
    print("%s, pc=%s: %d iterations (host loop %d: deviation %d), reason %s, restarts %d, %d actions; lambda %s; |theta - lambda| %s; Parlett bounds %s; "
          "|X^T B X - I| %.3e; resid against the recomputed one / |A x| %.3e (tolerance %.3e); %s"
          % (name, pc, its, ref["iterations"], abs(its - ref["iterations"]), out["reason_name"], out["restarts"], out["actions"], np.array2string(lam[:nev], precision=8),
             np.array2string(err[:nev], precision=2), np.array2string(bound[:nev], precision=2), defect, resid_dev, resid_tol, kname))
    assert out["reason"] == E.CONVERGED == ref["reason"] and out["nconverged"] == nev
    assert lam_ref[nev] - lam_ref[nev - 1] > 1e-3 * lam_ref[nev], "nev does not cut in a spectral gap"
    assert np.all(err[:nev] <= bound[:nev] + 64 * U * np.abs(lam_ref[:nev]))
    assert np.all(np.diff(lam) >= 0) and defect <= ORTHO_TOL
    assert resid_dev <= resid_tol
    assert not X[~free].any(), "a fixed row is not exactly zero"
    assert out["history"].shape == (its + 1, m) and np.array_equal(out["history"][-1], out["resid"])
    assert np.all(out["resid"][:nev] <= 1e-8 * ax[:nev] * (1 + 1e-6))
    assert out["actions"] == (2 if M is not None else 1) * m * (its + 1)
    assert abs(its - ref["iterations"]) <= ITERATION_MARGIN
    assert kname.startswith("eigen(lobpcg, block %d, pc=%s, mat_mult_block(bs=%d, " % (m, pc, K.bs)) and kname.endswith(", %d iterations)" % its), kname


@pytest.mark.parametrize("name", ["membrane", "rod", "elasticity"])
def test_fixed_rows_of_the_assembled_matrices_are_identity_rows_and_zero_columns(name):
    _, K, M, _, _, free = problem(name)
    for label, A in (("K", K), ("M", M)):
        rp, ci, val = A.host()
        bs = A.bs
        blocks = val.reshape(-1, bs, bs)
        row = np.repeat(np.arange(A.nbrows), np.diff(rp))
        ri = (row[:, None, None] * bs + np.arange(bs)[None, :, None]) + np.zeros((1, 1, bs), dtype=int)
        cj = (ci[:, None, None].astype(np.int64) * bs + np.arange(bs)[None, None, :]) + np.zeros((1, bs, 1), dtype=int)
        fixed_r, fixed_c = ~free[ri], ~free[cj]
        off = (fixed_r | fixed_c) & (ri != cj)
        diag = fixed_r & (ri == cj)
        print("%s, %s: %d fixed rows; %d stored entries in their rows and columns off the diagonal, all zero: %s; their diagonal: %s"
              % (name, label, (~free).sum(), off.sum(), not blocks[off].any(), np.unique(blocks[diag])))
        assert (~free).any() and diag.sum() == (~free).sum()
        assert not blocks[off].any() and np.all(blocks[diag] > 0)


@pytest.mark.parametrize("name", ["membrane", "rod"])
def test_the_matrix_free_solve_still_refuses_dim_1_and_2(name):
    import petiga_amd as P
    stiff, mass = lowdim_engines(name)
    nev, m = shape(name)
    with pytest.raises(P.IGXError) as e:
        stiff.eigen(nev, mass=mass, block=m)
    print(e.value)
    assert e.value.code == SUP and "IGXEigenSolve" in str(e.value)


def test_the_triple_eigenvalue_as_a_subspace():
    _, _, _, A, B, free = problem("cube")
    lam_ref, V = E.dense_reference(A, B, free, 6)
    assert abs(lam_ref[3] - lam_ref[1]) <= 1e-9 * lam_ref[1]
    for pc in ("none", "fastdiag"):
        out, _, _ = device("cube", pc)
        X, lam = out["Xh"], out["lambda"]
        bound, _ = E.parlett_bounds(A, B, free, X, lam)
        delta = min(lam_ref[4] - lam[3], lam[1] - lam_ref[0])
        angle = E.largest_principal_angle(B, X[:, 1:4], V[:, 1:4])
        limit = float(np.sqrt(np.sum(bound[1:4] ** 2)) / delta)
        print("cube, pc=%s: largest principal angle %.3e, Davis-Kahan bound %.3e (delta %.3f)" % (pc, angle, limit, delta))
        assert np.sin(angle) <= limit + 64 * U


def _same(a, b):
    return (np.array_equal(a["lambda"], b["lambda"]) and np.array_equal(a["history"], b["history"]) and a["iterations"] == b["iterations"]
            and np.array_equal(a["Xh"] if "Xh" in a else host_of(a), b["Xh"] if "Xh" in b else host_of(b)))


def test_a_solve_is_bit_repeatable_and_shares_its_store_with_the_matrix_free_solve():
    stiff, K, M, _, _, _ = problem("cube")
    mass = GE.problem("cube")[1]
    first, _, _ = device("cube", "jacobi")
    again = K.eigen(4, mass=M, block=GE.BLOCK, pc="jacobi", rtol=1e-8, maxit=300, history=True)
    assert _same(first, again)
    # a matrix-free solve with another pc between two matrix solves
    between = stiff.eigen(4, mass=mass, block=GE.BLOCK, pc="none", rtol=1e-8, maxit=300, history=True)
    third = K.eigen(4, mass=M, block=GE.BLOCK, pc="jacobi", rtol=1e-8, maxit=300, history=True)
    assert _same(first, third)
    fresh_stiff, fresh_mass = GE.problem.__wrapped__("cube")[:2]
    fresh = fresh_stiff.eigen(4, mass=fresh_mass, block=GE.BLOCK, pc="none", rtol=1e-8, maxit=300, history=True)
    print("cube: matrix solve %d iterations three times; the matrix-free solve between them %d iterations, a fresh engine's %d" % (first["iterations"], between["iterations"], fresh["iterations"]))
    assert _same(between, fresh)


def test_no_convergence_returns_the_reason():
    stiff, K, M, A, B, free = problem("cube")
    m = GE.BLOCK
    out = K.eigen(4, mass=M, block=m, maxit=0, history=True)
    print("maxit = 0: reason %s, %d iterations, %d actions, lambda %s" % (out["reason_name"], out["iterations"], out["actions"], np.array2string(out["lambda"][:4], precision=4)))
    assert out["reason"] == E.DIVERGED_ITS and out["iterations"] == 0 and out["history"].shape == (1, m) and out["actions"] == 2 * m
    X = host_of(out)
    assert E.orthonormality_defect(B, X) <= ORTHO_TOL and not X[~free].any()      # the Rayleigh-Ritz step on the start block has run
    out = K.eigen(4, mass=M, block=m, pc="jacobi", rtol=0.0, atol=0.0, maxit=5, history=True)
    print("rtol = 0: reason %s, %d iterations, nconverged %d" % (out["reason_name"], out["iterations"], out["nconverged"]))
    assert out["reason"] == E.DIVERGED_ITS and out["iterations"] == 5 and out["nconverged"] == 0 and out["history"].shape == (6, m)


def test_two_equal_start_columns():
    stiff, K, M, A, B, free = problem("cube")
    h = start_block(A.shape[0], GE.BLOCK)
    h[:, 3] = h[:, 1]
    X = [stiff.create_vec().set(h[:, j]) for j in range(GE.BLOCK)]
    out = K.eigen(4, mass=M, block=GE.BLOCK, X0=X, maxit=50)
    print("two equal start columns: reason %s after %d iterations, %d restarts" % (out["reason_name"], out["iterations"], out["restarts"]))
    assert out["reason"] == E.DIVERGED_BREAKDOWN or out["restarts"] >= 1
    assert np.all(np.isfinite(host_of(out)))


@pytest.mark.parametrize("name,pc", [("cube", "none"), ("cube", "jacobi"), ("cube", "fastdiag"), ("elasticity", "pbjacobi"), ("identity", "none"), ("membrane", "jacobi"), ("rod", "none")])
def test_launches_equal_the_count_derived_from_the_loop(name, pc):
    """m columns, its iterations; L_A, L_B: the chunk launches of one block product with K / with M (0 without M): the plan's count for
    (bs, m); z: 1 where the space has a Dirichlet face (mg_zero_fixed per start column); D: the launches that form T (the diagonal's copy; the
    block columns' copy and their inversion); t: launches of one application of T.
      set-up and step 0   m z + D + L_A + L_B + 2 x 2 (two IGXVecMDot) + (3 with M, else 2) IGXVecMAXPY
      every pass          2 (bv_resid, bv_record): its + 1 passes
      every iteration     m t + L_A + L_B + 2 x 2 + (6 with M, else 4) IGXVecMAXPY"""
    import petiga_amd as P
    stiff, K, M, _, _, _ = problem(name)
    out, _, launches = device(name, pc)
    (_, m), its = shape(name), out["iterations"]
    LA = len(P.mat_mult_block_plan(K.bs, m))
    assert LA == len(MB.plan(K.bs, m))
    LB = LA if M is not None else 0
    D = {"none": 0, "jacobi": 1, "pbjacobi": 2, "fastdiag": 0}[pc]
    t = {"none": 0, "jacobi": 1, "pbjacobi": 1}.get(pc)
    if pc == "fastdiag":
        stiff.fast_diag_apply(stiff.create_vec(), stiff.create_vec())
        t = stiff.last_timing()[2]
    nm = 3 if M is not None else 2
    count = m * 1 + D + LA + LB + 4 + nm + 2 * (its + 1) + its * (m * t + LA + LB + 4 + 2 * nm)
    print("%s, pc=%s: %d launches reported, %d derived (m = %d, its = %d, L_A = %d, L_B = %d, D = %d, t = %d)" % (name, pc, launches, count, m, its, LA, LB, D, t))
    assert launches == count


def test_mass_from_the_same_igx_and_from_a_second_one_give_the_same_bits():
    stiff, K, M2, _, _, _ = problem("membrane")
    nev, m = shape("membrane")
    eng = lowdim_engines("membrane")[0]
    K1 = assemble(eng)
    eng.set_form("mass")
    M1 = assemble(eng)
    eng.set_form("poisson")
    assert np.array_equal(K1.host(values_only=True), K.host(values_only=True)) and np.array_equal(M1.host(values_only=True), M2.host(values_only=True))
    one = K1.eigen(nev, mass=M1, block=m, pc="jacobi", rtol=1e-8, maxit=300, history=True)
    two, _, _ = device("membrane", "jacobi")
    print("membrane: M of the same IGX %d iterations, M of a second IGX %d" % (one["iterations"], two["iterations"]))
    assert one["reason"] == E.CONVERGED and _same(one, two)


def test_refusals_that_need_matrices():
    import petiga_amd as P
    stiff, K, M, _, _, _ = problem("cube")
    plain, Kp, Mp, _, _, _ = problem("elasticity")      # never set up for fast diagonalisation
    _, Km, Mm, _, _, _ = problem("membrane")
    m = GE.BLOCK
    X = [stiff.create_vec() for _ in range(m)]

    def refused(call, code, *words):
        with pytest.raises(P.IGXError) as e:
            call()
        print(e.value)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: K.eigen(4, mass=M, block=m, X0=X[:5]), ARG_WRONG, "IGXMatEigenSolve", "spec->block")
    refused(lambda: K.eigen(4, mass=M, block=m, X0=X[:5] + [None]), ARG_WRONG, "IGXMatEigenSolve", "null vector")
    refused(lambda: K.eigen(4, mass=M, block=m, X0=X[:5] + [plain.create_vec()], pc="fastdiag"), ARG_WRONG, "IGXMatEigenSolve", "another IGX")
    refused(lambda: K.eigen(4, mass=M, block=m, X0=X[:5] + [X[2]]), ARG_WRONG, "IGXMatEigenSolve", "twice")
    refused(lambda: K.eigen(4, mass=Mp, block=m, X0=X), ARG_WRONG, "IGXMatEigenSolve", "dof differs")
    refused(lambda: K.eigen(4, mass=Mm, block=m, X0=X), ARG_WRONG, "IGXMatEigenSolve", "dim differs")
    refused(lambda: Kp.eigen(3, mass=Mp, block=m, pc="fastdiag"), ORDER, "IGXFastDiagSetUp", "IGXMatEigenSolve")
    # fast diagonalisation's own refusal, under the solve's prefix
    refused(lambda: Km.eigen(4, mass=Mm, block=m, pc="fastdiag"), SUP, "IGXMatEigenSolve: the eigen solve on the stored matrices takes its preconditioner", ", and fast diagonalisation needs dim = 3")
    # two ranks on an axis
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.set_comm(2, 0)
    g.setup()
    Kg = g.create_mat()
    refused(lambda: Kg.eigen(2, block=3), SUP, "IGXMatEigenSolve", "one rank")
    out = K.eigen(4, mass=M, block=m, X0=X, maxit=0)      # a refused call leaves nothing behind (a zero start block: a breakdown, not an error)
    assert out["reason"] == E.DIVERGED_BREAKDOWN
