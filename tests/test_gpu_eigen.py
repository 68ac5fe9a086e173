"""IGXEigenSolve on the GPU (include/petiga_amd.h; the host loop: petiga_amd/csrc/solve_loops.hpp, its sweeps: block_vec.hpp) against
scipy.linalg.eigh of the ORACLE's matrices on the free rows.
  cases      cube        Poisson + Mass, p = 2, 6^3 elements, all faces Dirichlet, nev 4, block 6, every pc (the triple second eigenvalue)
             nurbs-p3    p = 3, 5^3 elements on the warped rational map of the multigrid tests, Jacobi
             periodic    p = 2, 6^3, axis 1 periodic, Dirichlet on the faces of axes 0 and 2, nev 3 (1 + a pair, then a gap), fast diagonalisation
             elasticity  Elasticity + three-field Mass, p = 2, 4^3, mixed faces per field, point-block Jacobi
             identity    mass = NULL against eigh(A) on the cube
  per case   |theta_k - lambda_k| <= |B^-1/2 r_k| / |B^1/2 x_k| in sorted order (Parlett's residual bound, r_k recomputed from the oracle's
             matrices; + 64 u lambda_k for the reference's own rounding), nev cutting in a spectral gap (asserted);
             max |X^T B X - I| <= 1e-10 (the CPU test's bound); the returned resid equals the recomputed |r_k| within RESID_TOL |A x_k|,
             RESID_TOL = 8 (its + 1) (3 m + 2) u: AX and BX are carried through its + 1 updates of at most 3 m + 2 roundings per entry each,
             and 8 allows for the growth |S| |C| / |S C| of a scaled Gram basis; fixed rows exactly zero
  subspace   the triple eigenvalue's Ritz vectors span the reference's eigenspace: sin(largest principal angle) <= |R|_F / delta
             (Davis-Kahan, delta the distance of the Ritz cluster to the rest of the spectrum)
  iterations against tests/eigen_ref.py on the same start block with the oracle's matrices (and the engine's own T for the point blocks and
             the fast diagonalisation).  The Gram sums round differently on the device.  ITERATION_MARGIN = the largest deviation seen over
             the cases on an MI355X plus one (both in profiles/eigen.txt)
  also       fast diagonalisation takes strictly fewer iterations than no preconditioner on the cube; a solve is bit-repeatable; maxit = 0
             and an unreachable rtol return 0 with IGX_EIGEN_DIVERGED_ITS; two equal start columns end in a breakdown or a restart;
             IGXGetLastTiming's launches equal the count written down from the loop; the kernel name; the refusals that need vectors
Every test prints what it sees before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import eigen_ref as E
import multigrid_ref as M
from common import make_pair, warped_geometry

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
ARG_WRONG, ORDER = 62, 58
ORTHO_TOL = 1e-10
ITERATION_MARGIN = 0 + 1      # measured on an MI355X: the largest |device - host loop| over the eight solves below is 0 iterations
EL = (1.7, 0.6)
ALL = [(d, s) for d in range(3) for s in range(2)]
CASES = {
    "cube": dict(dof=1, p=2, N=(6, 6, 6), fixed=[(d, s, 0) for d, s in ALL], nev=4),
    "nurbs-p3": dict(dof=1, p=3, N=(5, 5, 5), fixed=[(d, s, 0) for d, s in ALL], nev=4, nurbs=True),
    "periodic": dict(dof=1, p=2, N=(6, 6, 6), periodic=(1,), fixed=[(d, s, 0) for d in (0, 2) for s in range(2)], nev=3),
    "elasticity": dict(dof=3, p=2, N=(4, 4, 4), fixed=[(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (1, 1, 1), (2, 0, 2)], nev=3, form="elasticity"),
}
BLOCK = 6
SOLVES = [("cube", "none"), ("cube", "jacobi"), ("cube", "pbjacobi"), ("cube", "fastdiag"), ("nurbs-p3", "jacobi"), ("periodic", "fastdiag"),
          ("elasticity", "pbjacobi"), ("identity", "none")]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(stiff engine, mass engine or None, oracle A, oracle B or None, free mask): made once, never written to"""
    import oracle_api as O
    c = CASES["cube" if name == "identity" else name]
    periodic = [i in c.get("periodic", ()) for i in range(3)]
    engines, mats, nodes = [], [], None
    for form in (c.get("form", "poisson"), "mass"):
        orc, eng = make_pair(3, c["dof"], c["p"], list(c["N"]), periodic=periodic)
        if c.get("nurbs"):
            X, W = warped_geometry(orc, 3, seed=2, rational=True, amp=0.05)
            orc.set_geometry(X, W)
            eng.set_geometry(X, W)
        for d, s, f in c["fixed"]:
            orc.set_boundary_value(d, s, f, 0.0)
            eng.set_boundary_value(d, s, f, 0.0)
        if form == "elasticity":
            eng.set_form("elasticity", EL)
            A, _ = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))
        else:
            eng.set_form(form)
            A, _ = orc.compute_system("orc_form_" + form)
        engines.append(eng)
        mats.append(A.scipy().tocsr())
        nodes = [orc.axis(i)["nnp"] for i in range(3)]
    free = ~M.fixed_mask(nodes, c["dof"], c["fixed"])
    assert free.size == mats[0].shape[0]
    if name != "elasticity":
        engines[0].fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    if name == "identity":
        return engines[0], None, mats[0], None, free
    return engines[0], engines[1], mats[0], mats[1], free


def nev_of(name):
    return CASES["cube" if name == "identity" else name]["nev"]


def start_block(n, m=BLOCK):
    return np.random.default_rng(0).standard_normal((m, n)).T.copy()


def host_of(out):
    return np.column_stack([v.get() for v in out["X"]])


@functools.lru_cache(maxsize=None)
def device(name, pc):
    """(the solve's dict with the vectors on the host as "Xh", the kernel name, the launches IGXGetLastTiming reports)"""
    stiff, mass, _, _, _ = problem(name)
    out = stiff.eigen(nev_of(name), mass=mass, block=BLOCK, pc=pc, rtol=1e-8, maxit=300, history=True)
    name_, (_, _, launches) = stiff.kernel_name(), stiff.last_timing()
    out["Xh"] = host_of(out)
    out["Xh"].setflags(write=False)
    return out, name_, launches


def engine_T(stiff, pc, A):
    """the preconditioner of the host loop: numpy for the diagonal, the engine's own kernels for the point blocks and the fast diagonalisation"""
    if pc == "none":
        return None
    if pc == "jacobi":
        d = A.diagonal()
        return lambda r: r / d
    r_, z_ = stiff.create_vec(), stiff.create_vec()
    if pc == "fastdiag":
        def T(r):
            stiff.fast_diag_apply(r_.set(r), z_)
            return z_.get()
        return T
    cols = [stiff.create_vec() for _ in range(stiff.dof)]
    stiff.compute_matrix_block_diagonal(cols)
    stiff.block_diagonal_invert(cols)

    def T(r):
        stiff.block_diagonal_apply(cols, r_.set(r), z_)
        return z_.get()
    return T


@pytest.mark.parametrize("name,pc", SOLVES)
def test_lowest_pairs_against_eigh_of_the_oracle(name, pc):
    stiff, mass, A, B, free = problem(name)
    nev, m = nev_of(name), BLOCK
    out, kname, _ = device(name, pc)
    X, lam, its = out["Xh"], out["lambda"], out["iterations"]
    lam_ref, V = E.dense_reference(A, B, free, m + 1)
    bound, rnorm = E.parlett_bounds(A, B, free, X, lam)
    err = np.abs(lam - lam_ref[:m])
    defect = E.orthonormality_defect(B, X)
    ax = np.array([np.linalg.norm(A @ X[:, j]) for j in range(m)])
    resid_dev = float((np.abs(out["resid"] - rnorm) / ax).max())
    resid_tol = 8 * (its + 1) * (3 * m + 2) * U
    ref = E.lobpcg(A, B, start_block(A.shape[0]), nev, T=engine_T(stiff, pc, A), rtol=1e-8, maxit=300, fixed=~free)
    print("%s, pc=%s: %d iterations (host loop %d), reason %s, restarts %d, %d actions; lambda %s; |theta - lambda| %s; Parlett bounds %s; |X^T B X - I| %.3e; "
          "resid against the recomputed one / |A x| %.3e (tolerance %.3e); %s"
          % (name, pc, its, ref["iterations"], out["reason_name"], out["restarts"], out["actions"], np.array2string(lam[:nev], precision=8),
             np.array2string(err[:nev], precision=2), np.array2string(bound[:nev], precision=2), defect, resid_dev, resid_tol, kname))
    assert out["reason"] == E.CONVERGED == ref["reason"] and out["nconverged"] == nev
    assert lam_ref[nev] - lam_ref[nev - 1] > 1e-3 * lam_ref[nev], "nev does not cut in a spectral gap"
    assert np.all(err[:nev] <= bound[:nev] + 64 * U * np.abs(lam_ref[:nev]))
    assert np.all(np.diff(lam) >= 0) and defect <= ORTHO_TOL
    assert resid_dev <= resid_tol
    assert not X[~free].any(), "a fixed row is not exactly zero"
    assert out["history"].shape == (its + 1, m) and np.array_equal(out["history"][-1], out["resid"])
    assert np.all(out["resid"][:nev] <= 1e-8 * ax[:nev] * (1 + 1e-6))
    assert out["actions"] == (2 if mass is not None else 1) * m * (its + 1)
    assert abs(its - ref["iterations"]) <= ITERATION_MARGIN
    assert kname.startswith("eigen(lobpcg, block %d, pc=%s, vec_sumfact" % (m, pc)) and kname.endswith(", %d iterations)" % its), kname


def test_the_triple_eigenvalue_as_a_subspace():
    _, _, A, B, free = problem("cube")
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


def test_fast_diagonalisation_beats_no_preconditioner_on_the_cube():
    a, b = device("cube", "fastdiag")[0]["iterations"], device("cube", "none")[0]["iterations"]
    print("cube: %d iterations with fast diagonalisation, %d without a preconditioner" % (a, b))
    assert a < b


def test_a_solve_is_bit_repeatable():
    stiff, mass, _, _, _ = problem("cube")
    first, _, _ = device("cube", "jacobi")
    again = stiff.eigen(4, mass=mass, block=BLOCK, pc="jacobi", rtol=1e-8, maxit=300, history=True)
    assert np.array_equal(first["lambda"], again["lambda"]) and np.array_equal(first["history"], again["history"])
    assert np.array_equal(first["Xh"], host_of(again)) and first["iterations"] == again["iterations"]


def test_no_convergence_returns_the_reason():
    stiff, mass, A, B, free = problem("cube")
    out = stiff.eigen(4, mass=mass, block=BLOCK, maxit=0, history=True)
    print("maxit = 0: reason %s, %d iterations, %d actions, lambda %s" % (out["reason_name"], out["iterations"], out["actions"], np.array2string(out["lambda"][:4], precision=4)))
    assert out["reason"] == E.DIVERGED_ITS and out["iterations"] == 0 and out["history"].shape == (1, BLOCK) and out["actions"] == 2 * BLOCK
    X = host_of(out)
    assert E.orthonormality_defect(B, X) <= ORTHO_TOL and not X[~free].any()      # the Rayleigh-Ritz step on the start block has run
    out = stiff.eigen(4, mass=mass, block=BLOCK, pc="jacobi", rtol=0.0, atol=0.0, maxit=5, history=True)
    print("rtol = 0: reason %s, %d iterations, nconverged %d" % (out["reason_name"], out["iterations"], out["nconverged"]))
    assert out["reason"] == E.DIVERGED_ITS and out["iterations"] == 5 and out["nconverged"] == 0 and out["history"].shape == (6, BLOCK)


def test_two_equal_start_columns():
    stiff, mass, A, B, free = problem("cube")
    h = start_block(A.shape[0])
    h[:, 3] = h[:, 1]
    X = [stiff.create_vec().set(h[:, j]) for j in range(BLOCK)]
    out = stiff.eigen(4, mass=mass, block=BLOCK, X=X, maxit=50)
    ref = E.lobpcg(A, B, h, 4, maxit=50, fixed=~free)
    print("two equal start columns: reason %s after %d iterations, %d restarts (host loop: reason %d)" % (out["reason_name"], out["iterations"], out["restarts"], ref["reason"]))
    assert out["reason"] == E.DIVERGED_BREAKDOWN or out["restarts"] >= 1
    assert np.all(np.isfinite(host_of(out)))


@pytest.mark.parametrize("name,pc", [("cube", "none"), ("cube", "jacobi"), ("cube", "fastdiag"), ("elasticity", "pbjacobi"), ("identity", "none")])
def test_launches_equal_the_count_derived_from_the_loop(name, pc):
    """m columns, its iterations; a, b: launches of one action of stiff / of mass (0 without a mass); z: 1 where the space has a Dirichlet face
    (mg_zero_fixed per start column); D: the launches that form T (the diagonal; the point blocks and their inversion); t: launches of one
    application of T.
      set-up and step 0   m z + D + m (a + b) + 2 x 2 (two IGXVecMDot) + (3 with a mass, else 2) IGXVecMAXPY
      every pass          2 (bv_resid, bv_record): its + 1 passes
      every iteration     m t + m (a + b) + 2 x 2 + (6 with a mass, else 4) IGXVecMAXPY"""
    stiff, mass, _, _, _ = problem(name)
    out, _, launches = device(name, pc)
    m, its = BLOCK, out["iterations"]
    x, y = stiff.create_vec(), stiff.create_vec()
    stiff.compute_matrix_action(x, y)
    a = stiff.last_timing()[2]
    b = 0
    if mass is not None:
        mass.compute_matrix_action(mass.create_vec(), mass.create_vec())
        b = mass.last_timing()[2]
    D = t = 0
    if pc == "jacobi":
        stiff.compute_matrix_diagonal(y)
        D, t = stiff.last_timing()[2], 1
    elif pc == "pbjacobi":
        cols = [stiff.create_vec() for _ in range(stiff.dof)]
        stiff.compute_matrix_block_diagonal(cols)
        D = stiff.last_timing()[2] + 1
        t = 1
    elif pc == "fastdiag":
        stiff.fast_diag_apply(x, y)
        t = stiff.last_timing()[2]
    nm = 3 if mass is not None else 2
    count = m * 1 + D + m * (a + b) + 4 + nm + 2 * (its + 1) + its * (m * t + m * (a + b) + 4 + 2 * nm)
    print("%s, pc=%s: %d launches reported, %d derived (m = %d, its = %d, a = %d, b = %d, D = %d, t = %d)" % (name, pc, launches, count, m, its, a, b, D, t))
    assert launches == count


def test_refusals_that_need_vectors():
    import petiga_amd as P
    stiff, mass, _, _, _ = problem("cube")
    plain, _, _, _, _ = problem("elasticity")      # never set up for fast diagonalisation
    X = [stiff.create_vec() for _ in range(BLOCK)]
    with pytest.raises(P.IGXError) as e:
        stiff.eigen(4, mass=mass, block=BLOCK, X=X[:5] + [mass.create_vec()], pc="fastdiag")
    assert e.value.code == ARG_WRONG and "another IGX" in str(e.value) and "eigen solve" in str(e.value)
    with pytest.raises(P.IGXError) as e:
        stiff.eigen(4, mass=mass, block=BLOCK, X=X[:5] + [X[2]])
    assert e.value.code == ARG_WRONG and "twice" in str(e.value)
    with pytest.raises(P.IGXError) as e:
        plain.eigen(3, block=BLOCK, pc="fastdiag")
    assert e.value.code == ORDER and "IGXFastDiagSetUp" in str(e.value)
