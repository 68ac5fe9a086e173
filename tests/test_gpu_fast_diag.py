"""IGXFastDiagSetUp / IGXFastDiagApply on the GPU (fast_diag.hpp).  The reference of every exact-inverse case is a sparse direct solve
(scipy's spsolve) of the matrix of the same operator: the CPU oracle's, or the engine's own assembled matrix for a run-time struct.  The
yardstick is the numpy restatement of the method (tests/fast_diag_ref.py: scipy's BSpline, eigh, einsum): with
e_ref = max|Z_numpy - X| / max|X| over the free dofs the engine must satisfy max|Z - X| <= max(8 e_ref, 1e-13) max|X| there, and
Z[fixed] == R[fixed] / count bit for bit.  The ratios are printed."""
import numpy as np
import pytest

from common import make_pair, warped_geometry
from fast_diag_ref import FastDiagRef, axis_matrices, fixed_faces, pcg

pytestmark = pytest.mark.gpu

ALL6 = [(d, s) for d in range(3) for s in range(2)]

# T = a Na Nb + sum_d b_d d_d Na d_d Nb on every field, params (a, b0, b1, b2)
USER_ANISO = r"""
struct UserAniso {
  static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = 0;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    T[0] = p.prm[0] * Na[0] * Nb[0] + p.prm[1] * Na[1] * Nb[1] + p.prm[2] * Na[2] * Nb[2] + p.prm[3] * Na[3] * Nb[3];
  }
  static __device__ void vec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; }
};
struct UserAniso2 {
  static constexpr int DOF = 2, ORDER = 1; static constexpr unsigned NEED = 0;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    const double t = p.prm[0] * Na[0] * Nb[0] + p.prm[1] * Na[1] * Nb[1] + p.prm[2] * Na[2] * Nb[2] + p.prm[3] * Na[3] * Nb[3];
    T[0] = t; T[1] = 0.0; T[2] = 0.0; T[3] = t;
  }
  static __device__ void vec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; R[1] = Na[0]; }
};
"""


def _reference(orc, dof, faces, alpha, beta, nqp=None, periodic=None):
    axes = []
    for d in range(3):
        ax = orc.axis(d)
        axes.append(axis_matrices(ax["U"], ax["p"], None if nqp is None else nqp[d], bool(periodic and periodic[d])))
    return FastDiagRef(axes, dof, fixed_faces(dof, faces), alpha, beta)


def _engine_matrix(eng):
    """The engine's own assembled matrix of the operator IGXComputeMatrixAction applies: IGXComputeSystem's, which carries the matrix
    half of IGAElementFixSystem (IGXComputeMatrix assembles the form's matrix without the Dirichlet rows and columns)."""
    import scipy.sparse as sp
    A, b = eng.create_mat(), eng.create_vec()
    eng.compute_system(A, b)
    eng.synchronize()
    r, c, v = A.to_coo_global()
    n = int(r.max()) + 1
    return sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsc()


def _apply(eng, R, inplace=False):
    Rv = eng.create_vec().set(R)
    Zv = Rv if inplace else eng.create_vec()
    eng.fast_diag_apply(Rv, Zv)
    eng.synchronize()
    return Zv.get().copy()


def _check_exact(label, eng, A, ref, seed=0):
    """Z = P R against spsolve(A, R) on the free dofs and against R / count on the fixed ones; returns Z and R"""
    import scipy.sparse.linalg as spla
    rng = np.random.default_rng(seed)
    R = rng.standard_normal(A.shape[0])
    X = spla.spsolve(A.tocsc(), R)
    free = ref.free_mask()
    Zn = ref.apply(R)
    scale = np.abs(X[free]).max()
    e_ref = np.abs(Zn - X)[free].max() / scale
    Z = _apply(eng, R)
    e = np.abs(Z - X)[free].max() / scale
    print("%s: %d dofs (%d free): engine %.3e, numpy restatement %.3e, ratio %.2f; kernel %s"
          % (label, R.size, int(free.sum()), e, e_ref, e / max(e_ref, 1e-300), eng.kernel_name()))
    assert e <= max(8 * e_ref, 1e-13)
    want = R.reshape(ref.n[::-1] + [ref.dof]) / ref.count()[..., None]
    assert np.array_equal(Z[~free], want.reshape(-1)[~free]), "a fixed row is not R / count bit for bit"
    return Z, R


POISSON = {
    # name: (p, N, faces, knots, nqp)
    "p3 (5,4,3), mixed ends, every m < 16": (3, [5, 4, 3], [(0, 0), (1, 1), (2, 0)], None, None),
    "p2 (17,6,5), six faces, m = 17": (2, [17, 6, 5], ALL6, None, None),
    "p2 (70,3,3), faces on axis 0, m = 70": (2, [70, 3, 3], [(0, 0), (0, 1)], None, None),
    "p3 non-uniform with a C0 knot": (3, [5, 4, 3], [(0, 0), (0, 1), (2, 1)], [[0, 0, 0, 0, 0.25, 0.5, 0.5, 0.5, 0.7, 1, 1, 1, 1], None, None], None),
    "p2 (5,4,3), nqp = 4 on axis 1": (2, [5, 4, 3], [(0, 0), (1, 1), (2, 1)], None, [None, 4, None]),
    # the axis lengths of real runs (260 functions: two row blocks; the benchmark's 256^3 at p = 3 has 259), quasi-1-D and quasi-2-D so
    # that spsolve stays fast: here the host eigen-solver's accuracy at m = 258 decides
    "p2 (258,2,2), six faces, m = 258 on axis 0": (2, [258, 2, 2], ALL6, None, None),
    "p2 (2,258,2), six faces, m = 258 on axis 1": (2, [2, 258, 2], ALL6, None, None),
    "p2 (2,2,258), six faces, m = 258 on axis 2": (2, [2, 2, 258], ALL6, None, None),
    "p3 (97,45,2), six faces, m = 98 and 46": (3, [97, 45, 2], ALL6, None, None),
}


@pytest.mark.parametrize("name", sorted(POISSON))
def test_exact_inverse_of_poisson(name):
    p, N, faces, knots, nqp = POISSON[name]
    orc, eng = make_pair(3, 1, p, N, knots=knots, nqp=nqp)
    for g in (orc, eng):
        for d, s in faces:
            g.set_boundary_value(d, s, 0, 0.25)
    A_o, _ = orc.compute_system("orc_form_poisson")
    ref = _reference(orc, 1, [(d, s, 0) for d, s in faces], 0.0, [1.0, 1.0, 1.0], nqp=nqp)
    assert eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0]) == 0
    _check_exact(name, eng, A_o.scipy(), ref)


def test_exact_inverse_of_a_three_field_mass():
    orc, eng = make_pair(3, 3, 2, [5, 4, 3])
    A_o, _ = orc.compute_system("orc_form_mass")
    ref = _reference(orc, 3, [], 1.0, [0.0, 0.0, 0.0])
    assert eng.fast_diag_setup(1.0, [0.0, 0.0, 0.0]) == 0
    _check_exact("mass, dof = 3", eng, A_o.scipy(), ref)
    assert "fields share their tables" in eng.kernel_name()


PARAMS = (2.5, 1.0, 0.3, 4.0)


def test_alpha_and_anisotropic_beta():
    orc, eng = make_pair(3, 1, 2, [6, 5, 4])
    faces = [(0, 1, 0), (2, 0, 0)]
    for d, s, f in faces:
        eng.set_boundary_value(d, s, f, 0.0)
    eng.set_form_source(USER_ANISO, "UserAniso", PARAMS)
    ref = _reference(orc, 1, faces, PARAMS[0], PARAMS[1:])
    assert eng.fast_diag_setup(PARAMS[0], PARAMS[1:]) == 0
    _check_exact("a = 2.5, b = (1, 0.3, 4)", eng, _engine_matrix(eng), ref)


def test_two_fields_with_different_faces():
    orc, eng = make_pair(3, 2, 2, [6, 5, 4])
    faces = [(0, 0, 0), (1, 1, 1), (2, 0, 1)]
    for d, s, f in faces:
        eng.set_boundary_value(d, s, f, 0.0)
    eng.set_form_source(USER_ANISO, "UserAniso2", PARAMS)
    A = _engine_matrix(eng)
    ref = _reference(orc, 2, faces, PARAMS[0], PARAMS[1:])
    assert eng.fast_diag_setup(PARAMS[0], PARAMS[1:]) == 0
    Z, R = _check_exact("two fields, different faces", eng, A, ref)
    assert "tables per field" in eng.kernel_name()
    # each field against its own block
    import scipy.sparse.linalg as spla
    free = ref.free_mask()
    for f in range(2):
        idx = np.arange(f, R.size, 2)
        Xf = spla.spsolve(A[idx][:, idx].tocsc(), R[idx])
        ff = free[idx]
        e_ref = np.abs(ref.apply(R)[idx] - Xf)[ff].max() / np.abs(Xf[ff]).max()
        e = np.abs(Z[idx] - Xf)[ff].max() / np.abs(Xf[ff]).max()
        print("field %d against its own block: engine %.3e, numpy restatement %.3e" % (f, e, e_ref))
        assert e <= max(8 * e_ref, 1e-13)


def test_periodic_on_all_three_axes():
    orc, eng = make_pair(3, 1, 2, [6, 6, 8], periodic=True)
    eng.set_form_source(USER_ANISO, "UserAniso", (1.0, 1.0, 1.0, 1.0))
    ref = _reference(orc, 1, [], 1.0, [1.0, 1.0, 1.0], periodic=[True] * 3)
    assert ref.n == [6, 6, 8]
    assert eng.fast_diag_setup(1.0, [1.0, 1.0, 1.0]) == 0
    _check_exact("periodic (6,6,8)", eng, _engine_matrix(eng), ref)


def test_pseudo_inverse_of_pure_neumann_poisson():
    """nzeroed == 1: the constant.  The reference is the numpy restatement with the same mode zeroed.  Both evaluate the same six
    contractions and one scaling in double precision; the rounding error of either is bounded by c u kappa max|Z| with
    kappa = max denominator / smallest kept denominator (the amplification of the scaling) and c the summed lengths of the six
    contractions, 2 (n0 + n1 + n2): the difference of the two is held to twice that."""
    orc, eng = make_pair(3, 1, 2, [5, 4, 3])
    ref = _reference(orc, 1, [], 0.0, [1.0, 1.0, 1.0])
    assert ref.nzeroed == 1
    assert eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0]) == 1
    R = np.random.default_rng(3).standard_normal(7 * 6 * 5)
    Zn, Z = ref.apply(R), _apply(eng, R)
    den = np.abs(ref.denominators(0))
    kappa = den.max() / den[den > 1e-12 * den.max()].min()
    bound = 2 * 2 * sum(ref.n) * 2.0 ** -53 * kappa
    e = np.abs(Z - Zn).max() / np.abs(Zn).max()
    print("pure Neumann: |Z - Z_numpy| / max|Z| = %.3e, bound %.3e (kappa %.1f)" % (e, bound, kappa))
    assert e <= bound


def test_in_place_and_repeatable():
    orc, eng = make_pair(3, 2, 3, [5, 4, 3])
    for f, (d, s) in ((0, (0, 0)), (1, (1, 1)), (1, (2, 0))):
        eng.set_boundary_value(d, s, f, 0.0)
    eng.fast_diag_setup(0.5, [1.0, 2.0, 1.0])
    R = np.random.default_rng(5).standard_normal(8 * 7 * 6 * 2)
    Z1, Z2, Z3 = _apply(eng, R), _apply(eng, R), _apply(eng, R, inplace=True)
    assert np.array_equal(Z1, Z2), "two runs differ"
    assert np.array_equal(Z1, Z3), "Apply(R, R) differs from Apply(R, Z)"
    assert np.all(np.isfinite(Z1)) and np.abs(Z1).max() > 0


def test_kernel_name_timing_and_a_second_setup():
    orc, eng = make_pair(3, 1, 2, [6, 5, 4])
    eng.set_boundary_value(0, 0, 0, 0.0)
    eng.set_timing(True)
    eng.fast_diag_setup(1.0, [1.0, 1.0, 1.0])
    R = np.random.default_rng(7).standard_normal(8 * 7 * 6)
    Z1 = _apply(eng, R)
    assert eng.kernel_name().startswith("fast_diag(mfma_f64_16x16x4")
    total, kernel, launches = eng.last_timing()
    assert launches == 6 and total > 0 and kernel > 0
    eng.fast_diag_setup(3.0, [0.5, 1.0, 2.0])
    Z2 = _apply(eng, R)
    ref = _reference(orc, 1, [(0, 0, 0)], 3.0, [0.5, 1.0, 2.0])
    Zn = ref.apply(R)
    assert np.abs(Z2 - Zn).max() <= 1e-12 * np.abs(Zn).max() and np.abs(Z2 - Z1).max() > 1e-3 * np.abs(Z1).max()


def test_wrong_state_and_wrong_vectors():
    import petiga_amd as P
    _, eng = make_pair(3, 1, 2, [4, 4, 3])
    _, other = make_pair(3, 1, 2, [4, 4, 4])
    eng.set_boundary_value(0, 0, 0, 0.0)
    eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    R, Z = eng.create_vec(), eng.create_vec()
    eng.fast_diag_apply(R, Z)
    with pytest.raises(P.IGXError) as e:
        eng.fast_diag_apply(R, other.create_vec())
    assert e.value.code == 62
    assert P.lib().IGXFastDiagApply(eng.h, R.h, None) == 62
    eng.set_fixtable(R)
    with pytest.raises(P.IGXError) as e:
        eng.fast_diag_apply(R, Z)
    assert e.value.code == 56 and "fast diagonalisation" in str(e.value) and "fix table" in str(e.value)
    with pytest.raises(P.IGXError) as e:
        eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    assert e.value.code == 56 and "fix table" in str(e.value)
    eng.set_fixtable(None)
    eng.fast_diag_apply(R, Z)
    eng.clear_boundary()
    with pytest.raises(P.IGXError) as e:
        eng.fast_diag_apply(R, Z)
    assert e.value.code == 73 and "IGXFastDiagSetUp" in str(e.value)
    eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    eng.fast_diag_apply(R, Z)
    eng.synchronize()


@pytest.mark.parametrize("p,N", [(3, [5, 4, 3]), (2, [8, 8, 8])])
def test_fast_diag_preconditioned_cg_on_the_action(p, N):
    """The loop of test_jacobi_preconditioned_cg_on_the_action (tests/test_gpu_matrix_diagonal.py) on a rational warped geometry, six
    Dirichlet faces: the operator is the GPU's IGXComputeMatrixAction, the preconditioner IGXFastDiagApply with alpha = 0, beta = 1, the
    stop criterion |r| <= 1e-10 |b|.  The engine may take two iterations more than the same loop on the oracle's matrix with the numpy
    restatement, the solution agrees with spsolve of the oracle's system to 1e-8 max|x|, and the count is below the count of the same
    loop with 1 / D of the engine's own IGXComputeMatrixDiagonal.  The Dirichlet values are zero and the right-hand side is the form's
    unit source: |b| is then carried by the free rows, so the plain residual norm measures them.  (With the values of the Jacobi test,
    0.5 + 0.25 d + 0.125 s, the fixed rows -- element count times value -- carry |b| and the loop stops while the free rows are still
    1e-8 off: on the oracle's matrix 24 and 14 iterations against 88 and 37 for Jacobi, errors 4.8e-8 and 1.4e-8.)  Seen on the CPU with
    the values here: 28 and 16 iterations against 100 and 47, errors 5.7e-10 and 1.9e-10; on an MI355X the same counts and errors."""
    import scipy.sparse.linalg as spla
    orc, eng = make_pair(3, 1, p, N)
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
    A_o, b_o = orc.compute_system("orc_form_poisson")
    A_s, b_o = A_o.scipy().tocsr(), np.asarray(b_o)
    want = spla.spsolve(A_s.tocsc(), b_o)
    ref = _reference(orc, 1, [(d, s, 0) for d, s in ALL6], 0.0, [1.0, 1.0, 1.0])
    _, k_ref = pcg(lambda v: A_s @ v, ref.apply, b_o)
    Xv, Yv, Dv = eng.create_vec(), eng.create_vec(), eng.create_vec()

    def op(v):
        Xv.set(v)
        eng.compute_matrix_action(Xv, Yv)
        eng.synchronize()
        return Yv.get().copy()

    def fd(v):
        Xv.set(v)
        eng.fast_diag_apply(Xv, Yv)
        eng.synchronize()
        return Yv.get().copy()

    eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    x, k = pcg(op, fd, rhs)
    eng.compute_matrix_diagonal(Dv)
    eng.synchronize()
    D = Dv.get().copy()
    _, k_jac = pcg(op, lambda v: v / D, rhs)
    err = np.abs(x - want).max() / np.abs(want).max()
    print("p = %d %s: %d iterations with fast diagonalisation (%d on the oracle's matrix with the numpy restatement), %d with Jacobi; max|x - spsolve| / max|x| = %.3e"
          % (p, N, k, k_ref, k_jac, err))
    assert k <= k_ref + 2
    assert err <= 1e-8
    assert k < k_jac
