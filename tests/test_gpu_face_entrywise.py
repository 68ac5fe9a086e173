"""Every launcher that makes a BOUNDARY-FORM pass, against the long double reference of face_ref.py, ENTRY BY ENTRY and ROW
BY ROW: |E - R| <= c u S, c = face_ref.C_FACE (calibrated on the CPU oracle alone by test_face_reference.py, which runs every case of
this file through the oracle).

test_boundary_forms.py and test_rtc_boundary_scalar.py hold the face passes with compare_mats at 1e-12 to 2e-11 of the largest free
entry, which cannot see a small entry, a far-band tile or one face's sign among six.  Here the geometry is common.warped_geometry's,
polynomial ("poly") or with random weights in [0.8, 1.2] ("nurbs"), amp 0.1 to 0.15, 3-D; every case pins its kernel and asserts its
name, compares every entry of to_coo_global() and every row of the vector, and prints `FACE name, kernel, worst ratio`.  The sizes are
the smallest that reach each path: all six faces and each face alone (the opposite face Dirichlet, a Dirichlet face cutting the visited
one), BoundaryIntegral (F rows only: detS and the lifting without the normal), one element along an axis (the same element touches both
faces), a periodic other axis with an odd element count (the colouring wraps), forms without a boundary branch, the point-form kernel,
run-time forms on both kernels (UserNitsche<3>, and a face-only struct whose S holds face terms alone), the Matrix / Vector drivers,
Bratu's Function / Jacobian with a visited face (vec_sumfact and state_pencil decline, feature_assemble integrates the state-dependent
callback over the face), one rank of two with the cut separating and crossing a visited face, and the functionals.

Worst ratios on an MI355X and the module's run time are in DESIGN 3.8."""
import numpy as np
import pytest

import face_ref as FR
import pointwise_ref as PW
import tensor_ref as T
from common import warped_geometry
from test_gpu_entrywise import _env
from test_rtc_boundary_scalar import NITSCHE

pytestmark = pytest.mark.gpu

LD = T.LD
C_FACE = FR.C_FACE
LAM = 3.5
ALL = [(a, s) for a in range(3) for s in range(2)]
FEATURE, GENERIC = ("feature_assemble",), ("generic_assemble",)

FACE_ONLY = r"""
// UserNitsche's face terms alone: nothing inside
template <int DIM> struct UserFaceOnly {
  static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = NEED_X | NEED_G;
  static constexpr bool HAS_BOUNDARY = true;
  static __device__ void mat(const PtView &, const double *, const double *, double *T) { T[0] = 0.0; }
  static __device__ void vec(const PtView &, const double *, double *R) { R[0] = 0.0; }
  static __device__ double alpha(const PtView &p) {
    double s = 0;
    for (int i = 0; i < DIM; ++i) { double Ni = 0; for (int j = 0; j < DIM; ++j) Ni += p.G[i * DIM + j] * p.normal[j]; s += Ni * Ni; }
    return 5 * (p.prm[0] + 1) / (2 / sqrt(s));
  }
  static __device__ void bmat(const PtView &p, const double *Na, const double *Nb, double *T) {
    double dna = 0, dnb = 0;
    for (int i = 0; i < DIM; ++i) { dna += Na[1 + i] * p.normal[i]; dnb += Nb[1 + i] * p.normal[i]; }
    T[0] = -Na[0] * dnb - Nb[0] * dna + alpha(p) * Na[0] * Nb[0];
  }
  static __device__ void bvec(const PtView &p, const double *Na, double *R) {
    double g = 0, dna = 0;
    for (int i = 0; i < DIM; ++i) { g += p.x[i] * p.x[i]; dna += Na[1 + i] * p.normal[i]; }
    R[0] = -dna * g + alpha(p) * Na[0] * g;
  }
};
"""

FLUX = r"""
// S[0] = int x . n dS over the visited faces, S[1] the volume (the normal is null inside)
template <int DIM> struct UserFlux {
  static constexpr int DOF = 1, ORDER = 1, NSCALAR = 2; static constexpr unsigned NEED = NEED_X;
  static __device__ void scalar(const PtView &p, double *S) {
    S[0] = 0.0; S[1] = 0.0;
    if (p.atboundary) { for (int i = 0; i < DIM; ++i) S[0] += p.x[i] * p.normal[i]; }
    else S[1] = 1.0;
  }
};
"""


def _case(geo, seed, faces, form="nitsche", k=None, driver="system", kernel=3, names=FEATURE, amp=0.15, bcs=None, **kw):
    """geo: "poly" / "nurbs" / None (no set_geometry); faces: the visited (axis, side); form: "nitsche", "boundary_integral", "mass",
    "poisson", "user_nitsche" or "face_only"; k: Nitsche's degree parameter (default: the largest degree); kw: setup_case keywords."""
    kw.setdefault("dof", 1)
    p = kw["p"]
    k = (max(p) if isinstance(p, (list, tuple)) else p) if k is None else k
    return dict(kw=kw, geo=geo, seed=seed, amp=amp, faces=list(faces), form=form, k=k, driver=driver, kernel=kernel, names=names, bcs=bcs)


def _alone(a, s):
    """The Dirichlet pattern of test_boundary_integral_on_device: the opposite face carries a value, a Dirichlet face on the next axis
    cuts the visited one."""
    return {(a, 1 - s, 0): 1.0, ((a + 1) % 3, 0, 0): -0.5}


_g = T.graded_knots
CASES = {
    # all six faces, the feature kernel
    "six-p2-nurbs": _case("nurbs", 41, ALL, p=2, N=[4, 3, 3], amp=0.1),
    "six-p3-poly": _case("poly", 42, ALL, p=3, N=[3, 3, 2], amp=0.1),
    "six-p321-nurbs": _case("nurbs", 43, ALL, p=[3, 2, 1], N=[3, 4, 5], amp=0.1),
    "six-p2-graded100-nogeo": _case(None, 0, ALL, p=2, N=0, knots=[_g(2, 5, 100.0), _g(2, 4, 0.01), _g(2, 4, 100.0)]),
    # BoundaryIntegral: F rows only
    **{"bint-%d%d-%s" % (a, s, geo): _case(geo, 50 + a, [(a, s)], "boundary_integral", p=2, N=[5, 4, 6], amp=0.1, bcs=_alone(a, s))
       for a, s in ((0, 0), (1, 1), (2, 1)) for geo in ("poly", "nurbs")},
    # one element along an axis; a periodic other axis with an odd count
    "one-element-axis0": _case("nurbs", 61, [(0, 0), (0, 1)], p=2, N=[1, 3, 3]),
    "periodic1-odd": _case("nurbs", 62, [(0, 1), (2, 0)], p=2, N=[4, 5, 3], periodic=[False, True, False]),
    # forms without a boundary branch
    "mass-dof2-p3-nurbs": _case("nurbs", 63, [(1, 0), (2, 1)], "mass", dof=2, p=3, N=[4, 3, 3]),
    "poisson-p2-nurbs": _case("nurbs", 64, [(0, 1)], "poisson", p=2, N=[4, 3, 3], bcs={(1, 0, 0): 0.5}),
    # the point-form kernel
    "generic-p4-nurbs": _case("nurbs", 65, ALL, p=4, N=[2, 2, 2], kernel=1, names=GENERIC),
    "generic-p2-nurbs": _case("nurbs", 66, ALL, p=2, N=[4, 3, 3], kernel=1, names=GENERIC),
    # run-time forms on both kernels
    **{"%s-kernel%d" % (f.replace("_", "-"), kn): _case("nurbs", 67, ALL, f, p=2, N=[4, 3, 3], kernel=kn,
                                                        names=("hiprtc",) + (GENERIC if kn else FEATURE))
       for f in ("user_nitsche", "face_only") for kn in (0, 1)},
    # Matrix and Vector: no fix-up, the same passes
    "matrix-vector-p2-poly": _case("poly", 68, ALL, p=2, N=[3, 4, 3], driver="matrix"),
}
# each face alone (one wrong tangent pair or sign must not average away over other faces)
ALONE = {(a, s): _case("nurbs", 70 + 2 * a + s, [(a, s)], p=2, N=[5, 4, 6], amp=0.1, bcs=_alone(a, s)) for a, s in ALL}
BRATU = _case("nurbs", 80, [(1, 0)], "bratu", p=2, N=[5, 4, 3], kernel=0, bcs={(0, 0, 0): 0.2, (2, 1, 0): -0.1})
# one rank of two (box=(2, rank): the partition cuts axis 2): both faces of the cut axis (each rank holds one and skips the other), and
# a face on another axis (each rank integrates its half)
RANKS = {"cut-axis": _case("nurbs", 81, [(2, 0), (2, 1)], p=2, N=[4, 4, 8]), "other-axis": _case("nurbs", 81, [(0, 1)], p=2, N=[4, 4, 8])}
SCALAR = _case("nurbs", 82, ALL, "volume", p=2, N=[4, 3, 5])
# the divergence theorem needs its integrands integrated to rounding: exact on the polynomial warp (degree 5 per axis at p + 1 points)
SCALAR_POLY = _case("poly", 82, ALL, "volume", p=2, N=[4, 3, 5])


# ---- set-up and references, shared with test_face_reference.py (which runs them on the CPU oracle)
def setup(case, engine, box=None, faces=None):
    """(oracle, engine or None, X, W, bcs) of a case: geometry, Dirichlet values (none for Matrix / Vector) and visited faces set."""
    orc, eng, _ = T.setup_case(dim=3, engine=engine, box=box, **case["kw"])
    X = W = None
    if case["geo"]:
        X, W = warped_geometry(orc, 3, seed=case["seed"], rational=(case["geo"] == "nurbs"), amp=case["amp"])
    bcs = None if case["driver"] == "matrix" else case["bcs"]
    for g in (orc, eng):
        if g is None:
            continue
        if X is not None:
            g.set_geometry(X, W)
        for (d, s, f), v in (bcs or {}).items():
            g.set_boundary_value(d, s, f, v)
        for a, s in (case["faces"] if faces is None else faces):
            g.set_boundary_form(a, s, True)
    return orc, eng, X, W, bcs


def reference(orc, X, W, bcs, case, faces=None, wrong=None):
    return FR.FaceRef(orc, X, W, bcs=bcs, faces=case["faces"] if faces is None else faces, wrong=wrong)


def linear_reference(fr, case):
    """(K, F, FS) of a linear case."""
    form = case["form"]
    if form == "face_only":                                # UserNitsche's passes minus the interior one: S holds face terms alone
        K, F, FS = fr.linear("nitsche", (case["k"],), "matrix")
        Ki, Fi, FSi = fr.interior.linear(T.poisson_f(3), "matrix")
        K.R, K.S, F, FS = K.R - Ki.R, K.S - Ki.S, F - Fi, FS - FSi
        return fr._fix_system(K, F, FS, case["driver"])
    return fr.linear({"user_nitsche": "nitsche"}.get(form, form), (case["k"],), case["driver"])


def state(n, seed=13):
    return 0.3 * np.random.default_rng(seed).standard_normal(n)


# ---- the tests
def _engine_form(eng, case):
    form = case["form"]
    if form == "user_nitsche":
        eng.set_form_source(NITSCHE, "UserNitsche<3>", (float(case["k"]),))
    elif form == "face_only":
        eng.set_form_source(FACE_ONLY, "UserFaceOnly<3>", (float(case["k"]),))
    elif form == "nitsche":
        eng.set_form("nitsche", (float(case["k"]),))
    elif form == "bratu":
        eng.set_form("bratu", (LAM,))
    else:
        eng.set_form(form)
    eng.set_kernel(case["kernel"])


def _names(eng, names):
    kn = eng.kernel_name()
    for s in names:
        assert s in kn, kn
    assert ("generic_assemble" in kn) == any("generic_assemble" in s for s in names), kn
    return kn


def _report(name, kn, worst):
    print("FACE %-28s %-64s worst %s u S (c = %g)" % (name, kn[:64], "  ".join("%s %.2f" % kv for kv in worst.items()), C_FACE))


def _assemble(eng, driver):
    A, b = eng.create_mat(), eng.create_vec()
    b.set(np.full(b.n, np.nan))                            # the drivers zero b
    if driver == "system":
        eng.compute_system(A, b)
    else:
        eng.compute_matrix(A)
        eng.compute_vector(b)
    eng.synchronize()
    return A, b


def _check_linear(name, case, monkeypatch):
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(case, True)
    _engine_form(eng, case)
    A, b = _assemble(eng, case["driver"])
    kn = _names(eng, case["names"])
    fr = reference(orc, X, W, bcs, case)
    assert len(fr.faces) == len(case["faces"])
    K, F, FS = linear_reference(fr, case)
    r, cc, v = A.to_coo_global()
    worst = {"K": T.compare_entrywise((r, cc, v), *K.at(r, cc), C_FACE, fr.tref, name + " K"),
             "F": PW.compare_rows(b.get(), F, FS, C_FACE, fr.tref, name + " F")}
    _report(name, kn, worst)


@pytest.mark.parametrize("name", list(CASES))
def test_face_passes_entrywise(name, monkeypatch):
    _check_linear(name, CASES[name], monkeypatch)


@pytest.mark.parametrize("axis,side", ALL)
def test_each_face_alone_entrywise(axis, side, monkeypatch):
    _check_linear("alone-%d%d" % (axis, side), ALONE[axis, side], monkeypatch)


def test_state_dependent_callback_on_a_face(monkeypatch):
    """Bratu's Function and Jacobian at a random state with face (1, 0) visited: the sum-factorised vector kernel and the pencil walk
    decline, feature_assemble integrates the ordinary callback at the face's interpolated state."""
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(BRATU, True)
    _engine_form(eng, BRATU)
    n = orc.global_size()
    U = state(n)
    Uv, F, J = eng.create_vec().set(U), eng.create_vec().set(np.full(n, np.nan)), eng.create_mat()
    fr = reference(orc, X, W, bcs, BRATU)
    worst = {}
    eng.compute_function(Uv, F)
    eng.synchronize()
    kn = _names(eng, FEATURE)
    assert "vec_sumfact" not in kn, kn
    worst["F"] = PW.compare_rows(F.get(), *fr.bratu_function(LAM, U), C_FACE, fr.tref, "bratu F")
    eng.compute_jacobian(Uv, J)
    eng.synchronize()
    kn = _names(eng, FEATURE)
    assert "state_pencil" not in kn, kn
    r, cc, v = J.to_coo_global()
    worst["J"] = T.compare_entrywise((r, cc, v), *fr.bratu_jacobian(LAM, U).at(r, cc), C_FACE, fr.tref, "bratu J")
    _report("bratu-face10-p2-nurbs", kn, worst)


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("run", list(RANKS))
def test_rank_boxes_entrywise(run, rank, monkeypatch):
    """The local rows of one rank of two before the ghost-row exchange (one process), as test_gpu_entrywise.test_rank_boxes_entrywise:
    the reference is the rank's element box and the faces, or the part of them, that lie in it."""
    case = RANKS[run]
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(case, True, box=(2, rank))
    es, ew, r_o = eng.sizes()["elem_start"][:3], eng.sizes()["elem_width"][:3], orc.ranges()
    assert list(es) == list(r_o["elem_start"]) and list(ew) == list(r_o["elem_width"]), (es, ew, r_o)
    assert list(ew) == [4, 4, 4] and es[2] == 4 * rank
    _engine_form(eng, case)
    A, b = _assemble(eng, "system")
    kn = _names(eng, FEATURE)
    fr = reference(orc, X, W, bcs, case)
    assert sorted(fr.faces) == ([(2, rank)] if run == "cut-axis" else [(0, 1)])
    K, F, FS = linear_reference(fr, case)
    r, cc, v = A.to_coo_global()
    assert fr.tref.coupled(r, cc).all()
    worst = {"K": T.compare_entrywise((r, cc, v), *K.at(r, cc), C_FACE, None, "%s rank %d K" % (run, rank))}
    rows = b.indices()
    assert np.unique(rows).size == rows.size and rows.min() >= 0
    worst["F"] = T.compare_entrywise((rows, b.get()), F[rows], FS[rows], C_FACE, None, "%s rank %d F" % (run, rank))
    _report("rank%d-%s" % (rank, run), kn, worst)


def scalar_references(fr):
    """{name: (R, S)} of the volume, the visited faces' area and int x . n dS."""
    return {"volume": fr.volume(), "area": fr.area(), "flux": fr.flux_of_x()}


def _hold(tag, value, R, S, worst):
    ratio = float(abs(LD(value) - R) / (LD(T.U_RND) * S))
    assert ratio <= C_FACE, "%s = %r, reference %r: %.1f u S" % (tag, value, float(R), ratio)
    worst[tag] = max(worst.get(tag, 0.0), ratio)
    return float(LD(T.U_RND) * S * C_FACE)


@pytest.mark.parametrize("kernel", [0, 1])
def test_volume_and_area_of_the_visited_faces(kernel, monkeypatch):
    """compute_scalar("volume") with each face visited alone and with all six, S[0] and S[1] each to its own bound, on the feature
    launcher (kernel 0) and on the point-form launcher (kernel 1), each bitwise repeatable."""
    _env(monkeypatch, {})
    worst = {}
    for faces in [[f] for f in ALL] + [ALL]:
        orc, eng, X, W, _ = setup(SCALAR, True, faces=faces)
        eng.set_kernel(kernel)
        ref = scalar_references(reference(orc, X, W, None, SCALAR, faces=faces))
        S = eng.compute_scalar("volume")
        kn = _names(eng, GENERIC if kernel else FEATURE)
        assert np.array_equal(S, eng.compute_scalar("volume"))
        _hold("volume", S[0], *ref["volume"], worst)
        _hold("area", S[1], *ref["area"], worst)
    _report("volume-area-kernel%d" % kernel, kn, worst)


def test_user_functional_on_the_faces(monkeypatch):
    """A user functional by source (int x . n dS on the faces, the volume inside) with all six faces visited, each component to its
    own bound, bitwise repeatable.  A run-time functional has ONE launcher, the point-form one (generic_assemble<...> (hiprtc):
    IGXComputeScalarSource does not look at IGXSetKernel, so "both launchers" of a user functional do not exist and the name is asserted
    instead.  The divergence theorem S[0] = 3 S[1] is held to the sum of the two bounds where the rule integrates both sides to
    rounding: on the polynomial warp.  At the p + 1 points of the NURBS case the two sides differ by 1.2044e-05 on the device, in the
    oracle and in the reference alike (each component within 0.2 u S of the reference): the quadrature error of a rational integrand,
    not a rounding error.  It falls below the rounding bound at 9 points per axis (test_face_reference.py holds the identity there on
    the reference alone), where that launcher refuses the functional: "element work set of the run-time form exceeds 64 KiB of LDS"
    (code 56)."""
    _env(monkeypatch, {})
    worst = {}
    for case in (SCALAR, SCALAR_POLY):
        orc, eng, X, W, _ = setup(case, True)
        ref = scalar_references(reference(orc, X, W, None, case))
        Sf = eng.compute_scalar_source(FLUX, "UserFlux<3>", 2)
        kn = _names(eng, ("generic_assemble<UserFlux<3>> (hiprtc",))
        assert np.array_equal(Sf, eng.compute_scalar_source(FLUX, "UserFlux<3>", 2))
        bf = _hold("flux", Sf[0], *ref["flux"], worst)
        bv = _hold("volume", Sf[1], *ref["volume"], worst)
        if case is SCALAR_POLY:
            assert abs(Sf[0] - 3 * Sf[1]) <= bf + 3 * bv, (Sf, bf, bv)
    _report("user-functional", kn, worst)
