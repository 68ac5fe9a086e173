"""IGXProbe on the GPU (IGX.probe: probe_locate + probe_eval + probe_geom, petiga_amd/csrc/probe.hpp) against the long double restatement
of its contract (tests/probe_ref.py), entry by entry: |E - R| <= c u S with the constants the CPU tests fixed (C_ID on the identity, C_MAP
on a map, C3 for order 3 on a map), no tolerance of this file's own.

Spaces: degrees (2, 3, 1) on 5 x 4 x 3 elements with graded knots and a C0 knot of full multiplicity, p = 3 on 4^3, a periodic axis, a
2-D and a 1-D space, p = 5 on 2^3; dof 1 and 3; the identity, an affine map, the polynomial warp and the NURBS map.
Points: every knot of every axis crossed with mid-span values (the whole cross product), all corners, the quadrature points of the two
corner elements and of an interior one (where, without a periodic axis, the oracle's own tabulation is a second witness held to the same
bound; with one its element-local numbering is the ghosted one and the points are checked against the reference alone), seeded random points.
Then: the known answer of the reference's probe test through the engine; position independence bit for bit (orders, embeddings, a list
one longer than the capped grid); two ranks; a state the library solved; the edges (poisoned buffer, no points, stale probe)."""
import itertools

import numpy as np
import pytest

import probe_ref as PR
import tensor_ref as T
from common import make_pair, warped_geometry
from test_probe_reference import KNOWN_POINTS, check_known_answer, known_answer_coefficients

pytestmark = pytest.mark.gpu


def _c0_knots(p, n, seed):
    U = T.graded_knots(p, n, 1.7, seed=seed)
    mid = np.unique(U)[max(1, n // 2)]
    return np.sort(np.concatenate([U, [mid] * (p - 1)]))


# name -> (dim, dof, p, N, knots (None: uniform), periodic)
SPACES = {
    "mixed-3d": (3, 3, [2, 3, 1], [5, 4, 3], "c0", None),
    "p3-4x4x4": (3, 1, [3, 3, 3], [4, 4, 4], None, None),
    "periodic": (3, 1, [2, 2, 2], [4, 3, 3], None, [True, False, False]),
    "2d": (2, 3, [3, 2], [4, 5], "c0", None),
    "1d": (1, 1, [3], [6], "c0", None),
    "p5-2x2x2": (3, 1, [5, 5, 5], [2, 2, 2], None, None),
}
CASES = [("mixed-3d", k) for k in PR.GEOMETRIES] + [("p3-4x4x4", "identity"), ("p3-4x4x4", "nurbs"), ("periodic", "identity"), ("periodic", "nurbs"),
                                                    ("2d", "nurbs"), ("2d", "affine"), ("1d", "nurbs"), ("1d", "identity"), ("p5-2x2x2", "nurbs")]


def _space(name, kind, comm=None):
    dim, dof, p, N, knots, periodic = SPACES[name]
    kn = [_c0_knots(p[d], N[d], 40 + d) for d in range(dim)] if knots == "c0" else None
    orc, eng = make_pair(dim, dof, p, N, knots=kn, periodic=periodic, order=3)
    X, W = PR.geometry(orc, dim, kind)
    if X is not None:
        orc.set_geometry(X, W)
        eng.set_geometry(X, W)
    return orc, eng, PR.ProbeRef(PR.axes_of(orc), dof, X, W)


def _points(orc, seed=0, stride=1):
    """(points, slices of the quadrature points per element ID)"""
    dim = orc.dim
    per_axis = []
    for d in range(dim):
        ax = orc.axis(d)
        k = np.unique(ax["U"][ax["p"]:len(ax["U"]) - ax["p"]])
        per_axis.append(np.concatenate([k, 0.5 * (k[1:] + k[:-1])]))
    cross = np.array(list(itertools.product(*per_axis)))[::stride]
    lim = [(orc.axis(d)["U"][orc.axis(d)["p"]], orc.axis(d)["U"][-orc.axis(d)["p"] - 1]) for d in range(dim)]      # the axis is [U[p], U[n+1]]
    corners = np.array(list(itertools.product(*lim)))
    nel = [orc.axis(d)["nel"] for d in range(dim)]
    quad, parts, at = [], {}, len(cross) + len(corners)
    periodic = any(orc.axis(d)["periodic"] for d in range(dim))
    for ID in sorted({tuple(0 for _ in nel), tuple(n - 1 for n in nel), tuple(n // 2 for n in nel)}):
        pt = orc.element(list(ID))["point"]
        if not periodic:
            parts[ID] = slice(at, at + len(pt))
        at += len(pt)
        quad.append(pt)
    rng = np.random.default_rng(seed)
    lo, hi = np.array([l[0] for l in lim]), np.array([l[1] for l in lim])
    rnd = lo + (hi - lo) * rng.random((40, dim))
    return np.concatenate([cross, corners] + quad + [rnd]), parts


@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_every_entry_within_the_bound(name, kind):
    orc, eng, ref = _space(name, kind)
    mapped = kind != "identity"
    pts, parts = _points(orc)
    coef = np.random.default_rng(11).uniform(-1, 1, orc.global_size())
    U = eng.create_vec().set(coef)
    prb = eng.probe(pts, order=3)
    assert prb.local.all()
    eng.set_timing(True)
    for der in range(4):
        out = np.full((len(pts), orc.dof) + (orc.dim,) * der, np.nan)             # a poisoned buffer is fully overwritten
        E = prb.evaluate(U, der, out=out)
        R, S = ref.evaluate(coef, pts, der)
        c = PR.bound(der, mapped)
        worst = PR.compare(E, R, S, c, "%s %s der %d" % (name, kind, der))
        print("%s %s der %d: %d points, worst %.2f u S (c = %g); %s" % (name, kind, der, len(pts), worst, c, eng.kernel_name()))
        assert eng.kernel_name().startswith("probe(%dd, p=" % orc.dim) and "order=%d" % der in eng.kernel_name() and "%d points" % len(pts) in eng.kernel_name()
        total_ms, kernel_ms, launches = eng.last_timing()
        assert launches == 1 and kernel_ms > 0 and total_ms > 0
        for ID, sl in parts.items():                                                  # the oracle's tabulation at its own quadrature points
            p2, Eo = PR.oracle_at_element(orc, ID, coef, der)
            assert np.array_equal(p2, pts[sl])
            PR.compare(Eo, R[sl], S[sl], c, "%s %s der %d: the oracle at element %s" % (name, kind, der, ID))
    want = "rational" if kind == "nurbs" else ("identity" if kind == "identity" else "polynomial")
    assert want in eng.kernel_name()
    x = prb.geom_map()
    R, S = ref.geom_map(pts)
    PR.compare(x, R, S, PR.bound(0, mapped), "%s %s geom_map" % (name, kind))
    prb.close()


def test_known_answer_through_the_engine():
    orc, eng = make_pair(3, 1, 3, [4, 3, 5])
    coef = known_answer_coefficients(PR.axes_of(orc))
    U = eng.create_vec().set(coef)
    prb = eng.probe(KNOWN_POINTS, order=3)
    check_known_answer(lambda der: prb.evaluate(U, der))


def test_position_independence_bit_for_bit():
    import petiga_amd as P
    orc, eng, _ = _space("p3-4x4x4", "nurbs")
    coef = np.random.default_rng(3).uniform(-1, 1, orc.global_size())
    U = eng.create_vec().set(coef)
    base, _ = _points(orc, seed=4, stride=11)
    base = base[:96]
    rng = np.random.default_rng(8)

    def run(points, der):
        return eng.probe(points, order=3).evaluate(U, der)

    for der in (0, 1, 2, 3):
        first = run(base, der)
        assert np.array_equal(first, run(base, der))                                  # a second run
        assert np.array_equal(first[::-1], run(base[::-1], der))
        perm = rng.permutation(len(base))
        assert np.array_equal(first[perm], run(base[perm], der))
        turn = eng.probe(base[:1]).info()["points_per_turn"]
        assert turn == P.PROBE_GRID_POINTS
        for length in (1, 63, 64, 65, 1000, turn + 1):
            if length > 1000 and der >= 2:
                continue                                                              # (the grid turns over at der 0 and 1: the same loop)
            m = min(length, len(base))
            where = np.sort(rng.choice(length, size=m, replace=False))
            where[-1] = length - 1                                                    # the last point of the list: past the capped grid
            pts = rng.random((length, 3))
            pts[where] = base[:m]
            got = run(pts, der)
            assert np.array_equal(got[where], first[:m]), (der, length)
            assert np.all(np.isfinite(got))


def test_two_ranks_partition_the_points():
    """two IGX of one process, ranks 0 and 1 of a partition along axis 0; every rank's vector holds its rows and ghosts of one global
    vector (set through the natural indices of its entries)"""
    import petiga_amd as P
    dim, dof, p, N = 3, 2, [2, 3, 2], [4, 3, 3]
    orc, one = make_pair(dim, dof, p, N)
    X, W = warped_geometry(orc, dim, seed=3, rational=True)
    one.set_geometry(X, W)
    coef = np.random.default_rng(6).uniform(-1, 1, orc.global_size())
    pts, _ = _points(orc, seed=2)
    pts = np.concatenate([pts, [[0.5, 0.3, 0.7], [0.5, 0.0, 1.0], [0.25, 0.5, 0.5]]])      # on the shared face (u0 = 0.5) and on a knot beside it
    U1 = one.create_vec().set(coef)
    full = [one.probe(pts, order=3).evaluate(U1, der) for der in range(4)]
    xfull = one.probe(pts).geom_map()
    parts, flags, xs = [], [], []
    for rank in range(2):
        g = P.IGX(dim, dof)
        g.set_comm(2, rank)
        g.set_processors(0, 2)
        for i in range(dim):
            g.axis_uniform(i, p[i], N[i])
        g.setup()
        g.set_geometry(X, W)
        v = g.create_vec()
        v.set(coef[v.indices(0)])
        prb = g.probe(pts, order=3)
        flags.append(prb.local)
        parts.append([prb.evaluate(v, der) for der in range(4)])
        xs.append(prb.geom_map())
    assert np.all(flags[0] ^ flags[1]) and flags[0].any() and flags[1].any()          # the flags partition the points
    on_face = pts[:, 0] == 0.5
    assert on_face.any() and flags[1][on_face].all()                                  # the shared face belongs to the span on its right
    for der in range(4):
        for rank in range(2):
            assert np.all(parts[rank][der][~flags[rank]] == 0.0)                      # off-rank entries are exactly 0
        assert np.array_equal(parts[0][der] + parts[1][der], full[der])               # the sum over the ranks: the single-rank bits
    assert np.array_equal(xs[0] + xs[1], xfull)


FLUX = r"""
template <int DIM> struct ProbeFlux {
  static constexpr int DOF = 1, ORDER = 1, NSCALAR = 1; static constexpr unsigned NEED = NEED_U | NEED_GU;
  static __device__ void scalar(const PtView &p, double *S) { double f = 0; if (p.atboundary) for (int i = 0; i < DIM; ++i) f += p.gu[i] * p.normal[i]; S[0] = f; }
};
"""


def test_a_state_the_library_solved():
    """Poisson on the NURBS map by IGXSolve: the probe returns the Dirichlet values on their faces to the solve's tolerance, and its
    gradient, summed over the quadrature points of a face with the oracle's normals and measures, is the flux the functional reports"""
    dim, p, N = 3, 2, [4, 4, 4]
    orc, eng = make_pair(dim, 1, p, N)
    X, W = warped_geometry(orc, dim, seed=5, rational=True, amp=0.1)
    vals = {(0, 0): 1.0, (0, 1): 2.5}
    for g in (orc, eng):
        g.set_geometry(X, W)
        for (d, s), v in vals.items():
            g.set_boundary_value(d, s, 0, v)
    eng.set_form("poisson")
    b, x = eng.create_vec(), eng.create_vec()
    A = eng.create_mat()
    eng.compute_system(A, b)
    info = eng.solve(b, x, method="cg", op="matrix", pc="jacobi", rtol=1e-12, maxit=2000)
    assert info["reason"] > 0, info
    # A fixed row of the operator is count * x_i with the right-hand side count * v and no other entry in its row or column, so its error is
    # its own residual / count <= |r|_2 (the recurrence residual, plus the rounding of the true one: a few u |v|); on the face the basis is a
    # partition of unity of the fixed functions alone, sum |R_a| = 1, so the probed value is off by at most that plus its own c u S, S = |v|
    tol = info["rnorm"] + 2 * PR.C_MAP * PR.U_RND * max(abs(v) for v in vals.values())
    assert info["rnorm"] <= 1e-12 * info["bnorm"]
    rng = np.random.default_rng(9)
    for (d, s), v in vals.items():
        pts = rng.random((50, 3))
        pts[:, d] = float(s)
        got = eng.probe(pts).evaluate(x, 0)
        print("face (%d, %d): max |probe - %g| = %.3e, bound %.3e" % (d, s, v, np.abs(got - v).max(), tol))
        assert np.abs(got - v).max() <= tol, (d, s, np.abs(got - v).max(), tol)
    # the flux through the face (0, 1)
    for g in (orc, eng):
        g.clear_boundary()
        g.set_boundary_form(0, 1, True)
    flux = eng.compute_scalar_source(FLUX, "ProbeFlux<3>", 1, x)[0]
    total = 0.0
    for j in range(N[1]):
        for k in range(N[2]):
            el = orc.element([N[0] - 1, j, k], boundary_id=1)
            grad = eng.probe(el["point"], order=1).evaluate(x, 1)[:, 0, :]
            total += np.sum(el["weight"] * el["detJac"] * np.einsum("qi,qi->q", grad, el["normal"]))
    print("flux through the face: functional %.15g, probe %.15g" % (flux, total))
    assert abs(total - flux) <= 1e-11 * max(abs(flux), 1.0)


def test_edges():
    import petiga_amd as P
    orc, eng, _ = _space("2d", "nurbs")
    U = eng.create_vec().set(np.ones(orc.global_size()))
    empty = eng.probe(np.zeros((0, 2)), order=1)
    assert empty.evaluate(U, 1).shape == (0, 3, 2) and empty.geom_map().shape == (0, 2) and empty.local.shape == (0,)
    eng.set_timing(True)                                                              # every call that launches is timed under its own name
    prb = eng.probe([[0.5, 0.5], [1.0, 0.0]], order=1)
    total_ms, kernel_ms, launches = eng.last_timing()
    assert eng.kernel_name().startswith("probe_locate(") and launches == 1 and 0 < kernel_ms and 0 < total_ms
    assert prb.geom_map().shape == (2, 2) and prb.info() == dict(npts=2, order=1, nsd=2, points_per_turn=P.PROBE_GRID_POINTS)
    total_ms, kernel_ms, launches = eng.last_timing()
    assert eng.kernel_name().startswith("probe_geom(") and launches == 1 and 0 < kernel_ms and 0 < total_ms
    empty.evaluate(U, 0)
    assert eng.kernel_name().startswith("probe(") and eng.last_timing() == (0.0, 0.0, 0)      # no points: nothing launched, nothing timed
    eng.set_timing(False)
    v = prb.evaluate(U, 0)
    assert np.all(np.abs(v - 1.0) <= 8 * PR.U_RND)                                    # the partition of unity of the rational basis
    with pytest.raises(P.IGXError) as e:
        prb.evaluate(U, 2)
    assert e.value.code == 63
    other = make_pair(2, 3, [3, 2], [4, 5])[1]
    with pytest.raises(P.IGXError) as e:
        prb.evaluate(other.create_vec(), 0)                                           # a vector of another IGX
    assert e.value.code == 62 and "probe" in str(e.value)
    eng.setup()                                                                       # ... and the probe is stale
    for call in (lambda: prb.evaluate(U, 0), prb.geom_map, lambda: prb.local):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == 58 and "stale" in str(e.value)
