"""IGXTransfer on the GPU beyond the entry-by-entry check (tests/test_gpu_transfer_entrywise.py): what the transfer MEANS and what it
promises bit for bit.

  exactness    the prolonged vector is the same function: fine.probe(P xc) against coarse.probe(xc) at 200 random points plus knots and both
               ends, der 0 and 1, on the identity geometry, on a polynomial map and on a NURBS map whose fine net is geometry.refine of the
               coarse one.  On a rational geometry the library's basis is rational, R_j = w_j N_j / W, so the same function has the fine
               coefficients (T (w_c * x_c)) / w_f: the test prolongs the weighted vector and divides (the header says so).
               Bound: both probes lie within c u S of their reference (probe_ref.bound: C_ID on the identity, C_MAP on a map); the fine
               one evaluates a vector that carries the prolongation's c_P u S_P per entry, S_P >= |P xc| the prolongation's own sum of
               absolute terms; so |E_f - E_c| <= u (c S_c + (c + c_P) S_f) with S_c = probe_ref's S of x_c and S_f its S of the vector S_P.
  Galerkin     Poisson without Dirichlet values on the identity geometry with p + 1 Gauss points: the rule is exact on both meshes and the
               fine elements subdivide the coarse ones, so P^T (A_f (P x)) = A_c x; both actions are IGXComputeMatrixAction.
               Bound: with y1 = P x, y2 = A_f y1, y3 = P^T y2 each stage adds its own c u |stage| |input| and carries the earlier errors
               through |stage|: |lhs - rhs| <= u ((c_P + C_A + c_R) |P^T| |A_f| |P| |x| + C_A |A_c| |x|) with the assembled matrices'
               absolute values (Mat.to_scipy_global).  C_A = tensor_ref.C_ID = 128, the constant the action's own entrywise test holds
               it to on the identity geometry; |A| understates that test's S (signs cancel inside an entry), by a factor the 4x margin
               inside C_ID has covered in every case measured.  Largest observed ratio on an MI355X: see test_galerkin_identity.
               (Through the probe the largest |E_f - E_c| seen is 0.021 of its bound.)
  bit facts    no refinement: a bit-for-bit copy both ways (signed zeros included); clamped end rows copy boundary values bit for bit
               (values whose products with the table's entries are exact -- zero always); launch counts; whose figures last_timing()
               returns; the kernel's name.
  refusals     with vectors, and a stale transfer."""
import numpy as np
import pytest

import probe_ref as PR
import tensor_ref as T
import transfer_ref as TR
from test_gpu_transfer_entrywise import make, tables, u

pytestmark = pytest.mark.gpu
ARG_WRONG, ORDER = 62, 58


def _engines(dof, caxes, faxes):
    import petiga_amd as P
    out = []
    for axes in (caxes, faxes):
        g = P.IGX(len(axes), dof)
        for i, (p, U, periodic) in enumerate(axes):
            g.axis_knots(i, p, U, periodic=periodic)
        g.setup()
        out.append(g)
    return out


def _points(faxes, seed):
    dim = len(faxes)
    rng = np.random.default_rng(seed)
    lim = [(U[p], U[len(U) - 1 - p]) for p, U, _ in faxes]
    lo, hi = np.array([l[0] for l in lim]), np.array([l[1] for l in lim])
    rnd = lo + (hi - lo) * rng.random((200, dim))
    knots = [np.unique(U[p:len(U) - p]) for p, U, _ in faxes]
    onk = np.stack([rng.choice(k, 40) for k in knots], axis=1)                 # every coordinate a fine knot (evaluated from the right)
    mixed = np.where(rng.random((40, dim)) < 0.5, onk, rnd[:40])
    return np.concatenate([rnd, onk, mixed, lo[None, :], hi[None, :]])


def _annulus(kind):
    """coarse and fine 2-D spaces on the quarter annulus: (caxes, faxes, (Xc, Wc), (Xf, Wf)); kind "polynomial" drops the weights"""
    from petiga_amd import geometry as G
    deg, kn, Pw = G.quarter_annulus(2)
    kc, Pc = G.refine(deg, kn, Pw, [[0.5], [1.0 / 3, 2.0 / 3]])
    kf, Pf = G.refine(deg, kc, Pc, [[0.25, 0.75, 0.8], [1.0 / 6, 0.5, 0.5]])      # axis 1: 0.5 twice -> C0 there
    Xc, Wc = G.split_net(Pc)
    Xf, Wf = G.split_net(Pf)
    if kind == "polynomial":
        Xc, Xf, Wc, Wf = Pc.reshape(-1, 3)[:, :2].copy(), Pf.reshape(-1, 3)[:, :2].copy(), None, None      # the homogeneous net as a polynomial map: it refines exactly
    return [(deg[d], kc[d], False) for d in range(2)], [(deg[d], kf[d], False) for d in range(2)], (Xc, Wc), (Xf, Wf)


EXACT = ["identity-3d", "identity-periodic", "polynomial", "nurbs"]


@pytest.mark.parametrize("kind", EXACT)
def test_the_prolonged_vector_is_the_same_function(kind):
    dof = 2
    geo = None
    if kind == "identity-3d":
        caxes, faxes = [u(2, 3), u(3, 2), u(1, 2)], [u(2, 6), (3, TR.insert(TR.uniform_knots(3, 2), 3, [0.2, 0.5, 0.7]), False), u(1, 2)]
    elif kind == "identity-periodic":
        caxes, faxes = [u(2, 4, True), u(2, 2)], [u(2, 8, True), u(2, 6)]
    else:
        caxes, faxes, gc, gf = _annulus(kind)
        geo = (gc, gf)
    c, f = _engines(dof, caxes, faxes)
    if geo:
        c.set_geometry(*geo[0])
        f.set_geometry(*geo[1])
    t = f.transfer(c)
    mats, nrow, _ = tables(t)
    c_P = sum(nrow) + 1
    rng = np.random.default_rng(17)
    xc = rng.uniform(-1, 1, c.create_vec().n)
    wc = np.repeat(geo[0][1], dof) if (geo and geo[0][1] is not None) else 1.0
    wf = np.repeat(geo[1][1], dof) if (geo and geo[1][1] is not None) else 1.0
    Xc, Xf = c.create_vec().set(xc * wc), f.create_vec()
    t.prolong(Xc, Xf)
    xf = Xf.get() / wf                                                        # one more rounding per entry on a rational geometry
    Xc.set(xc)
    Xf.set(xf)
    _, SP = TR.prolong(mats, np.abs(xc * wc), dof)
    SP = (SP / wf).astype(np.float64) * (1 + 4 * TR.U_RND)
    pts = _points(faxes, 3)
    axes = lambda ax: [dict(p=p, U=np.asarray(U), nnp=TR.nnp_of(p, U, per), periodic=per) for p, U, per in ax]
    refc = PR.ProbeRef(axes(caxes), dof, *(geo[0] if geo else (None, None)))
    reff = PR.ProbeRef(axes(faxes), dof, *(geo[1] if geo else (None, None)))
    pc, pf = c.probe(pts, order=1), f.probe(pts, order=1)
    for der in (0, 1):
        Ec, Ef = pc.evaluate(Xc, der), pf.evaluate(Xf, der)
        _, Sc = refc.evaluate(xc, pts, der)
        _, Sf = reff.evaluate(SP, pts, der)
        cb = PR.bound(der, geo is not None)
        bound = TR.U_RND * (cb * Sc + (cb + c_P + 1) * Sf)
        err = np.abs(Ef.astype(TR.LD) - Ec.astype(TR.LD))
        worst = float(np.max(err / bound))
        print("%s der %d: %d points, |E_f - E_c| at most %.3g of its bound (largest difference %.3g)" % (kind, der, len(pts), worst, float(err.max())))
        assert worst <= 1.0
    pc.close(); pf.close(); t.close()


@pytest.mark.parametrize("p,nc", [(2, 3), (3, 2)])
def test_galerkin_identity(p, nc):
    """Largest observed |lhs - rhs| on an MI355X: 0.0084 of the bound at p = 2 (4.2e-16 of max |A_c x|), 0.0137 at p = 3 (6.2e-16); the
    figures are in profiles/transfer.txt."""
    c, f = _engines(1, [u(p, nc)] * 3, [u(p, 2 * nc)] * 3)
    for g in (c, f):
        g.set_form("poisson")
    t = f.transfer(c)
    mats, nrow, ncol = tables(t)
    c_P, c_R = sum(nrow) + 1, sum(ncol) + 1
    x = np.random.default_rng(23).uniform(-1, 1, c.create_vec().n)
    Xc, Yc, Xf, Yf, Zc = c.create_vec().set(x), c.create_vec(), f.create_vec(), f.create_vec(), c.create_vec()
    c.compute_matrix_action(Xc, Yc)
    t.prolong(Xc, Xf)
    f.compute_matrix_action(Xf, Yf)
    t.restrict(Yf, Zc)
    lhs, rhs = Zc.get(), Yc.get()
    Ac, Af = c.create_mat(), f.create_mat()
    c.compute_matrix(Ac)
    f.compute_matrix(Af)
    absAc, absAf = abs(Ac.to_scipy_global()), abs(Af.to_scipy_global())
    _, s1 = TR.prolong(mats, np.abs(x), 1)
    s2 = absAf @ s1.astype(np.float64)
    _, s3 = TR.restrict(mats, s2, 1)
    bound = TR.U_RND * ((c_P + T.C_ID + c_R) * s3.astype(np.float64) + T.C_ID * (absAc @ np.abs(x)))
    worst = float(np.max(np.abs(lhs - rhs) / bound))
    print("Galerkin p = %d, %d^3 -> %d^3 elements: |P^T A_f P x - A_c x| at most %.3g of its bound, %.3g of max|A_c x|" % (
        p, nc, 2 * nc, worst, float(np.max(np.abs(lhs - rhs)) / np.max(np.abs(rhs)))))
    assert worst <= 1.0
    assert np.max(np.abs(rhs)) > 1e-3                                           # not a comparison of zeros
    t.close()


def test_bit_facts_counts_and_names():
    import petiga_amd as P
    # no refinement: a bit-for-bit copy both ways, the sign of a zero included, on both paths
    c, f, dof = make("mixed-p137")
    c2 = _engines(dof, [u(1, 8), u(3, 3), u(7, 1)], [u(1, 8), u(3, 3), u(7, 1)])[1]
    t = c2.transfer(c)
    x = np.random.default_rng(2).standard_normal(c.create_vec().n)
    x[::7] = -0.0
    x[3::11] = 0.0
    for path in ("fused", "axis"):
        t.set_path(path)
        y = t.prolong(c.create_vec().set(x), c2.create_vec().fill(np.nan)).get()
        assert np.array_equal(y.view(np.int64), x.view(np.int64)), path
        assert c2.last_timing()[2] == 1 and c2.kernel_name() == "transfer_prolong(3d, p=1,3,7, 9x6x8 -> 9x6x8, dof 3, %s)" % ("fused" if path == "fused" else "axis passes")
    z = t.restrict(c2.create_vec().set(x), c.create_vec().fill(np.nan)).get()
    assert np.array_equal(z.view(np.int64), x.view(np.int64))
    assert c2.last_timing()[2] == 1 and c2.kernel_name() == "transfer_restrict(3d, p=1,3,7, 9x6x8 -> 9x6x8, dof 3, axis passes)"
    t.close()
    # clamped ends: boundary values arrive bit for bit (dyadic refinement, values of few bits; zero always)
    t = f.transfer(c)
    nc = [t.sizes(d)[1] for d in range(3)]
    nf = [t.sizes(d)[0] for d in range(3)]
    xc = np.random.default_rng(3).standard_normal((nc[2], nc[1], nc[0], dof))
    xc[:, :, 0, :], xc[:, :, -1, :], xc[0, :, :, 1], xc[:, -1, :, 2] = -2.5, 0.0, 0.375, 1.0
    xc[0, :, 0, 1], xc[0, :, -1, 1] = 0.375, 0.375
    xc[:, -1, 0, 2], xc[:, -1, -1, 2] = 1.0, 1.0
    Xc = c.create_vec().set(xc.reshape(-1))
    f.set_timing(True)
    for path, launches in (("fused", 1), ("axis", 3)):
        t.set_path(path)
        xf = t.prolong(Xc, f.create_vec().fill(np.nan)).get().reshape(nf[2], nf[1], nf[0], dof)
        assert np.all(xf[:, :, 0, 0] == -2.5) and np.all(xf[:, :, -1, 0] == 0.0) and np.all(xf[0, :, :, 1] == 0.375) and np.all(xf[:, -1, :, 2] == 1.0), path
        # launch counts and whose figures last_timing() returns: the call's own, read twice, kernel time = total
        total, kernel, n = f.last_timing()
        assert f.last_timing() == (total, kernel, n) and n == launches and 0 < kernel == total, (path, total, kernel, n)
        assert f.kernel_name() == "transfer_prolong(3d, p=1,3,7, 9x6x8 -> 17x9x9, dof 3, %s)" % ("fused" if path == "fused" else "axis passes")
    t.restrict(f.create_vec().set(np.ones(f.create_vec().n)), c.create_vec())
    total, kernel, n = f.last_timing()
    assert n == 3 and 0 < kernel == total and f.kernel_name() == "transfer_restrict(3d, p=1,3,7, 17x9x9 -> 9x6x8, dof 3, axis passes)"
    # another call on the fine IGX takes the figures over: a probe's single launch
    prb = f.probe(np.full((5, 3), 0.5), order=0)
    prb.evaluate(f.create_vec(), 0)
    assert f.kernel_name().startswith("probe(") and f.last_timing()[2] == 1
    f.set_timing(False)
    # one refined axis of three: one pass; 2-D and 1-D names
    c1, f1 = _engines(1, [u(2, 3), u(2, 3), u(2, 3)], [u(2, 3), u(2, 6), u(2, 3)])
    t1 = f1.transfer(c1).set_path("axis")
    t1.prolong(c1.create_vec(), f1.create_vec())
    assert f1.last_timing()[2] == 1 and f1.kernel_name() == "transfer_prolong(3d, p=2,2,2, 5x5x5 -> 5x8x5, dof 1, axis passes)"
    t1.restrict(f1.create_vec(), c1.create_vec())
    assert f1.last_timing()[2] == 1
    c2d, f2d, _ = make("2d-periodic")
    t2 = f2d.transfer(c2d)
    t2.prolong(c2d.create_vec(), f2d.create_vec())
    assert f2d.kernel_name() == "transfer_prolong(2d, p=2,2, 5x5 -> 10x11, dof 1, fused)"
    t.close(); t1.close(); t2.close()


def test_refusals_with_vectors_and_a_stale_transfer():
    import petiga_amd as P
    c, f, dof = make("clustered")
    t = f.transfer(c)
    Xc, Xf = c.create_vec(), f.create_vec()

    def refused(call, code, *words):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == code and "transfer" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: t.prolong(Xf, Xf), ARG_WRONG, "coarse vector", "another IGX")
    refused(lambda: t.prolong(Xc, Xc), ARG_WRONG, "fine vector", "another IGX")
    refused(lambda: t.restrict(Xc, Xc), ARG_WRONG, "fine vector")
    refused(lambda: t.restrict(Xf, Xf), ARG_WRONG, "coarse vector")
    refused(lambda: t.prolong(None, Xf), ARG_WRONG, "null vector")
    same = f.transfer(f)                                                      # a space is nested in itself
    refused(lambda: same.prolong(Xf, Xf), ARG_WRONG, "same one twice")
    assert np.array_equal(same.prolong(f.create_vec().fill(1.5), Xf).get(), np.full(Xf.n, 1.5))
    same.close()
    c.set_stream(0x40)                                                        # refused before any use of it
    refused(lambda: t.prolong(Xc, Xf), ARG_WRONG, "stream")
    refused(lambda: t.restrict(Xf, Xc), ARG_WRONG, "stream")
    c.set_stream(None)
    t.prolong(Xc, Xf)
    for which in (c, f):
        t2 = f.transfer(c)
        which.setup()
        refused(lambda: t2.prolong(c.create_vec(), f.create_vec()), ORDER, "stale", "IGXSetUp")
        refused(lambda: t2.restrict(f.create_vec(), c.create_vec()), ORDER, "stale")
        refused(lambda: t2.axis(0), ORDER, "stale")
        t2.close()
        t2.close()
    assert P.lib().IGXTransferDestroy(None) == 0
