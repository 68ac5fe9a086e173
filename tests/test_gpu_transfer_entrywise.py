"""IGXTransferProlong / IGXTransferRestrict on the GPU (petiga_amd/csrc/transfer.hpp) against tests/transfer_ref.py applied with THE ENGINE'S
OWN TABLES (IGXTransferGetAxis; the tables themselves are held to the reference in tests/test_transfer_abi.py), every entry of every
vector, both paths of the prolongation, and the adjointness of the pair through IGXVecDot.

The bound is |E - R| <= c u S, S the long double sum of absolute terms of the nested sum, u = 2^-53.
  c.  An output entry is three nested chains, one per axis: the first product, then one fma per further term.  A chain of n terms carries
  n roundings, each relative to a partial sum that S dominates, so its error is at most n u S to first order, and nesting adds the counts:
  c = n0 + n1 + n2 + 1, the 1 for the second-order terms (and for add's one addition).  For the prolongation n_d is the longest row of
  axis d (at most p_d + 1), for the restriction the longest COLUMN (unbounded: 11 on the clustered axis here).
  Adjointness.  <P^T r, x> and <r, P x> each carry the transfer's c and the dot product's rounding: a product, per-lane sums of at most
  3 terms at these lengths, a wavefront tree of 6, 8 wavefronts and 256 partials in order (krylov.hpp): C_DOT = 1 + 3 + 6 + 8 + 256 = 274.
  Both sides are bounded by sum |r| |P| |x|, so |lhs - rhs| <= (c_P + c_R + 2 C_DOT) u sum |r| |P| |x|.

Shapes, from TR_FX x TR_FY x TR_FZ = 16 x 8 x 8 fine rows per box (transfer.hpp; Transfer.info() reports them): per axis one box (16, 8),
a box plus one row (17, 9), two boxes plus a partial one (35, 19).  Largest observed ratios |E - R| / (u S) on an MI355X: see the
docstring of test_every_entry_both_ways."""
import numpy as np
import pytest

import transfer_ref as TR

pytestmark = pytest.mark.gpu
BOX = (16, 8, 8)
C_DOT = 274


def _cluster(p, N, k=10):
    U = TR.uniform_knots(p, N)
    b = np.unique(U)
    return TR.insert(U, p, b[1] + (b[2] - b[1]) * (np.arange(1, k + 1) / (k + 1.5)) ** 2)


def _c0(p, N):
    U = TR.uniform_knots(p, N)
    return TR.insert(U, p, np.repeat(np.unique(U)[1:-1], p - 1))


def u(p, N, periodic=False):
    return (p, TR.uniform_knots(p, N, periodic=periodic), periodic)


# name -> (dof, coarse axes, fine axes); an axis is (p, U, periodic).  Fine extents in the comments.
SPACES = {
    # degrees 1, 3, 7, dof 3: 17 x 9 x 9 = a box plus one row on every axis
    "mixed-p137": (3, [u(1, 8), u(3, 3), u(7, 1)], [u(1, 16), u(3, 6), u(7, 2)]),
    # p = 2, dof 1: 35 (3x: two boxes plus 3) x 8 (one box) x 19 (UNREFINED: two boxes plus 3)
    "p2-35x8x19": (1, [u(2, 11), u(2, 3), u(2, 17)], [u(2, 33), u(2, 6), u(2, 17)]),
    # dof 4, axis 0 clustered (ten knots in one span: 16 = one box; restriction rows of 11 terms), 10 x 6 on the others
    "clustered": (4, [u(2, 4), u(2, 4), u(2, 2)], [(2, _cluster(2, 4), False), u(2, 8), u(2, 4)]),
    # dof 8, p = 3, 19 (unrefined) x 11 x 11: a box's footprint needs 86016 bytes of LDS, so the prolongation falls back to the axis passes
    "no-fit": (8, [u(3, 16), u(3, 4), u(3, 4)], [u(3, 16), u(3, 8), u(3, 8)]),
    # 2-D, one periodic axis (5 -> 10 functions), the other 3x
    "2d-periodic": (1, [u(2, 5, True), u(2, 3)], [u(2, 10, True), u(2, 9)]),
    # 3-D, a periodic coarse axis of p + 1 = 3 < 2p + 1 functions refined 4x; 17 on axis 1
    "periodic-small": (3, [u(2, 3, True), u(3, 7), u(1, 2)], [u(2, 12, True), u(3, 14), u(1, 4)]),
    # 1-D, dof 3, multiplicity raised to C0 on the fine side: 31 functions
    "1d-c0": (3, [u(3, 5)], [(3, _c0(3, 10), False)]),
}


def make(name):
    import petiga_amd as P
    dof, caxes, faxes = SPACES[name]
    out = []
    for axes in (caxes, faxes):
        g = P.IGX(len(axes), dof)
        for i, (p, U, periodic) in enumerate(axes):
            g.axis_knots(i, p, U, periodic=periodic)
        g.setup()
        out.append(g)
    return out[0], out[1], dof


def tables(t):
    """the engine's own per-axis tables as dense long double matrices, and the longest row and column of every axis"""
    mats, nrow, ncol = [], [], []
    for d in range(3):
        nf, nc, _ = t.sizes(d)
        first, count, band = t.axis(d)
        M = TR.dense(first, count, band, nc)
        mats.append(M)
        nrow.append(int(count.max()))
        ncol.append(int((M != 0).sum(axis=0).max()))
    return mats, nrow, ncol


def ratio(E, R, S, what):
    E, R, S = np.asarray(E, dtype=TR.LD), np.asarray(R, dtype=TR.LD), np.asarray(S, dtype=TR.LD)
    assert E.shape == R.shape and np.all(np.isfinite(E.astype(np.float64))), what
    err = np.abs(E - R)
    assert not np.any(err[S == 0] != 0), "%s: an entry with S = 0 is not exact" % what
    r = np.zeros(err.shape, dtype=TR.LD)
    r[S != 0] = err[S != 0] / (TR.LD(TR.U_RND) * S[S != 0])
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("name", list(SPACES))
def test_every_entry_both_ways(name):
    """Largest observed ratios |E - R| / (u S) on an MI355X, prolongation (both paths alike) / restriction, with the bounds c:
    mixed-p137 1.76 (8) / 1.37 (10); p2-35x8x19 1.99 (7) / 1.71 (13); clustered 2.74 (8) / 1.50 (19); no-fit 2.40 (8) / 1.71 (12);
    2d-periodic 2.40 (7) / 0.77 (13); periodic-small 1.90 (9) / 1.02 (19); 1d-c0 1.20 (7) / 0.93 (22).  Adjointness: at most 0.15 u sum |r| |P| |x|
    (c = 566..577).  The table is in profiles/transfer.txt."""
    c, f, dof = make(name)
    t = f.transfer(c)
    assert t.info()["box"] == tuple(min(BOX[d], t.sizes(d)[0]) for d in range(3))
    mats, nrow, ncol = tables(t)
    c_P, c_R = sum(nrow) + 1, sum(ncol) + 1
    rng = np.random.default_rng(5)
    xc, rf = rng.uniform(-1, 1, c.create_vec().n), rng.uniform(-1, 1, f.create_vec().n)
    Xc, Xf, Rf, Rc = c.create_vec().set(xc), f.create_vec(), f.create_vec().set(rf), c.create_vec()
    RP, SP = TR.prolong(mats, xc, dof)
    RR, SR = TR.restrict(mats, rf, dof)
    fits = t.info()["fused"]
    assert fits == (name != "no-fit")
    for path in (("fused", "axis") if fits else ("auto", "axis")):
        t.set_path(path)
        Xf.fill(np.nan)                                      # a poisoned vector is fully overwritten
        t.prolong(Xc, Xf)
        E = Xf.get()
        w = ratio(E, RP, SP, "%s prolong %s" % (name, path))
        print("%s: prolong, %s: %d entries, worst %.2f u S (c = %d); %s" % (name, path, E.size, w, c_P, f.kernel_name()))
        assert w <= c_P
        assert ("fused)" if path == "fused" else "axis passes)") in f.kernel_name()
        E2 = t.prolong(Xc, Xf.fill(np.nan)).get()
        assert np.array_equal(E, E2)                          # bit-repeatable
        # add: xf += P xc, one more rounding per entry -- equal to prolong-then-AXPBY
        y0 = rng.uniform(-1, 1, E.size)
        Ya = t.prolong(Xc, f.create_vec().set(y0), add=True).get()
        Yb = f.create_vec().set(y0).axpby(1.0, Xf, 1.0).get()
        assert np.max(np.abs(Ya - Yb) - TR.U_RND * np.abs(Yb)) <= 0
        w = ratio(Ya, RP + y0, SP + np.abs(y0), "%s prolong add %s" % (name, path))
        assert w <= c_P
    if not fits:
        import petiga_amd as P
        with pytest.raises(P.IGXError) as e:
            t.set_path("fused")
        assert e.value.code == 56 and "LDS" in str(e.value) and "transfer" in str(e.value)
    t.set_path("auto")
    Rc.fill(np.nan)
    t.restrict(Rf, Rc)
    E = Rc.get()
    w = ratio(E, RR, SR, "%s restrict" % name)
    print("%s: restrict: %d entries, longest rows %s, worst %.2f u S (c = %d); %s" % (name, E.size, ncol, w, c_R, f.kernel_name()))
    assert w <= c_R and "axis passes)" in f.kernel_name() and f.kernel_name().startswith("transfer_restrict(")
    assert np.array_equal(E, t.restrict(Rf, Rc.fill(np.nan)).get())
    if name == "clustered":
        assert ncol[0] >= 8                                    # the gather's variable loop: a long row
    # adjointness through the library's own dot products
    lhs, rhs = Rc.dot(Xc), Rf.dot(t.prolong(Xc, Xf))
    T = float(np.dot(np.abs(rf).astype(TR.LD), SP))
    c_adj = c_P + c_R + 2 * C_DOT
    print("%s: <P^T r, x> = %.17g, <r, P x> = %.17g, difference %.2f u sum|r||P||x| (c = %d)" % (name, lhs, rhs, abs(lhs - rhs) / (TR.U_RND * T), c_adj))
    assert abs(lhs - rhs) <= c_adj * TR.U_RND * T
    t.close()
