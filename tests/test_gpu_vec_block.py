"""IGXVecMDot and IGXVecMAXPY on the GPU (include/petiga_amd.h; petiga_amd/csrc/block_vec.hpp), entry by entry.
  lengths   175 (less than one step of a workgroup), 1025 and 1331 (odd; the 16-byte loads end in a single row), 274 625 (odd, and past one
            pass of the capped grid: 256 workgroups x 8 wavefronts x 32 rows = 65 536 rows per pass): the lengths of the Krylov tests
  blocks    (1, 1), (3, 5), (16, 16), (17, 16), (48, 48) and a pair of blocks that share columns
  MDot      every entry against the exact sum within n u sum_k |x_k y_k|, the bound of ANY summation order (Higham, Accuracy and Stability,
            3.1: gamma_n ~ n u), so it needs no measurement.  The yardstick for every entry is the sum in long double (64-bit mantissa: its own
            error, n 2^-64 sum |x y|, is 2^-11 of the bound); on a sample of entries -- the corners of the block and of every 16-wide tile
            -- it is math.fsum of the long-double products split in two doubles, which is exact.  The largest ratio error / bound seen is
            printed (on an MI355X: see DESIGN.md 3.21).  Two calls agree bit for bit.  A column past nx that is poisoned with NaN is never read.
  MAXPY     every entry against long double within (nx + 2) u (|beta y| + sum_i |C_ij x_i|): nx fused multiply-adds and the product beta y,
            each one rounding of a partial sum that the bound's parenthesis majorises; beta in {0, 1, -0.5}; beta = 0 over a NaN-filled Y
  refusals  that need vectors: a foreign vector, aliasing in MAXPY
  figures   IGXGetKernelName and IGXGetLastTiming's launch count cover both calls
Every test prints what it sees before it asserts (run with -s)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
ARG_WRONG = 62
LENGTHS = {175: (5, 3, 3), 1025: (3, 3, 39), 1331: (9, 9, 9), 274625: (63, 63, 63)}      # elements per axis at p = 2: n = prod(N + 2)
BLOCKS = [(1, 1), (3, 5), (16, 16), (17, 16), (48, 48)]


@functools.lru_cache(maxsize=None)
def engine(n):
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, LENGTHS[n][i])
    g.setup()
    return g


@functools.lru_cache(maxsize=None)
def columns(n):
    """(engine, 48 X vectors, 48 Y vectors, their host values [48, n] twice): made once, never written to"""
    g = engine(n)
    rng = np.random.default_rng(n)
    hx, hy = rng.standard_normal((48, n)), rng.standard_normal((48, n)) * np.exp(rng.uniform(-3, 3, (48, 1)))
    X, Y = [g.create_vec().set(hx[i]) for i in range(48)], [g.create_vec().set(hy[j]) for j in range(48)]
    assert X[0].n == n
    hx.setflags(write=False)
    hy.setflags(write=False)
    return g, X, Y, hx, hy


def long_double_gram(hx, hy):
    """(X Y^T in long double, sum |x y| in double) by chunks of rows"""
    nx, ny, n = hx.shape[0], hy.shape[0], hx.shape[1]
    G, S = np.zeros((nx, ny), dtype=np.longdouble), np.zeros((nx, ny))
    for a in range(0, n, 8192):
        xl, yl = hx[:, a:a + 8192].astype(np.longdouble), hy[:, a:a + 8192].astype(np.longdouble)
        G += xl @ yl.T
        S += np.abs(hx[:, a:a + 8192]) @ np.abs(hy[:, a:a + 8192]).T
    return G, S


@functools.lru_cache(maxsize=None)
def reference(n):
    _, _, _, hx, hy = columns(n)
    return long_double_gram(hx, hy)


def exact_dot(x, y):
    """math.fsum of the long-double products, each split into two doubles: the exact sum of the products as long double holds them"""
    p = x.astype(np.longdouble) * y.astype(np.longdouble)
    hi = p.astype(np.float64)
    lo = (p - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]).tolist())


def sample_entries(nx, ny):
    rows = sorted({i for i in (0, 15, 16, 31, 32, nx - 1) if 0 <= i < nx})
    cols = sorted({j for j in (0, 15, 16, 31, 32, ny - 1) if 0 <= j < ny})
    return [(i, j) for i in rows for j in cols if (i + j) % 2 == 0 or (i, j) == (nx - 1, ny - 1)]


@pytest.mark.parametrize("n", sorted(LENGTHS))
@pytest.mark.parametrize("nx,ny", BLOCKS)
def test_mdot_entry_by_entry(n, nx, ny):
    import petiga_amd as P
    g, X, Y, hx, hy = columns(n)
    Gl, S = reference(n)
    G = P.Vec.mdot(X[:nx], Y[:ny])
    name, (_, _, launches) = g.kernel_name(), g.last_timing()
    G2 = P.Vec.mdot(X[:nx], Y[:ny])
    bound = n * U * S[:nx, :ny]
    ratio = float((np.abs(G.astype(np.longdouble) - Gl[:nx, :ny]).astype(np.float64) / bound).max())
    worst = 0.0
    for i, j in sample_entries(nx, ny):
        worst = max(worst, abs(G[i, j] - exact_dot(hx[i], hy[j])) / bound[i, j])
    print("mdot %d x %d, n = %d: largest error / (n u sum|x y|) = %.3e against long double, %.3e against the exact sum on %d sampled entries; %s, %d launches"
          % (nx, ny, n, ratio, worst, len(sample_entries(nx, ny)), name, launches))
    assert G.shape == (nx, ny) and np.all(np.isfinite(G))
    assert ratio <= 1.0 and worst <= 1.0
    assert np.array_equal(G, G2), "two calls differ"
    assert name.startswith("vec_mdot(%d x %d, mfma_f64_16x16x4" % (nx, ny)) and launches == 2, (name, launches)


@pytest.mark.parametrize("n", sorted(LENGTHS))
def test_mdot_shared_columns_and_gram(n):
    import petiga_amd as P
    g, X, Y, hx, hy = columns(n)
    A, B = X[:5], [X[2], X[0], Y[1]]
    ha, hb = hx[:5], np.stack([hx[2], hx[0], hy[1]])
    G = P.Vec.mdot(A, B)
    Gl, S = long_double_gram(ha, hb)
    ratio = float((np.abs(G.astype(np.longdouble) - Gl).astype(np.float64) / (n * U * S)).max())
    # X == Y: a Gram matrix; it is symmetric bit for bit, because entry (i, j) and entry (j, i) add the same products in the same order
    W = P.Vec.mdot(X[:17], X[:17])
    Wl, Sw = long_double_gram(hx[:17], hx[:17])
    ratio_w = float((np.abs(W.astype(np.longdouble) - Wl).astype(np.float64) / (n * U * Sw)).max())
    print("n = %d: shared columns 5 x 3: error / bound %.3e; Gram 17 x 17: %.3e, max |W - W^T| = %.3e" % (n, ratio, ratio_w, np.abs(W - W.T).max()))
    assert ratio <= 1.0 and ratio_w <= 1.0
    assert np.all(np.diag(W) > 0) and np.array_equal(W, W.T)


def test_mdot_never_reads_a_column_past_the_block():
    """the arrays hold 48 entries, the block 17 x 3: entries 17.. of X and 3.. of Y are vectors full of NaN"""
    import ctypes as C
    import petiga_amd as P
    n = 1331
    g, X, Y, hx, hy = columns(n)
    poison = g.create_vec().set(np.full(n, np.nan))
    xs, ys = X[:17] + [poison] * 31, Y[:3] + [poison] * 45
    G = np.zeros((17, 3))
    P._ck(P.lib().IGXVecMDot(17, P._vec_array(xs), 3, P._vec_array(ys), G.ctypes.data_as(C.POINTER(C.c_double))))
    Gl, S = reference(n)
    print("poisoned columns past 17 x 3: finite = %s" % bool(np.all(np.isfinite(G))))
    assert np.all(np.isfinite(G))
    assert float((np.abs(G.astype(np.longdouble) - Gl[:17, :3]).astype(np.float64) / (n * U * S[:17, :3])).max()) <= 1.0


@pytest.mark.parametrize("n", sorted(LENGTHS))
@pytest.mark.parametrize("nx,ny", BLOCKS)
def test_maxpy_entry_by_entry(n, nx, ny):
    import petiga_amd as P
    g, X, _, hx, hy = columns(n)
    rng = np.random.default_rng(nx * 100 + ny)
    Cm = rng.standard_normal((nx, ny))
    base = Cm.T.astype(np.longdouble) @ hx[:nx].astype(np.longdouble)      # the long-double reference of the sum, once for the three beta
    base_mag = np.abs(Cm.T) @ np.abs(hx[:nx])
    Out = [g.create_vec() for _ in range(ny)]
    worst = 0.0
    for beta in (0.0, 1.0, -0.5):
        y0 = np.full((ny, n), np.nan) if beta == 0.0 else hy[:ny]
        for j in range(ny):
            Out[j].set(y0[j])
        P.Vec.maxpy(Out, X[:nx], Cm, beta)
        name, (_, _, launches) = g.kernel_name(), g.last_timing()
        got = np.stack([v.get() for v in Out])
        ref, mag = base.copy(), base_mag.copy()
        if beta != 0.0:
            ref += np.longdouble(beta) * y0.astype(np.longdouble)
            mag += np.abs(beta * y0)
        ratio = float((np.abs(got.astype(np.longdouble) - ref).astype(np.float64) / ((nx + 2) * U * mag)).max())
        worst = max(worst, ratio)
        print("maxpy %d -> %d, n = %d, beta = %g: largest error / ((nx + 2) u (|beta y| + sum |C x|)) = %.3e; %s" % (nx, ny, n, beta, ratio, name))
        assert np.all(np.isfinite(got)) and ratio <= 1.0
        assert name.startswith("vec_maxpy(%d -> %d" % (nx, ny)) and launches == 1, (name, launches)
    # the inputs are untouched
    assert np.array_equal(X[0].get(), hx[0]) and np.array_equal(X[nx - 1].get(), hx[nx - 1])


def test_refusals_that_need_vectors():
    import petiga_amd as P
    g, X, Y, _, _ = columns(175)
    other = engine(1025).create_vec()
    Cm = np.ones((2, 2))
    for call in (lambda: P.Vec.mdot([X[0], other], Y[:2]), lambda: P.Vec.mdot(X[:2], [Y[0], other]), lambda: P.Vec.maxpy([Y[0], other], X[:2], Cm)):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == ARG_WRONG and "different IGX" in str(e.value)
    out = [g.create_vec(), g.create_vec()]
    for ys, xs, word in (([out[0], X[1]], X[:2], "also a vector of X"), ([out[0], out[0]], X[:2], "twice"), ([X[0], out[1]], X[:2], "also a vector of X")):
        with pytest.raises(P.IGXError) as e:
            P.Vec.maxpy(ys, xs, Cm)
        assert e.value.code == ARG_WRONG and word in str(e.value), str(e.value)
    with pytest.raises(P.IGXError) as e:
        P.Vec.mdot([X[0], None], Y[:2])
    assert e.value.code == ARG_WRONG and "null vector" in str(e.value)
    # X may repeat a vector in MDot and in MAXPY's inputs
    G = P.Vec.mdot([X[0], X[0]], [X[0]])
    assert G[0, 0] == G[1, 0] > 0
    P.Vec.maxpy(out, [X[0], X[0]], np.array([[1.0, 0.0], [1.0, 0.0]]), 0.0)
    assert np.array_equal(out[0].get(), 2.0 * X[0].get()) and not out[1].get().any()
