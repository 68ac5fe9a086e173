"""A long double restatement of the transfer's contract (IGXTransfer, include/petiga_amd.h): for two nested knot vectors of one degree the
nf x nc matrix T with B^c_j = sum_i T[i][j] B^f_i, and P = T2 (x) T1 (x) T0 (x) I_dof applied to vectors in the engine's natural
numbering [n2][n1][n0][dof].

  matrix_rowwise       every row directly: the blossom of the coarse polynomial piece on the coarse span that holds the fine knot t_i, at the
                       fine knots t_i+p .. t_i+1, by de Boor's triangle on the unit vectors -- p levels of convex combinations, the recursion
                       IGXTransferCreate uses, here in long double.  A periodic axis is built on the unwrapped knot sequence of one
                       period, U[p+1 .. p+nnp], continued by the period, and folded: row i < nnp_f, column j mod nnp_c.
  matrix_by_insertion  an independent construction: geometry.insert_knot (Boehm) on an identity net, one knot at a time (double).
  basis                every function of a knot vector at points, by scipy.interpolate.BSpline (the witness of function equality).
  bands                (first, count, T [nf, p+1]) of a dense matrix in IGXTransferGetAxis' layout.
  prolong / restrict   P x and P^T r in long double from per-axis band tables, with the sums of absolute terms S.

wrong: one of the perturbed constructions of the teeth test -- "first" (every band shifted by one column), "left" (the span of a fine knot
taken from the left at a coarse knot), "multiplicity" (a repeated coarse knot counted once), "unfolded" (a periodic row not folded: the
columns past nnp_c dropped), "transpose" (the table transposed; square cases only)."""
import numpy as np

LD = np.longdouble
U_RND = 2.0 ** -53


def nnp_of(p, U, periodic):
    """functions of the axis: len(U) - p - 1, less the C + 1 that a periodic axis wraps (src/petigaaxis.c:286-312)"""
    U = np.asarray(U, dtype=np.float64)
    n = len(U) - p - 2
    if not periodic:
        return n + 1
    s = int(np.sum(U[n + 1:] == U[n + 1]))
    return n - (p - s)


def _ext(p, U, nnp, a, b):
    """the periodic knot sequence at any index: the knots of one period U[p+1 .. p+nnp] continued by the period, by one formula for both
    axes.  The continued knots are DOUBLES by definition (this formula evaluated in double, as IGXTransferCreate does): they are data of
    the contract like the given knots, so equal knots of the two axes stay equal and the reference sees the knots the engine sees."""
    K, a, b = [np.float64(v) for v in U[p + 1:p + 1 + nnp]], np.float64(a), np.float64(b)
    L = b - a

    def at(j):
        k, r = divmod(j - (p + 1), nnp)
        v = K[r]
        if k == 0:
            return LD(v)
        return LD(a - (np.float64(-k - 1) * L + (b - v))) if k < 0 else LD(b + (np.float64(k - 1) * L + (v - a)))
    return at


def matrix_rowwise(p, Uc, Uf, periodic=False, wrong=None):
    """dense T [nf, nc], long double"""
    Uc, Uf = np.asarray(Uc, dtype=np.float64), np.asarray(Uf, dtype=np.float64)
    nc_true, nf = nnp_of(p, Uc, periodic), nnp_of(p, Uf, periodic)
    if wrong == "multiplicity":                      # (the table keeps its shape: the columns lost are left empty)
        Uc = np.concatenate([Uc[:p + 1], np.unique(Uc[p + 1:len(Uc) - p - 1]), Uc[len(Uc) - p - 1:]])
    nc = nnp_of(p, Uc, periodic)
    if periodic:
        a, b = Uf[p], Uf[len(Uf) - 1 - p]
        cu, tf, mu, last = _ext(p, Uc, nc, a, b), _ext(p, Uf, nf, a, b), -(nc + p + 1), None
    else:
        cu, tf, mu, last = (lambda j: LD(Uc[j])), (lambda i: LD(Uf[i])), p, len(Uc) - p - 2
    T = np.zeros((nf, nc), dtype=LD)
    for i in range(nf):
        t0 = tf(i)
        if wrong == "left":
            while (last is None or mu + 1 <= last) and cu(mu + 1) < t0:
                mu += 1
        else:
            while (last is None or mu + 1 <= last) and cu(mu + 1) <= t0:
                mu += 1
        D = np.eye(p + 1, dtype=LD)
        for k in range(1, p + 1):
            x = tf(i + p + 1 - k)
            for jj in range(p, k - 1, -1):
                j = mu - p + jj
                den = cu(j + p + 1 - k) - cu(j)
                w = (x - cu(j)) / den if den != 0 else LD(0)
                D[jj] = (1 - w) * D[jj - 1] + w * D[jj]
        for q in range(p + 1):
            j = mu - p + q + (1 if wrong == "first" else 0)
            if periodic and wrong != "unfolded":
                j %= nc
            if 0 <= j < nc:
                T[i, j] += D[p, q]
    if nc != nc_true:
        T = np.concatenate([T, np.zeros((nf, nc_true - nc), dtype=LD)], axis=1)
    return T.T.copy() if wrong == "transpose" else T


def matrix_by_insertion(p, Uc, Uf):
    """dense T [nf, nc] (double) on a clamped axis: Boehm's insertion of every new knot, one at a time, on an identity net"""
    from petiga_amd.geometry import insert_knot
    Uc, Uf = np.asarray(Uc, dtype=np.float64), np.asarray(Uf, dtype=np.float64)
    new, rest = [], list(Uc)
    for v in Uf:
        if rest and rest[0] == v:
            rest.pop(0)
        else:
            new.append(float(v))
    assert not rest, "the knot vectors are not nested"
    U, Pw = Uc.copy(), np.eye(len(Uc) - p - 1)
    for v in new:
        U, Pw = insert_knot(p, U, Pw, v, 0)
    assert np.array_equal(U, Uf)
    return Pw


def basis(p, U, x, periodic=False):
    """[nx, nnp] (double): every function of the axis at the points x of [U[p], U[m-p]]; a periodic axis adds function i >= nnp to i - nnp"""
    from scipy.interpolate import BSpline
    U, x = np.asarray(U, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n = len(U) - p - 1
    B = np.stack([np.nan_to_num(BSpline.basis_element(U[i:i + p + 2], extrapolate=False)(x)) for i in range(n)], axis=1)
    right = x == U[len(U) - 1 - p]                    # basis_element is right-open: the upper end belongs to the last span
    if np.any(right):
        eps = np.nextafter(x[right], -np.inf)
        B[right] = np.stack([np.nan_to_num(BSpline.basis_element(U[i:i + p + 2], extrapolate=False)(eps)) for i in range(n)], axis=1)
    nnp = nnp_of(p, U, periodic)
    out = np.zeros((len(x), nnp))
    for i in range(n):
        out[:, i % nnp] += B[:, i]
    return out


def function_gap(p, Uc, Uf, T, periodic=False, npts=400, seed=0):
    """max over points and coarse functions of |B^c_j(x) - sum_i T[i][j] B^f_i(x)|: npts random points of the axis, away from the knots by
    nothing in particular, plus every knot from the right"""
    Uf = np.asarray(Uf, dtype=np.float64)
    a, b = Uf[p], Uf[len(Uf) - 1 - p]
    x = np.concatenate([a + (b - a) * np.random.default_rng(seed).random(npts), np.unique(Uf[p:len(Uf) - p])[:-1]])
    return float(np.max(np.abs(basis(p, Uc, x, periodic) - basis(p, Uf, x, periodic) @ np.asarray(T, dtype=np.float64))))


def bands(T, periodic=False):
    """(first, count, band [nf, w]) of a dense matrix: the non-zeros of every row must be consecutive (cyclically on a periodic axis)"""
    T = np.asarray(T)
    nf, nc = T.shape
    first, count, rows = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64), []
    for i in range(nf):
        nz = np.flatnonzero(T[i] != 0)
        assert len(nz), "row %d is empty" % i
        start = int(nz[0])
        if periodic and nz[0] == 0 and nz[-1] == nc - 1 and len(nz) < nc:      # the band wraps: it starts after the gap
            gap = np.flatnonzero(np.diff(nz) > 1)
            assert len(gap) == 1, "row %d: the non-zeros are not consecutive" % i
            start = int(nz[gap[0] + 1])
        cols = (start + np.arange(len(nz))) % nc
        assert sorted(cols) == sorted(nz), "row %d: the non-zeros are not consecutive" % i
        first[i], count[i] = start, len(nz)
        rows.append(T[i, cols])
    w = int(count.max())
    band = np.zeros((nf, w), dtype=T.dtype)
    for i, r in enumerate(rows):
        band[i, :len(r)] = r
    return first, count, band


def dense(first, count, band, nc):
    """the dense long double matrix of band tables (IGXTransferGetAxis' layout; columns (first + k) mod nc)"""
    nf = len(first)
    T = np.zeros((nf, nc), dtype=LD)
    for i in range(nf):
        for k in range(int(count[i])):
            T[i, (int(first[i]) + k) % nc] += LD(band[i, k])
    return T


def _kron_apply(mats, x, dof):
    """(y, S): (M2 (x) M1 (x) M0 (x) I_dof) x and the sum of absolute terms, x in natural numbering [n2][n1][n0][dof]; mats[d] is
    [nout_d, nin_d]"""
    nin = [m.shape[1] for m in mats]
    v = np.asarray(x, dtype=LD).reshape(nin[2], nin[1], nin[0], dof)
    a = np.abs(v)
    for d, sub in ((0, "ax,zyxc->zyac"), (1, "ay,zyxc->zaxc"), (2, "az,zyxc->ayxc")):
        M = np.asarray(mats[d], dtype=LD)
        v, a = np.einsum(sub, M, v), np.einsum(sub, np.abs(M), a)
    return v.reshape(-1), a.reshape(-1)


def prolong(mats, xc, dof):
    """(R, S) of P xc; mats: the dense per-axis matrices [nf_d, nc_d], three of them (identity [[1]] beyond dim)"""
    return _kron_apply(mats, xc, dof)


def restrict(mats, rf, dof):
    """(R, S) of P^T rf"""
    return _kron_apply([np.asarray(m).T for m in mats], rf, dof)


def uniform_knots(p, N, C=None, periodic=False, a=0.0, b=1.0):
    """IGAAxisInitUniform's knot vector (src/petigaaxis.c:401-456)"""
    C = p - 1 if C is None else C
    s = p - C
    m = 2 * (p + 1) + (N - 1) * s - 1
    n = m - p - 1
    U = np.zeros(m + 1)
    U[:p + 1], U[m - p:] = a, b
    k = p + 1
    for e in range(1, N):
        for _ in range(s):
            U[k] = a + e / N * (b - a)
            k += 1
    if periodic:
        for k in range(C + 1):
            U[C - k] = U[p] - U[m - p] + U[n - k]
            U[m - C + k] = U[m - p] - U[p] + U[p + 1 + k]
    return U


def insert(U, p, new):
    """the knot vector with the values `new` inserted (a clamped axis: the ends stay)"""
    return np.sort(np.concatenate([np.asarray(U, dtype=np.float64), np.asarray(new, dtype=np.float64)]))
