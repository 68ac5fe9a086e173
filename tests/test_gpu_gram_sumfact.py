"""The p = 3 Gram walk on the identity geometry with its walk-axis contraction sum-factorised (pencil_mfma_sf in
petiga_amd/csrc/gram_mfma.hpp, the default; IGX_GRAM_SUMFACT=0: the 480-MFMA phase pencil_mfma).  Only the order of the summation
changes: both phases against the oracle to 1e-12, against each other to 1e-13 of the largest entry, the Dirichlet rows and the
fixed entries of F bit for bit.  Cases: non-uniform and open knot vectors, mixed Dirichlet faces (System driver), the Matrix and System drivers,
a periodic axis 0 (the axis-2 walk), segments of two elements, the ranks of a 2-rank partition."""
import numpy as np
import pytest

from common import compare_mats, make_pair

pytestmark = pytest.mark.gpu


def _faces(g, bc):
    if bc == "all":
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 1.0 + 0.5 * d - 0.25 * s)
    elif bc == "some":
        g.set_boundary_value(0, 0, 0, 0.5); g.set_boundary_value(1, 1, 0, -1.0); g.set_boundary_value(2, 0, 0, 2.0)
    elif bc == "yz":      # (axis 0 periodic)
        g.set_boundary_value(1, 0, 0, 0.5); g.set_boundary_value(2, 1, 0, -1.5)


def _assemble(monkeypatch, sumfact, N, driver, bc, knots=None, C=None, periodic=None, nseg=0):
    monkeypatch.setenv("IGX_GRAM_SUMFACT", str(sumfact))
    if nseg:
        monkeypatch.setenv("IGX_NSEG", str(nseg))
    else:
        monkeypatch.delenv("IGX_NSEG", raising=False)
    orc, eng = make_pair(3, 1, 3, list(N), C=C, periodic=periodic, knots=knots)
    for g in (orc, eng):
        _faces(g, bc)
    eng.set_form("poisson")
    A = eng.create_mat()
    b = eng.create_vec() if driver == "system" else None
    if b is None:
        eng.compute_matrix(A)
    else:
        eng.compute_system(A, b)
    eng.synchronize()
    assert "gram_pencil" in eng.kernel_name() and "p=3" in eng.kernel_name(), eng.kernel_name()
    return orc, eng, A, b


def _open_nonuniform(n, seed):
    """An open knot vector on [0, 1] with n non-uniform spans."""
    rng = np.random.default_rng(seed)
    h = 0.5 + rng.random(n)
    x = np.concatenate([[0.0], np.cumsum(h) / h.sum()])
    x[-1] = 1.0
    return np.concatenate([[0.0] * 3, x, [1.0] * 3])


CASES = [
    # N, driver, bc, knots / C / periodic, nseg
    ((9, 8, 7), "system", "all", dict(knots=[_open_nonuniform(9, 1), _open_nonuniform(8, 2), _open_nonuniform(7, 3)]), 0),
    ((10, 7, 6), "matrix", "none", dict(knots=[_open_nonuniform(10, 4), None, _open_nonuniform(6, 5)]), 0),
    ((12, 6, 5), "system", "some", dict(knots=[_open_nonuniform(12, 6), _open_nonuniform(6, 7), None]), 3),      # three segments: halo elements
    ((10, 8, 6), "system", "yz", dict(periodic=[True, False, False]), 0),      # periodic axis 0: the walk takes axis 2
    ((9, 7, 6), "matrix", "none", dict(periodic=[True, False, False]), 0),
    ((8, 6, 5), "system", "all", {}, 4),                                         # segments of two elements
    ((8, 8, 7), "matrix", "none", {}, 4),
]


@pytest.mark.parametrize("N,driver,bc,kw,nseg", CASES)
def test_sumfact_against_oracle_and_mfma_phase(N, driver, bc, kw, nseg, monkeypatch):
    orc, eng, A, b = _assemble(monkeypatch, 1, N, driver, bc, nseg=nseg, **kw)
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    if b is not None:
        assert np.abs(b.get() - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    vals, bv = A.host(True).copy(), (b.get().copy() if b is not None else None)
    _, eng0, A0, b0 = _assemble(monkeypatch, 0, N, driver, bc, nseg=nseg, **kw)
    vals0 = A0.host(True)
    rp, ci, _ = A0.host()
    assert np.abs(vals - vals0).max() <= 1e-13 * np.abs(vals0).max()
    if b is not None and bc != "none":      # Dirichlet rows (a lone diagonal) and the fixed entries of F: set, not summed -- bit for bit
        nnz_row = np.array([np.count_nonzero(vals0[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])
        fixed = np.flatnonzero(nnz_row == 1)
        assert fixed.size > 0
        for i in fixed:
            assert np.array_equal(vals[rp[i]:rp[i + 1]], vals0[rp[i]:rp[i + 1]])
        assert np.array_equal(bv[fixed], b0.get()[fixed])
    if b is not None:
        assert np.abs(bv - b0.get()).max() <= 1e-13 * np.abs(b0.get()).max()


def test_sumfact_repeatable_bitwise(monkeypatch):
    """The walk stays colour-ordered: two assemblies are identical."""
    _, eng, A, b = _assemble(monkeypatch, 1, (11, 9, 8), "system", "some")
    vals, bv = A.host(True).copy(), b.get().copy()
    eng.compute_system(A, b)
    eng.synchronize()
    assert np.array_equal(A.host(True), vals) and np.array_equal(b.get(), bv)


@pytest.mark.parametrize("size", [2])
def test_sumfact_on_a_partition(size, monkeypatch):
    """Every rank of a 2-rank partition (local rows before the ghost-row exchange): the two phases agree per rank."""
    import petiga_amd as P
    N = (10, 9, 16)
    out = {}
    for sf in (1, 0):
        monkeypatch.setenv("IGX_GRAM_SUMFACT", str(sf))
        for r in range(size):
            g = P.IGX(3, 1)
            for i in range(3):
                g.axis_uniform(i, 3, N[i])
            g.set_comm(size, r)
            g.setup()
            _faces(g, "all")
            g.set_form("poisson")
            A, b = g.create_mat(), g.create_vec()
            g.compute_system(A, b)
            g.synchronize()
            assert "gram_pencil" in g.kernel_name(), g.kernel_name()
            out[(sf, r)] = (A.host(True).copy(), b.get().copy())
    for r in range(size):
        (v1, b1), (v0, b0) = out[(1, r)], out[(0, r)]
        assert np.abs(v1 - v0).max() <= 1e-13 * np.abs(v0).max()
        assert np.abs(b1 - b0).max() <= 1e-13 * max(np.abs(b0).max(), 1.0)
