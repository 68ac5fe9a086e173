"""gram_pencil_patch3 (petiga_amd/csrc/gram_patch3.hpp, round 8): the p = 3 Gram walk in patches of pencils whose wavefronts add into ONE
window of band rows in LDS -- combined across all three axes before a run reaches memory.  The element phase is the sum-factorised
pencil walk's and the walk stays bit-repeatable: it reports itself as a Gram pencil walk ("gram_pencil(...,p=3,walk=0,MXxMY pencils per
workgroup,one window)").  IGX_PATCH3=2 forces it wherever it covers the configuration, IGX_PATCH3=0 keeps the pencil walk.
Engine vs oracle (demo/Poisson3D.c through IGAComputeMatrix / IGAComputeSystem): pattern bit-exact, values to 1e-12, and entry by entry
against the tensor-product reference (tests/tensor_ref.py); against the pencil walk to 1e-13, the Dirichlet rows and fixed F bit for bit."""
import ctypes as C

import numpy as np
import pytest

import tensor_ref as T
from common import compare_mats, make_pair

pytestmark = pytest.mark.gpu

PATCH = "pencils per workgroup,one window"


def _poison(mat):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    _, _, val = mat.device_ptrs()
    assert hip.hipMemset(val, 0xFF, mat.nblocks * mat.bs * mat.bs * 8) == 0
    assert hip.hipDeviceSynchronize() == 0


def _open_nonuniform(n, seed):
    """An open knot vector on [0, 1] with n non-uniform spans."""
    rng = np.random.default_rng(seed)
    h = 0.5 + rng.random(n)
    x = np.concatenate([[0.0], np.cumsum(h) / h.sum()])
    x[-1] = 1.0
    return np.concatenate([[0.0] * 3, x, [1.0] * 3])


def _bcs(kind):
    if kind == "all":
        return {(d, s, 0): 1.0 + 0.5 * d - 0.25 * s for d in range(3) for s in range(2)}
    if kind == "some":
        return {(0, 0, 0): 0.5, (1, 1, 0): -1.0, (2, 0, 0): 2.0}
    if kind == "yz":
        return {(1, 0, 0): 0.75, (2, 1, 0): -1.5}
    return {}


def _env(monkeypatch, patch3, nseg=0, sumfact=None):
    monkeypatch.setenv("IGX_PATCH3", str(patch3))
    for k, v in (("IGX_NSEG", nseg), ("IGX_GRAM_SUMFACT", sumfact)):
        if v:
            monkeypatch.setenv(k, str(v))
        else:
            monkeypatch.delenv(k, raising=False)


def _assemble(eng, driver, poison=True):
    eng.set_form("poisson")
    A = eng.create_mat()
    b = eng.create_vec() if driver == "system" else None
    if poison:
        _poison(A)
    if b is None:
        eng.compute_matrix(A)
    else:
        eng.compute_system(A, b)
    eng.synchronize()
    return A, b


# N, driver, Dirichlet faces, boundary loads, knots, segments
CASES = [
    ((9, 8, 6), "system", "all", {}, None, 0),                     # whole patches of 4 x 2 pencils: 2 x 3 of them
    ((10, 9, 7), "system", "all", {}, None, 0),                    # partial patches on both axes (9 = 2 x 4 + 1, 7 = 3 x 2 + 1)
    ((17, 5, 4), "system", "some", {(2, 1, 0): 1.5}, None, 3),     # three segments along the walk, a boundary load
    ((8, 4, 2), "matrix", "none", {}, None, 0),                    # one patch
    ((8, 5, 4), "system", "all", {(0, 1, 0): -0.5}, None, 4),      # segments of two elements
    ((12, 13, 11), "matrix", "none", {}, None, 2),
    ((11, 10, 9), "system", "yz", {}, "open", 0),                  # non-uniform open knot vectors, Dirichlet values on two faces
    ((9, 7, 5), "matrix", "none", {}, "open", 3),
    ((8, 3, 3), "system", "all", {}, None, 0),                     # patches narrower than 4 x 2 on axis 1 and on axis 2
]


def _case(N, bc, loads, knots):
    kn = [_open_nonuniform(n, 11 + i) for i, n in enumerate(N)] if knots == "open" else None
    return T.setup_case(dim=3, dof=1, p=3, N=list(N), knots=kn, bcs=_bcs(bc), loads=loads, engine=True)


@pytest.mark.parametrize("N,driver,bc,loads,knots,nseg", CASES)
def test_patch3_vs_oracle_and_reference(N, driver, bc, loads, knots, nseg, monkeypatch):
    """First-touch stores on a NaN-poisoned matrix; IGAElementFixSystem on the combined runs; boundary loads from their own launch."""
    _env(monkeypatch, 2, nseg)
    orc, eng, _ = _case(N, bc, loads, knots)
    A, b = _assemble(eng, driver)
    kn = eng.kernel_name()
    assert "gram_pencil" in kn and "p=3" in kn and "walk=0" in kn and PATCH in kn and "gram_patch" not in kn, kn
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    if b is not None:
        assert np.abs(b.get() - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    ref = T.reference(orc, 3, T.poisson(3), bcs=_bcs(bc), loads=loads, driver="system" if driver == "system" else "matrix")
    r, cc, v = A.to_coo_global()
    R, S = ref.entries(r, cc)
    T.compare_entrywise((r, cc, v), R, S, T.C_ID, ref, "patch3 K")
    if b is not None:
        bv = b.get()
        rows = np.arange(bv.size)
        R, S = ref.vector(rows)
        T.compare_entrywise((rows, bv), R, S, T.C_ID, ref, "patch3 F")


@pytest.mark.parametrize("N,driver,bc,loads,knots,nseg", [CASES[1], CASES[2], CASES[5], CASES[6]])
def test_patch3_vs_pencil_walk(N, driver, bc, loads, knots, nseg, monkeypatch):
    """Only the order of the sums differs from the pencil walk: 1e-13 of the largest entry; the Dirichlet rows (a lone diagonal: the
    element count) and the fixed entries of F (count x value) bit for bit."""
    out = {}
    for patch3 in (2, 0):
        _env(monkeypatch, patch3, nseg)
        _, eng, _ = _case(N, bc, loads, knots)
        A, b = _assemble(eng, driver)
        assert (PATCH in eng.kernel_name()) == (patch3 == 2), eng.kernel_name()
        out[patch3] = (A.host(True).copy(), b.get().copy() if b is not None else None, A.host()[0])
    (v2, b2, _), (v0, b0, rp) = out[2], out[0]
    assert np.abs(v2 - v0).max() <= 1e-13 * np.abs(v0).max()
    if b0 is not None:
        assert np.abs(b2 - b0).max() <= 1e-13 * max(np.abs(b0).max(), 1.0)
    if bc != "none":
        nnz_row = np.array([np.count_nonzero(v0[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])
        fixed = np.flatnonzero(nnz_row == 1)
        assert fixed.size > 0
        for i in fixed:
            assert np.array_equal(v2[rp[i]:rp[i + 1]], v0[rp[i]:rp[i + 1]])
        if b0 is not None:
            assert np.array_equal(b2[fixed], b0[fixed])


@pytest.mark.parametrize("driver", ["system", "matrix"])
def test_patch3_repeatable_bitwise(driver, monkeypatch):
    """The sub-phases give every window entry, F row and lifting a fixed order of adds: two assemblies -- one of them on a NaN-poisoned
    matrix, one on a zeroed one (IGX_NO_FIRST_TOUCH) -- are identical."""
    _env(monkeypatch, 2, 3)
    _, eng, _ = _case((19, 11, 9), "some" if driver == "system" else "none", {(1, 0, 0): 0.25} if driver == "system" else {}, None)
    A, b = _assemble(eng, driver, poison=False)
    assert PATCH in eng.kernel_name(), eng.kernel_name()
    vals, bv = A.host(True).copy(), (b.get().copy() if b is not None else None)
    _poison(A)
    if b is None:
        eng.compute_matrix(A)
    else:
        eng.compute_system(A, b)
    eng.synchronize()
    assert np.array_equal(A.host(True), vals)
    if b is not None:
        assert np.array_equal(b.get(), bv)
    monkeypatch.setenv("IGX_NO_FIRST_TOUCH", "1")
    _, eng2, _ = _case((19, 11, 9), "some" if driver == "system" else "none", {(1, 0, 0): 0.25} if driver == "system" else {}, None)
    A2, b2 = _assemble(eng2, driver)
    assert PATCH in eng2.kernel_name(), eng2.kernel_name()
    assert np.array_equal(A2.host(True), vals)
    if b is not None:
        assert np.array_equal(b2.get(), bv)


def test_uncovered_cases_keep_the_pencil_walk(monkeypatch):
    """IGX_PATCH3=2 and still the pencil walk: a rank of a 2-rank partition, a periodic axis 0, a fix table, an affine geometry, the
    480-MFMA Gram phase (IGX_GRAM_SUMFACT=0).  Each still agrees with the oracle."""
    import petiga_amd as P
    _env(monkeypatch, 2)
    # two ranks (the local rows before the exchange are not compared here: the pencil walk's own tests do)
    for r in range(2):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, 3, (10, 9, 16)[i])
        g.set_comm(2, r)
        g.setup()
        g.set_form("poisson")
        A, b = g.create_mat(), g.create_vec()
        g.compute_system(A, b)
        g.synchronize()
        assert "gram_pencil" in g.kernel_name() and PATCH not in g.kernel_name(), g.kernel_name()
    # periodic axis 0 (the walk takes axis 2)
    orc, eng = make_pair(3, 1, 3, [10, 8, 9], periodic=[True, False, False])
    A, _ = _assemble(eng, "matrix")
    assert "gram_pencil" in eng.kernel_name() and PATCH not in eng.kernel_name(), eng.kernel_name()
    compare_mats(A, orc.compute_system("orc_form_poisson")[0], 1e-12)
    # a fix table
    orc, eng = make_pair(3, 1, 3, [9, 8, 6])
    for g in (orc, eng):
        g.set_boundary_value(0, 0, 0, 1.0); g.set_boundary_value(2, 1, 0, 2.0)
    table = np.random.default_rng(3).standard_normal(orc.global_size())
    orc.set_fixtable(table)
    eng.set_fixtable(eng.create_vec().set(table))
    A, b = _assemble(eng, "system")
    assert "gram_pencil" in eng.kernel_name() and PATCH not in eng.kernel_name(), eng.kernel_name()
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    assert np.abs(b.get() - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    # an affine geometry
    orc, eng, _ = T.setup_case(dim=3, dof=1, p=3, N=[9, 8, 6], geometry="affine", seed=2, engine=True)
    A, _ = _assemble(eng, "matrix")
    assert "gram_pencil" in eng.kernel_name() and "mapped geometry" in eng.kernel_name() and PATCH not in eng.kernel_name(), eng.kernel_name()
    compare_mats(A, orc.compute_system("orc_form_poisson")[0], 1e-12)
    # the 480-MFMA phase
    _env(monkeypatch, 2, 0, sumfact=0)
    monkeypatch.setenv("IGX_GRAM_SUMFACT", "0")
    orc, eng = make_pair(3, 1, 3, [9, 8, 6])
    A, _ = _assemble(eng, "matrix")
    assert "gram_pencil" in eng.kernel_name() and PATCH not in eng.kernel_name(), eng.kernel_name()
    compare_mats(A, orc.compute_system("orc_form_poisson")[0], 1e-12)


def test_patch3_default_choice(monkeypatch):
    """IGX_PATCH3 unset: the launcher keeps the pencil walk below 16^3 elements (not measured there) and takes the patch walk from
    16^3 on (faster at every size measured); IGX_PATCH3=0 keeps the pencil walk everywhere."""
    import petiga_amd as P
    monkeypatch.delenv("IGX_PATCH3", raising=False)
    monkeypatch.delenv("IGX_NSEG", raising=False)
    monkeypatch.delenv("IGX_GRAM_SUMFACT", raising=False)

    def name(n):
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, 3, n)
        g.setup()
        g.set_form("poisson")
        A = g.create_mat()
        g.compute_matrix(A)
        g.synchronize()
        return g.kernel_name()
    assert PATCH not in name(8) and PATCH not in name(15)
    assert PATCH in name(16) and PATCH in name(40)
    monkeypatch.setenv("IGX_PATCH3", "0")
    assert PATCH not in name(40)
