"""gram_pencil_patch3 (petiga_amd/csrc/gram_patch3.hpp) at the shapes where keeping a pencil's open band rows in registers can go wrong
and adding every tile to the window could not (round 11: a wavefront sums the tiles of a row across its elements in registers and adds
the row's four blocks to the window once, in eight ticks; the rows slide with the walk; behind the last element of the last segment
three rows are still in registers and reach the window through the same ticks): segments shorter than their halo, a last segment of
one element, Gram sums that differ in every element, a cut where the band positions are not contiguous, wavefronts without a pencil,
and a walk that is one segment of one patch.  Every case: the patch walk is the one that ran; pattern and values against the oracle to
1e-12, every entry against the tensor-product reference within T.C_ID, F likewise for the System driver; a first-touch assembly over a
NaN-poisoned matrix and a second one bit for bit; one more with IGX_NO_FIRST_TOUCH=1 bit for bit.  Cases a and c also against the
pencil walk, at the tolerance of test_gpu_patch_p3.py::test_patch3_vs_pencil_walk."""
import numpy as np
import pytest

import tensor_ref as T
from common import compare_mats
from test_gpu_patch3_inflight import ALL_FACES, PATCH, _assemble, _case, _compute, _env, _poison

pytestmark = pytest.mark.gpu

# id, N (axis 0 is the walk axis; eight elements is the shortest the launcher gives this kernel), driver, Dirichlet faces, knots, IGX_NSEG
CASES = [
    ("a-halo-longer-than-segment", (8, 5, 4), "system", ALL_FACES, None, 4),      # segments of two elements behind a halo of three: dropped and owned rows alternate
    ("b-last-segment-of-one", (13, 5, 4), "system", ALL_FACES, None, 6),          # the tail adds rows fed almost only by the halo
    ("c-nonuniform", (11, 5, 4), "system", ALL_FACES, "open", 3),                 # every element's Gram sums differ: a wrong slide or a tile in the wrong row shows in every entry
    ("c-one-face", (11, 5, 4), "system", {(0, 1, 0): 1.25}, "open", 3),           # a value only behind the trailing layers
    ("d-cut-in-open-knots", (9, 7, 5), "matrix", {}, "open", 2),                  # a cut in the walk axis where the band positions are not contiguous
    ("e-narrow-3x3", (8, 3, 3), "system", ALL_FACES, None, 0),                    # wavefronts without a pencil in both directions
    ("f-narrow-1x2", (8, 1, 2), "system", ALL_FACES, None, 0),                    # one pencil of eight in its row
    ("g-one-patch-one-segment", (8, 4, 2), "matrix", {}, None, 0),                # the tail alone
]


def _values(A, b):
    return A.host(True).copy(), (b.get().copy() if b is not None else None)


@pytest.mark.parametrize("name,N,driver,bcs,knots,nseg", CASES, ids=[c[0] for c in CASES])
def test_patch3_rows(name, N, driver, bcs, knots, nseg, monkeypatch):
    _env(monkeypatch, nseg)
    orc, eng, _ = _case(N, bcs, knots)
    A, b = _assemble(eng, driver, poison=True)      # (asserts that the patch walk ran) first touch over NaN
    vals, bv = _values(A, b)
    assert not np.isnan(vals).any()
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    if b is not None:
        assert np.abs(bv - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    ref = T.reference(orc, 3, T.poisson(3), bcs=bcs, loads={}, driver=driver)
    r, cc, v = A.to_coo_global()
    R, S = ref.entries(r, cc)
    T.compare_entrywise((r, cc, v), R, S, T.C_ID, ref, "patch3 rows K")
    if b is not None:
        rows = np.arange(bv.size)
        R, S = ref.vector(rows)
        T.compare_entrywise((rows, bv), R, S, T.C_ID, ref, "patch3 rows F")
    # a second assembly into the same matrix, poisoned again: bit for bit
    _poison(A)
    _compute(eng, A, b)
    assert np.array_equal(A.host(True), vals)
    if b is not None:
        assert np.array_equal(b.get(), bv)
    # ... and every lane reading and adding into a zeroed matrix
    _env(monkeypatch, nseg, no_first_touch=True)
    _, eng2, _ = _case(N, bcs, knots)
    A2, b2 = _assemble(eng2, driver, poison=False)
    v2, bv2 = _values(A2, b2)
    assert not np.isnan(v2).any()
    assert np.array_equal(v2, vals)
    if b is not None:
        assert np.array_equal(bv2, bv)


@pytest.mark.parametrize("name,N,driver,bcs,knots,nseg", [CASES[0], CASES[2]], ids=[CASES[0][0], CASES[2][0]])
def test_patch3_rows_vs_pencil_walk(name, N, driver, bcs, knots, nseg, monkeypatch):
    """Only the order of the sums differs from the pencil walk: 1e-13 of the largest entry; the Dirichlet rows (a lone diagonal: the
    element count) and the fixed entries of F (count x value) bit for bit."""
    out = {}
    for patch3 in (2, 0):
        _env(monkeypatch, nseg)
        monkeypatch.setenv("IGX_PATCH3", str(patch3))
        _, eng, _ = _case(N, bcs, knots)
        eng.set_form("poisson")
        A, b = eng.create_mat(), eng.create_vec()
        _compute(eng, A, b)
        assert (PATCH in eng.kernel_name()) == (patch3 == 2), eng.kernel_name()
        out[patch3] = _values(A, b) + (A.host()[0],)
    (v2, b2, _), (v0, b0, rp) = out[2], out[0]
    assert np.abs(v2 - v0).max() <= 1e-13 * np.abs(v0).max()
    assert np.abs(b2 - b0).max() <= 1e-13 * max(np.abs(b0).max(), 1.0)
    nnz_row = np.array([np.count_nonzero(v0[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])
    fixed = np.flatnonzero(nnz_row == 1)
    assert fixed.size > 0
    for i in fixed:
        assert np.array_equal(v2[rp[i]:rp[i + 1]], v0[rp[i]:rp[i + 1]])
    assert np.array_equal(b2[fixed], b0[fixed])
