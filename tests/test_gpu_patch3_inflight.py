"""gram_pencil_patch3 (petiga_amd/csrc/gram_patch3.hpp) at the shapes where a change to the way its band rows leave and its tiles reach
the window can go wrong (round 10: the tiles are added with plain LDS reads and writes inside their sub-phases, the Gram sums of a step
are read ahead of them): a request for old values past the end of a segment (segments of two elements on the shortest walk axis the
launcher gives this kernel, eight elements -- a segment then walks five with its halo -- and a last segment of one element; a walk axis
of five elements never reaches this kernel), patches narrower than 4 x 2 whose second run has few lanes or none, a second run partly
filled, first-touch lanes over a NaN-poisoned matrix, and non-contiguous layers between contiguous ones (open non-uniform knots).
Every case: pattern and values against the oracle to 1e-12, every entry against the tensor-product reference within T.C_ID, F
likewise for the System driver, and two assemblies bit for bit -- the tolerances of test_gpu_patch_p3.py."""
import ctypes as C

import numpy as np
import pytest

import tensor_ref as T
from common import compare_mats

pytestmark = pytest.mark.gpu

PATCH = "pencils per workgroup,one window"
ALL_FACES = {(d, s, 0): 1.0 + 0.5 * d - 0.25 * s for d in range(3) for s in range(2)}


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


def _env(monkeypatch, nseg, no_first_touch=False):
    monkeypatch.setenv("IGX_PATCH3", "2")
    monkeypatch.delenv("IGX_GRAM_SUMFACT", raising=False)
    for k, v in (("IGX_NSEG", nseg), ("IGX_NO_FIRST_TOUCH", 1 if no_first_touch else 0)):
        if v:
            monkeypatch.setenv(k, str(v))
        else:
            monkeypatch.delenv(k, raising=False)


def _case(N, bcs, knots):
    kn = [_open_nonuniform(n, 11 + i) for i, n in enumerate(N)] if knots == "open" else None
    return T.setup_case(dim=3, dof=1, p=3, N=list(N), knots=kn, bcs=bcs, loads={}, engine=True)


def _compute(eng, A, b):
    if b is None:
        eng.compute_matrix(A)
    else:
        eng.compute_system(A, b)
    eng.synchronize()


def _assemble(eng, driver, poison):
    eng.set_form("poisson")
    A = eng.create_mat()
    b = eng.create_vec() if driver == "system" else None
    if poison:
        _poison(A)
    _compute(eng, A, b)
    assert PATCH in eng.kernel_name(), eng.kernel_name()
    return A, b


# id, N (axis 0 is the walk axis), driver, Dirichlet faces, knots, IGX_NSEG
CASES = [
    ("segment-end-8", (8, 5, 4), "system", ALL_FACES, None, 4),      # four segments of two elements: the request for layer L + 1 meets the end of a segment in every other step
    ("segment-end-1", (13, 5, 4), "system", ALL_FACES, None, 6),     # segments of three elements and a last one of a single element (four steps with its halo)
    ("narrow-3x2", (8, 3, 2), "system", ALL_FACES, None, 0),         # a patch narrower than 4 x 2: 30 x 23 = 690 runs, three wavefronts of run 1 without a lane
    ("narrow-2x2", (8, 2, 2), "system", ALL_FACES, None, 0),         # 23 x 23 = 529 runs: 17 lanes in run 1
    ("empty-run-1", (8, 1, 2), "system", ALL_FACES, None, 0),        # 16 x 23 = 368 runs <= 512: run 1 has no lane at all, run 0 not every lane
    ("full-patches", (9, 8, 6), "system", ALL_FACES, None, 0),       # 37 x 23 = 851 runs: run 1 partly filled
    ("first-touch", (10, 9, 7), "system", ALL_FACES, None, 3),       # three segments, partial patches: first-touch and read-add lanes side by side
    ("open-knots", (9, 7, 5), "matrix", {}, "open", 0),              # non-contiguous layers at both ends of the walk axis next to contiguous ones
]


@pytest.mark.parametrize("name,N,driver,bcs,knots,nseg", CASES, ids=[c[0] for c in CASES])
def test_patch3_inflight(name, N, driver, bcs, knots, nseg, monkeypatch):
    _env(monkeypatch, nseg)
    orc, eng, _ = _case(N, bcs, knots)
    A, b = _assemble(eng, driver, poison=True)      # first touch over NaN: a lane that consumed what it loaded shows up everywhere below
    vals, bv = A.host(True).copy(), (b.get().copy() if b is not None else None)
    assert not np.isnan(vals).any()
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    if b is not None:
        assert np.abs(bv - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    ref = T.reference(orc, 3, T.poisson(3), bcs=bcs, loads={}, driver=driver)
    r, cc, v = A.to_coo_global()
    R, S = ref.entries(r, cc)
    T.compare_entrywise((r, cc, v), R, S, T.C_ID, ref, "patch3 K")
    if b is not None:
        rows = np.arange(bv.size)
        R, S = ref.vector(rows)
        T.compare_entrywise((rows, bv), R, S, T.C_ID, ref, "patch3 F")
    # a second assembly into the same matrix, poisoned again: bit for bit
    _poison(A)
    _compute(eng, A, b)
    assert np.array_equal(A.host(True), vals)
    if b is not None:
        assert np.array_equal(b.get(), bv)
    if name == "first-touch":      # ... and every lane reading and adding into a zeroed matrix
        _env(monkeypatch, nseg, no_first_touch=True)
        _, eng2, _ = _case(N, bcs, knots)
        A2, b2 = _assemble(eng2, driver, poison=False)
        v2 = A2.host(True)
        assert not np.isnan(v2).any()
        assert np.array_equal(v2, vals)
        assert np.array_equal(b2.get(), bv)
