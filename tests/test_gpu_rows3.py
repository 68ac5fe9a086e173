"""gram_pencil_rows3 (petiga_amd/csrc/gram_rows3.hpp): the p = 3 Gram matrix gathered by rows -- a row's owner adds the contributions of
the elements that hold its node and stores the finished row once, reading nothing.  Every case runs under IGX_ROWS3=2, asserts that the
rows walk is what ran, and checks:
  * a first assembly over a NaN-poisoned matrix leaves no NaN (every entry is stored);
  * the pattern exactly and the values against the oracle to 1e-12;
  * every entry against the tensor-product reference within T.C_ID, F likewise for the System driver;
  * a second assembly over the matrix poisoned again, bit for bit;
  * against the patch walk (IGX_PATCH3=2, IGX_ROWS3=0): 1e-13 of the largest entry, the tolerance between two walks
    (test_patch3_rows_vs_pencil_walk), and the rows and F entries of fixed nodes bit for bit.
The shapes (axis 0 first) are the smallest at which each thing can go wrong: the smallest mesh; every row within three layers of a
fixed face; axes without a full row and tiles narrower than three node columns; several tiles with partial ones on both axes; three
segments with F added on top of boundary loads; tables that differ in every element; segments of two layers and of one; one
workgroup walking many items by ticket."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import tensor_ref as T
from common import compare_mats
from test_gpu_patch3_inflight import ALL_FACES, _assemble, _compute, _open_nonuniform, _poison

pytestmark = pytest.mark.gpu

ROWS = "rows gathered by their owner,each entry stored once"
SWITCHES = ("IGX_PATCH3", "IGX_ROWS3", "IGX_ROWS3_GRID", "IGX_GRAM_SUMFACT", "IGX_NSEG", "IGX_NO_FIRST_TOUCH", "IGX_PATCH3_PERSIST", "IGX_PATCH3_GRID", "IGX_PATCH3_ORDER")


@contextmanager
def _switches(**new):
    """The environment an engine is created under (the switches are read then)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if new.get(k) is not None:
                os.environ[k] = str(new[k])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _case(N, bcs, knots, loads):
    kn = [_open_nonuniform(n, 11 + i) for i, n in enumerate(N)] if knots == "open" else None
    return T.setup_case(dim=3, dof=1, p=3, N=list(N), knots=kn, bcs=bcs, loads=loads, engine=True)


def _rows_walk(N, driver, bcs, knots, loads, nseg=None, grid=None):
    """(orc, eng, A, b, values, F) of a first assembly by the rows walk over a NaN-poisoned matrix."""
    with _switches(IGX_ROWS3=2, IGX_NSEG=nseg, IGX_ROWS3_GRID=grid):
        orc, eng, _ = _case(N, bcs, knots, loads)
    eng.set_form("poisson")
    A = eng.create_mat()
    b = eng.create_vec() if driver == "system" else None
    _poison(A)
    _compute(eng, A, b)
    assert ROWS in eng.kernel_name(), eng.kernel_name()
    assert eng.dominant_kernel()["name"].startswith("gram_pencil<") and eng.dominant_kernel()["launches"] == 1
    vals, bv = A.host(True).copy(), (b.get().copy() if b is not None else None)
    assert not np.isnan(vals).any()
    assert bv is None or not np.isnan(bv).any()
    return orc, eng, A, b, vals, bv


def _fixed_rows(N, bcs):
    n = [m + 3 for m in N]
    idx = np.arange(n[0] * n[1] * n[2])
    i = (idx % n[0], (idx // n[0]) % n[1], idx // (n[0] * n[1]))
    fixed = np.zeros(idx.size, dtype=bool)
    for (d, s, _f) in bcs:
        fixed |= i[d] == (0 if s == 0 else n[d] - 1)
    return fixed


def _check(N, driver, bcs, knots=None, loads=None, nseg=None, grid=None):
    loads = loads or {}
    orc, eng, A, b, vals, bv = _rows_walk(N, driver, bcs, knots, loads, nseg, grid)
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    if b is not None:
        assert np.abs(bv - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    ref = T.reference(orc, 3, T.poisson(3), bcs=bcs, loads=loads, driver=driver)
    r, cc, v = A.to_coo_global()
    R, S = ref.entries(r, cc)
    T.compare_entrywise((r, cc, v), R, S, T.C_ID, ref, "rows3 K")
    if b is not None:
        rows = np.arange(bv.size)
        R, S = ref.vector(rows)
        T.compare_entrywise((rows, bv), R, S, T.C_ID, ref, "rows3 F")
    # a second assembly into the same matrix, poisoned again: bit for bit
    _poison(A)
    _compute(eng, A, b)
    assert np.array_equal(A.host(True), vals)
    if b is not None:
        assert np.array_equal(b.get(), bv)
    # the patch walk
    with _switches(IGX_PATCH3=2, IGX_ROWS3=0):
        _, eng2, _ = _case(N, bcs, knots, loads)
    A2, b2 = _assemble(eng2, driver, poison=True)      # asserts that the patch walk ran
    v2 = A2.host(True)
    rp = np.asarray(A.host()[0])
    assert np.array_equal(rp, np.asarray(A2.host()[0]))
    print("rows walk against the patch walk: K %.3e of the largest entry" % (np.abs(vals - v2).max() / np.abs(v2).max()))
    assert np.abs(vals - v2).max() <= 1e-13 * np.abs(v2).max()
    fixed = _fixed_rows(N, bcs) if driver == "system" else np.zeros(rp.size - 1, dtype=bool)
    in_fixed = np.repeat(fixed, np.diff(rp))
    assert np.array_equal(vals[in_fixed], v2[in_fixed])
    if b is not None:
        bv2 = b2.get()
        print("                                    F %.3e of the largest entry" % (np.abs(bv - bv2).max() / np.abs(bv2).max()))
        assert np.abs(bv - bv2).max() <= 1e-13 * np.abs(bv2).max()
        assert np.array_equal(bv[fixed], bv2[fixed])
    return vals, bv


THREE_FACES = {(0, 0, 0): 0.5, (1, 1, 0): -1.0, (2, 0, 0): 2.0}
FACES_12 = {(d, s, 0): 1.0 + 0.5 * d - 0.25 * s for d in (1, 2) for s in range(2)}

# id, N (axis 0 first), driver, Dirichlet faces, knots, boundary loads, IGX_NSEG
CASES = [
    ("smallest", (8, 4, 2), "matrix", {}, None, None, None),
    ("all-near-a-face", (8, 5, 4), "system", ALL_FACES, None, None, None),               # every row within three layers of a fixed face: lifting everywhere
    ("no-full-row-1", (8, 1, 2), "system", ALL_FACES, None, None, None),                 # axes of 4 and 5 nodes: the per-entry path only, narrow tiles
    ("no-full-row-3", (8, 3, 3), "system", ALL_FACES, None, None, None),                 # axes of 6 nodes
    ("several-tiles", (10, 9, 7), "system", ALL_FACES, None, None, None),                # 4 x 4 tiles, the last of axis 2 one column wide, interior full rows
    ("three-segments-loads", (17, 5, 4), "system", THREE_FACES, None, {(2, 1, 0): 1.5}, 3),      # F added on top of the boundary loads
    ("open-knots", (11, 10, 9), "system", FACES_12, "open", None, None),                 # every element's tables differ
    ("segments-of-2", (13, 5, 4), "system", ALL_FACES, None, None, 8),                   # 16 node layers in eight segments
    ("segments-of-1", (13, 5, 4), "system", ALL_FACES, None, None, 16),                  # ... and in sixteen
]


@pytest.mark.parametrize("name,N,driver,bcs,knots,loads,nseg", CASES, ids=[c[0] for c in CASES])
def test_rows3(name, N, driver, bcs, knots, loads, nseg):
    _check(N, driver, bcs, knots, loads, nseg)


_BASE = {}


def _base():
    """(10, 9, 7) with one workgroup per item: computed once, shared by the grids that must equal it."""
    if "v" not in _BASE:
        _BASE["v"] = _rows_walk((10, 9, 7), "system", ALL_FACES, None, {}, nseg=2)[4:]
    return _BASE["v"]


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_rows3_one_workgroup_walks_many_items(grid):
    """32 items (16 tiles in two segments) taken by ticket by one, two and three workgroups: everything the other cases check, and bit
    for bit what one workgroup per item leaves."""
    vals, bv = _check((10, 9, 7), "system", ALL_FACES, nseg=2, grid=grid)
    want = _base()
    assert np.array_equal(vals, want[0]) and np.array_equal(bv, want[1])


def test_rows3_choice(monkeypatch):
    """IGX_PATCH3 keeps its meaning and wins: 2 forces the patch walk, 0 the pencil walk, whatever IGX_ROWS3 says; IGX_ROWS3=0 never takes
    the rows walk; unset, small meshes keep the patch walk (test_patch3_default_choice pins 16^3 and 40^3)."""
    import petiga_amd as P

    def name(n, **env):
        with _switches(**env):
            g = P.IGX(3, 1)
            for i in range(3):
                g.axis_uniform(i, 3, n)
            g.setup()
        g.set_form("poisson")
        A = g.create_mat()
        g.compute_matrix(A)
        g.synchronize()
        return g.kernel_name()
    assert ROWS in name(8, IGX_ROWS3=2)
    assert ROWS not in name(8, IGX_ROWS3=2, IGX_PATCH3=2) and "one window" in name(8, IGX_ROWS3=2, IGX_PATCH3=2)
    assert ROWS not in name(8, IGX_ROWS3=2, IGX_PATCH3=0) and "pencil" in name(8, IGX_ROWS3=2, IGX_PATCH3=0)
    assert ROWS not in name(16, IGX_ROWS3=0) and ROWS not in name(16) and ROWS not in name(40)
