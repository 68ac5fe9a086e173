"""The rows walk's staged stores (petiga_amd/csrc/gram_rows3.hpp, IGX_ROWS3_STAGE): on a full layer (seven band positions on axis 0) of a
regular tile (3 x 3 node columns at least three nodes from both ends of axes 1 and 2) the nine finished rows are staged in LDS in memory
order and stored as contiguous spans by all eight wavefronts; every other layer and tile keeps the per-run stores.
Every case runs under IGX_ROWS3=2 IGX_ROWS3_STAGE=2, asserts that the staged path ran (the kernel's name says that the launch staged --
it does where the mesh has a regular tile and a full layer -- and the shape has the tile-layers the case is about), does all that
test_gpu_rows3._check does -- a NaN-poisoned matrix with no NaN left, the pattern exact and the values against the oracle to 1e-12, every entry against the tensor-product reference within T.C_ID, a second assembly bit for bit,
the patch walk within 1e-13 with fixed rows bit for bit -- and then holds A and b bit for bit against an engine created under
IGX_ROWS3_STAGE=0: the same adder forms every entry, only its way to memory differs.
The shapes (elements per axis, axis 0 first; nodes are elements + 3) are the smallest at which each thing can go wrong: a regular tile needs
six elements on axes 1 and 2, a full layer four on axis 0 -- and the walk, like the patch walk it is compared with, eight on axis 0
(axis_walkable): below that neither runs, so the two smallest cases are (8, 6, 6) with full layers 3 to 7, and one staged layer alone in
an item is the segments-of-1 case."""
import numpy as np
import pytest

import test_gpu_rows3 as R
from test_gpu_patch3_inflight import ALL_FACES

pytestmark = pytest.mark.gpu

STAGED = "full rows staged in LDS"


def _staged_tile_layers(N):
    """Tile-layers of the mesh that are staged: regular tiles x full layers."""
    def regular(nel):
        nn = nel + 3
        return sum(1 for a0 in range(0, nn, 3) if a0 >= 3 and a0 + 2 <= nn - 4)
    return max(0, N[0] + 3 - 6) * regular(N[1]) * regular(N[2])


def _staged_walk(monkeypatch, stage):
    """test_gpu_rows3's engines are created under IGX_ROWS3_STAGE=stage, and each rows walk says in its name which stores it made."""
    monkeypatch.setenv("IGX_ROWS3_STAGE", str(stage))
    if getattr(R._rows_walk, "_plain", None) is None:
        plain = R._rows_walk

        def walk(*a, **k):
            import os
            out = plain(*a, **k)
            # (a launch stages only where the mesh has a regular tile and a full layer: with none its name says it did not)
            assert (STAGED in out[1].kernel_name()) == (os.environ["IGX_ROWS3_STAGE"] == "2" and _staged_tile_layers(a[0]) > 0), out[1].kernel_name()
            return out
        walk._plain = plain
        monkeypatch.setattr(R, "_rows_walk", walk)


def _check(monkeypatch, N, driver, bcs, knots=None, loads=None, nseg=None, grid=None, tile_layers=None):
    assert (_staged_tile_layers(N) > 0) if tile_layers is None else (_staged_tile_layers(N) == tile_layers)
    _staged_walk(monkeypatch, 2)
    vals, bv = R._check(N, driver, bcs, knots, loads, nseg, grid)
    _staged_walk(monkeypatch, 0)
    v0, b0 = R._rows_walk(N, driver, bcs, knots, loads or {}, nseg, grid)[4:]
    assert np.array_equal(vals, v0)
    assert (bv is None and b0 is None) or np.array_equal(bv, b0)
    return vals, bv


# id, N (axis 0 first), driver, Dirichlet faces, knots, boundary loads, IGX_NSEG, staged tile-layers (None: some)
CASES = [
    ("staged-layers-matrix", (8, 6, 6), "matrix", {}, None, None, None, 5),              # layers 3-7 of the centre tile, per-entry rows all around; SYSTEM = false
    ("fix-up-in-staged-layers", (8, 6, 6), "system", ALL_FACES, None, None, None, 5),    # layers 3-7: both buffers; 3 and 7 within reach of the fixed layers
    ("several-tiles", (10, 12, 12), "system", ALL_FACES, None, None, None, 7 * 9),       # 3 x 3 adjacent staged tiles bordered by unstaged ones
    ("segments-of-2", (13, 6, 6), "system", ALL_FACES, None, None, 8, 10),               # a staged layer as an item's first and last
    ("segments-of-1", (13, 6, 6), "system", ALL_FACES, None, None, 16, 10),              # ... and only layer: the buffers start over in every item
    ("boundary-loads", (17, 6, 6), "system", R.THREE_FACES, None, {(2, 1, 0): 1.5}, 3, 14),      # F added on top of the loads
    ("open-knots", (11, 10, 9), "system", R.FACES_12, "open", None, None, None),         # every element's tables differ; axis 0 has no fixed face
    ("nothing-to-stage", (8, 5, 4), "system", ALL_FACES, None, None, None, 0),           # no regular tile: the walk runs and equals the unstaged one
]


@pytest.mark.parametrize("name,N,driver,bcs,knots,loads,nseg,tile_layers", CASES, ids=[c[0] for c in CASES])
def test_rows3_staged(monkeypatch, name, N, driver, bcs, knots, loads, nseg, tile_layers):
    _check(monkeypatch, N, driver, bcs, knots, loads, nseg, tile_layers=tile_layers)


_BASE = {}


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_rows3_staged_one_workgroup_walks_many_items(monkeypatch, grid):
    """50 items (25 tiles in two segments, nine of them regular) taken by ticket by one, two and three workgroups: a workgroup uses the
    buffers again in its next item.  Everything the other cases check, and bit for bit what one workgroup per item leaves."""
    N = (10, 12, 12)
    vals, bv = _check(monkeypatch, N, "system", ALL_FACES, nseg=2, grid=grid)
    if "v" not in _BASE:
        _staged_walk(monkeypatch, 2)
        _BASE["v"] = R._rows_walk(N, "system", ALL_FACES, None, {}, nseg=2)[4:]
    assert np.array_equal(vals, _BASE["v"][0]) and np.array_equal(bv, _BASE["v"][1])
