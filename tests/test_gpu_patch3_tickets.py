"""gram_pencil_patch3 (petiga_amd/csrc/gram_patch3.hpp) with resident workgroups that take their (segment, patch) items from a counter
by ticket (round 12), at the shapes where what one item leaves behind can reach the next: one workgroup that walks every item of every
colour (consecutive items differ in the patch's width on both axes, face against interior, segment, and end on a last segment of one
element behind its halo), grids that end on different tickets, more workgroups than items, Gram sums that differ in every element,
wavefronts without a pencil in one item and others idle in the next, the counter across repeated assemblies and across two engines.
The yardstick of every case is IGX_PATCH3_PERSIST=0, the launch of one workgroup per item: bit for bit, A and b.  Every case asserts that
the patch walk ran and assembles by first touch over a NaN-poisoned matrix.

(N = (13, 9, 7) with IGX_NSEG=6 walks five segments -- 3, 3, 3, 3 and 1 elements -- so its colours hold 20, 10, 10, 5, 10 and 5 items: a
grid of 5 does divide them, unlike what this round's issue says of it; which workgroup ends on which ticket is decided by the
run either way.)"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import tensor_ref as T
from common import compare_mats
from test_gpu_patch3_inflight import ALL_FACES, _assemble, _case, _compute, _poison

pytestmark = pytest.mark.gpu

N1, NSEG1 = (13, 9, 7), 6
SWITCHES = ("IGX_PATCH3", "IGX_GRAM_SUMFACT", "IGX_NSEG", "IGX_NO_FIRST_TOUCH", "IGX_PATCH3_PERSIST", "IGX_PATCH3_GRID", "IGX_PATCH3_ORDER")


@contextmanager
def _switches(nseg, persist, grid=None, no_first_touch=False, order=None):
    """The environment an engine is created under (the switches are read then)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    new = {"IGX_PATCH3": "2", "IGX_NSEG": str(nseg) if nseg else None, "IGX_NO_FIRST_TOUCH": "1" if no_first_touch else None,
           "IGX_PATCH3_PERSIST": str(persist), "IGX_PATCH3_GRID": None if grid is None else str(grid), "IGX_PATCH3_ORDER": None if order is None else str(order)}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if new.get(k) is not None:
                os.environ[k] = new[k]
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _values(A, b):
    return A.host(True).copy(), (b.get().copy() if b is not None else None)


def _run(N, driver, bcs, knots, nseg, persist, grid=None, no_first_touch=False, keep=False, order=None):
    with _switches(nseg, persist, grid, no_first_touch, order):
        orc, eng, _ = _case(N, bcs, knots)
    A, b = _assemble(eng, driver, poison=True)      # asserts that the patch walk ran
    vals, bv = _values(A, b)
    assert not np.isnan(vals).any()
    assert bv is None or not np.isnan(bv).any()
    return (vals, bv, orc, eng, A, b) if keep else (vals, bv)


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    if want[1] is not None:
        assert np.array_equal(got[1], want[1])


_BASE = {}


def _base1():
    """Case 1's shape with one workgroup per item: computed once, shared by the cases that must equal it."""
    if "v" not in _BASE:
        _BASE["v"] = _run(N1, "system", ALL_FACES, None, NSEG1, persist=0)
    return _BASE["v"]


def test_one_workgroup_walks_everything():
    want = _base1()
    vals, bv, orc, eng, A, b = _run(N1, "system", ALL_FACES, None, NSEG1, persist=1, grid=1, keep=True)
    _same((vals, bv), want)
    A_o, b_o = orc.compute_system("orc_form_poisson")
    compare_mats(A, A_o, 1e-12)
    assert np.abs(bv - b_o).max() <= 1e-12 * max(np.abs(b_o).max(), 1.0)
    ref = T.reference(orc, 3, T.poisson(3), bcs=ALL_FACES, loads={}, driver="system")
    r, cc, v = A.to_coo_global()
    R, S = ref.entries(r, cc)
    T.compare_entrywise((r, cc, v), R, S, T.C_ID, ref, "patch3 tickets K")
    rows = np.arange(bv.size)
    R, S = ref.vector(rows)
    T.compare_entrywise((rows, bv), R, S, T.C_ID, ref, "patch3 tickets F")


@pytest.mark.parametrize("grid", [2, 5, 0])
def test_grids_end_on_different_tickets(grid):
    _same(_run(N1, "system", ALL_FACES, None, NSEG1, persist=1, grid=grid), _base1())


def test_natural_order_of_tickets():
    _same(_run(N1, "system", ALL_FACES, None, NSEG1, persist=1, grid=2, order=0), _base1())


def test_more_workgroups_than_items():
    want = _run((8, 4, 2), "matrix", {}, None, 0, persist=0)
    _same(_run((8, 4, 2), "matrix", {}, None, 0, persist=1, grid=64), want)


def test_nonuniform_open_knots():
    bcs = {(0, 1, 0): 1.25}
    want = _run((11, 5, 4), "system", bcs, "open", 3, persist=0)
    _same(_run((11, 5, 4), "system", bcs, "open", 3, persist=1, grid=1), want)


def test_wavefronts_without_a_pencil():
    want = _run((8, 3, 3), "system", ALL_FACES, None, 0, persist=0)
    _same(_run((8, 3, 3), "system", ALL_FACES, None, 0, persist=1, grid=1), want)


def test_counter_across_assemblies():
    """A ticket left over from an earlier assembly would skip items: NaN stays where they were to be stored."""
    vals, bv, _, eng, A, b = _run(N1, "system", ALL_FACES, None, NSEG1, persist=1, grid=2, keep=True)
    _same((vals, bv), _base1())
    for _ in range(2):
        _poison(A)
        _compute(eng, A, b)
        got = _values(A, b)
        assert not np.isnan(got[0]).any()
        _same(got, (vals, bv))


def test_counter_across_engines():
    first = {}
    engines = {}
    for key, N, bcs in (("A", N1, ALL_FACES), ("B", (8, 3, 3), ALL_FACES)):
        vals, bv, _, eng, A, b = _run(N, "system", bcs, None, NSEG1 if key == "A" else 0, persist=1, grid=2, keep=True)
        first[key] = (vals, bv)
        engines[key] = (eng, A, b)
    _same(first["A"], _base1())
    for key in ("A", "B", "A"):
        eng, A, b = engines[key]
        _poison(A)
        _compute(eng, A, b)
        got = _values(A, b)
        assert not np.isnan(got[0]).any()
        _same(got, first[key])


def test_no_first_touch_with_one_workgroup():
    _same(_run(N1, "system", ALL_FACES, None, NSEG1, persist=1, grid=1, no_first_touch=True), _base1())
