"""IGXTransfer in the C ABI (include/petiga_amd.h) and its Python view, on a machine without a GPU: the calls are declared, exported and bound
with matching argument lists; every refusal that is decided before any HIP call comes with its code, a reason that names the transfer, and in
the order the header states (each case below breaks two rules at once and the earlier one must answer); IGXTransferGetAxis against
tests/transfer_ref.py entry by entry.  IGXTransferCreate and IGXTransferGetAxis touch no device.

Not reached here: the vector refusals of Prolong / Restrict past the null vector (a vector needs IGXCreateVec, which allocates on the device:
tests/test_gpu_transfer.py::test_refusals_with_vectors), and a degree above 7 (IGXAxisSetDegree refuses it with IGX_ERR_SUP, so no set-up
space holds one; IGXTransferCreate repeats the check under its own name for a route added later).

c_T of the GetAxis check.  The engine builds a row by p levels of D' = (1 - w) D_left + w D_right with w = (x - u_j) / (u_k - u_j) in double.
All of w, 1 - w and the entries lie in [0, 1].  Per level: w carries 3 roundings (two differences, a quotient: |dw| <= 3 u), 1 - w one more
(4 u), the two products and the sum one each (3 u), and a convex combination does not amplify the error its inputs carry.  That is at most
(3 + 4 + 3) u = 10 u of absolute error per level and c_T = 10 p for the whole row; the long double reference's own error is 2^-11 of that.
Entries the reference has as exact zeros (outside the band) must be exact zeros."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import transfer_ref as TR
from test_transfer_reference import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
CALLS = {"IGXTransferCreate": 3, "IGXTransferGetAxis": 8, "IGXTransferProlong": 4, "IGXTransferRestrict": 3, "IGXTransferDestroy": 1}      # the contract's five
EXTRA = {"IGXTransferSetPath": 2, "IGXTransferGetInfo": 4}                                                                                  # beyond it
ARG_WRONG, OUTOFRANGE, ORDER, SUP = 62, 63, 58, 56


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+_p_IGXTransfer\s*\*\s*IGXTransfer\s*;", text)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}
    L, V = P.lib(), C.c_void_p
    for name, nargs in {**CALLS, **EXTRA}.items():
        assert name in decl, "%s is not declared in include/petiga_amd.h" % name
        assert len([a for a in decl[name].split(",") if a.strip()]) == nargs, (name, decl[name])
        f = getattr(L, name)                            # AttributeError: the library does not export it
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    assert L.IGXTransferCreate.argtypes == [V, V, C.POINTER(V)]
    assert L.IGXTransferGetAxis.argtypes == [V, C.c_int, ip, ip, ip, ip, ip, dp]
    assert L.IGXTransferProlong.argtypes == [V, V, V, C.c_int] and L.IGXTransferRestrict.argtypes == [V, V, V]
    assert L.IGXTransferDestroy.argtypes == [C.POINTER(V)]
    assert callable(P.IGX.transfer) and all(hasattr(P.Transfer, a) for a in ("prolong", "restrict", "axis", "close"))


def _space(axes, dof=1, setup=True, comm=None):
    """axes: (p, U, periodic) per axis"""
    import petiga_amd as P
    g = P.IGX(len(axes), dof)
    for i, (p, U, periodic) in enumerate(axes):
        g.axis_knots(i, p, U, periodic=periodic)
    if comm:
        g.set_comm(*comm)
    if setup:
        g.setup()
    return g


def _create(c, f):
    import petiga_amd as P
    h = C.c_void_p()
    rc = P.lib().IGXTransferCreate(c.h if c is not None else None, f.h if f is not None else None, C.byref(h))
    return rc, P.lib().IGXGetLastError().decode(), h


def _ax(p, N, periodic=False):
    return (p, TR.uniform_knots(p, N, periodic=periodic), periodic)


def test_refusals_in_the_pinned_order():
    import petiga_amd as P
    L = P.lib()
    why = lambda: L.IGXGetLastError().decode()
    c, f = _space([_ax(2, 3), _ax(3, 2)]), _space([_ax(2, 6), _ax(3, 4)])
    rc, msg, h = _create(c, f)
    assert rc == 0 and h.value, (rc, msg)
    # 1. null pointers
    for args in ((None, f), (c, None)):
        rc, msg, _ = _create(*args)
        assert rc == ARG_WRONG and "transfer" in msg and "null" in msg, (rc, msg)
    assert L.IGXTransferCreate(c.h, f.h, None) == ARG_WRONG and "transfer" in why()
    # 2. before IGXSetUp (and another dim): the order comes first
    rc, msg, _ = _create(_space([_ax(2, 3)], setup=False), f)
    assert rc == ORDER and "IGXSetUp" in msg and "transfer" in msg, (rc, msg)
    rc, msg, _ = _create(c, _space([_ax(2, 6), _ax(3, 4)], setup=False))
    assert rc == ORDER, (rc, msg)
    # 3. dim before dof before degree before periodicity before the streams
    rc, msg, _ = _create(_space([_ax(2, 3)], dof=2), f)
    assert rc == ARG_WRONG and "transfer" in msg and "dim" in msg, (rc, msg)
    rc, msg, _ = _create(_space([_ax(3, 3), _ax(3, 2)], dof=2), f)
    assert rc == ARG_WRONG and "transfer" in msg and "dof" in msg, (rc, msg)
    rc, msg, _ = _create(_space([_ax(3, 3), _ax(3, 4, True)]), f)
    assert rc == ARG_WRONG and "degree" in msg and "axis 0" in msg and "elevation" in msg, (rc, msg)
    cs = _space([_ax(2, 3), _ax(3, 4, True)])
    cs.set_stream(0x40)                                   # never used: nothing here reaches the device
    rc, msg, _ = _create(cs, f)
    assert rc == ARG_WRONG and "periodicity" in msg and "axis 1" in msg, (rc, msg)
    # 4. the streams before the ranks
    cs = _space([_ax(2, 3), _ax(3, 2)], comm=(2, 0))
    cs.set_stream(0x40)
    rc, msg, _ = _create(cs, f)
    assert rc == ARG_WRONG and "stream" in msg and "transfer" in msg, (rc, msg)
    # 5. the ranks before nestedness, in the solvers' sentence; an axis that is neither clamped nor periodic
    rc, msg, _ = _create(_space([_ax(2, 5), _ax(3, 2)], comm=(2, 0)), f)
    assert rc == SUP and "the transfer needs one rank on every axis" in msg, (rc, msg)
    rc, msg, _ = _create(c, _space([_ax(2, 6), _ax(3, 4)], comm=(2, 1)))
    assert rc == SUP and "one rank" in msg, (rc, msg)
    open_axis = (1, np.arange(6.0), False)
    rc, msg, _ = _create(_space([open_axis]), _space([open_axis]))
    assert rc == SUP and "transfer" in msg and "clamped" in msg and "axis 0" in msg, (rc, msg)
    # 6. not nested: the axis and the knot
    rc, msg, _ = _create(_space([_ax(2, 3), _ax(3, 2)]), _space([_ax(2, 6), _ax(3, 3)]))
    assert rc == OUTOFRANGE and "transfer" in msg and "not nested" in msg and "axis 1" in msg and "0.5" in msg and "missing" in msg, (rc, msg)
    U2 = np.array([0, 0, 0, 0.5, 0.5, 1, 1, 1.0])
    rc, msg, _ = _create(_space([(2, U2, False)]), _space([(2, TR.uniform_knots(2, 4), False)]))
    assert rc == OUTOFRANGE and "axis 0" in msg and "0.5" in msg and "multiplicity 2" in msg, (rc, msg)
    rc, msg, _ = _create(_space([(2, TR.uniform_knots(2, 3, a=0.0, b=2.0), False)]), _space([_ax(2, 6)]))
    assert rc == OUTOFRANGE and "end knots differ" in msg and "axis 0" in msg, (rc, msg)
    rc, msg, _ = _create(_space([_ax(2, 5, True)]), _space([_ax(2, 8, True)]))
    assert rc == OUTOFRANGE and "not nested" in msg, (rc, msg)
    # the calls on a transfer: null, then stale, then the arguments
    assert L.IGXTransferProlong(None, None, None, 0) == ARG_WRONG and "transfer" in why()
    assert L.IGXTransferRestrict(None, None, None) == ARG_WRONG and L.IGXTransferGetAxis(None, 0, None, None, None, None, None, None) == ARG_WRONG
    assert L.IGXTransferSetPath(None, 0) == ARG_WRONG and L.IGXTransferGetInfo(None, None, None, None) == ARG_WRONG
    assert L.IGXTransferProlong(h, None, None, 0) == ARG_WRONG and "transfer" in why() and "null vector" in why()
    assert L.IGXTransferRestrict(h, None, None) == ARG_WRONG and "null vector" in why()
    for axis in (-1, 3):
        assert L.IGXTransferGetAxis(h, axis, None, None, None, None, None, None) == OUTOFRANGE and "transfer" in why()
    assert L.IGXTransferSetPath(h, 3) == OUTOFRANGE and L.IGXTransferSetPath(h, 2) == 0 and L.IGXTransferSetPath(h, 0) == 0
    nf, nc, w = C.c_int(), C.c_int(), C.c_int()
    assert L.IGXTransferGetAxis(h, 2, C.byref(nf), C.byref(nc), C.byref(w), None, None, None) == 0 and (nf.value, nc.value, w.value) == (1, 1, 1)
    # stale after IGXSetUp on either IGX: every call, before its other checks
    for which in (c, f):
        rc, msg, h2 = _create(c, f)
        assert rc == 0
        which.setup()
        for rc in (L.IGXTransferProlong(h2, None, None, 0), L.IGXTransferRestrict(h2, None, None), L.IGXTransferGetAxis(h2, 7, None, None, None, None, None, None),
                   L.IGXTransferSetPath(h2, 9), L.IGXTransferGetInfo(h2, None, None, None)):
            assert rc == ORDER
        assert "stale" in why() and "transfer" in why() and "IGXSetUp" in why()
        assert L.IGXTransferDestroy(C.byref(h2)) == 0 and not h2.value
    assert L.IGXTransferProlong(h, None, None, 0) == ORDER      # (made before both set-ups)
    assert L.IGXTransferDestroy(C.byref(h)) == 0 and not h.value and L.IGXTransferDestroy(C.byref(h)) == 0 and L.IGXTransferDestroy(None) == 0
    # the Python view
    with pytest.raises(P.IGXError) as e:
        _space([_ax(2, 6)]).transfer(_space([_ax(2, 4)]))
    assert e.value.code == OUTOFRANGE and "transfer" in str(e.value)
    t = f.transfer(c)
    assert t.sizes(0) == (8, 5, 3) and t.sizes(1) == (7, 5, 4) and t.info()["box"] == (8, 7, 1)
    t.close()
    t.close()


@pytest.mark.parametrize("name,p,Uc,Uf,periodic", CASES, ids=[c[0] for c in CASES])
def test_get_axis_against_the_reference(name, p, Uc, Uf, periodic):
    c, f = _space([(p, Uc, periodic)]), _space([(p, Uf, periodic)])
    t = f.transfer(c)
    nf, nc, w = t.sizes(0)
    first, count, band = t.axis(0)
    R = TR.matrix_rowwise(p, Uc, Uf, periodic)
    assert (nf, nc) == R.shape and w == p + 1
    assert np.all(count >= 1) and np.all(count <= w) and np.all(first >= 0) and np.all(first < nc)
    for i in range(nf):
        assert np.all(band[i, count[i]:] == 0) and band[i, 0] != 0 and band[i, count[i] - 1] != 0      # zero past count, the band trimmed
    E = TR.dense(first, count, band, nc)
    c_T = 10 * p
    err = np.abs(E - R)
    assert not np.any(err[R == 0] != 0), "%s: an entry outside the reference's band is not an exact zero" % name
    worst = float(err.max() / TR.U_RND)
    print("%s: %d x %d, worst |E - R| = %.2f u (c_T = %d)" % (name, nf, nc, worst, c_T))
    assert worst <= c_T
    assert np.all(band >= 0) and np.max(np.abs(band.sum(axis=1) - 1)) <= 2 * (p + 1) * TR.U_RND
    if nc > p + 1:                                       # the first column: non-decreasing, by at most one per row (cyclically on a periodic axis)
        step = np.diff(first.astype(np.int64)) % nc if periodic else np.diff(first.astype(np.int64))
        assert np.all((step == 0) | (step == 1))
    if not periodic:
        assert (first[0], count[0], band[0, 0]) == (0, 1, 1.0) and (first[-1], count[-1], band[-1, 0]) == (nc - 1, 1, 1.0)
    if name.endswith("-same"):
        assert np.array_equal(first, np.arange(nc)) and np.all(count == 1) and np.all(band[:, 0] == 1.0)
    t.close()
