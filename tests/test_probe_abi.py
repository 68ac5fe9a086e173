"""IGXProbe in the C ABI (include/petiga_amd.h) and its Python view: the five calls are declared, exported and bound with matching
argument lists, and every refusal that is decided before any HIP call comes with its code and a reason that names the probe -- on a
machine without a GPU (a probe of no points touches no device, so the refusals of the calls on a probe are reached too).
Two refusals of IGXProbeEvaluate are not reached here.  A vector of another IGX needs a vector, and IGXCreateVec allocates on the device: it
is checked on the GPU (tests/test_gpu_probe_points.py::test_edges).  A vector of the probe's own IGX with another size exists only after
another IGXSetUp, and then the probe is stale and IGX_ERR_ORDER comes first: that branch guards a route added later and no test reaches it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
CALLS = {"IGXProbeCreate": 5, "IGXProbeGetLocal": 3, "IGXProbeGeomMap": 2, "IGXProbeGetInfo": 5, "IGXProbeEvaluate": 4, "IGXProbeDestroy": 1}
ARG_WRONG, OUTOFRANGE, ORDER, SUP = 62, 63, 58, 56


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = _header()
    assert re.search(r"typedef\s+struct\s+_p_IGXProbe\s*\*\s*IGXProbe\s*;", text)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", text)}
    for name, nargs in CALLS.items():
        assert name in decl, "%s is not declared in include/petiga_amd.h" % name
        args = [a.strip() for a in decl[name].split(",") if a.strip()]
        assert len(args) == nargs, (name, args)
        f = getattr(P.lib(), name)                      # AttributeError: the library does not export it
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    L = P.lib()
    assert L.IGXProbeCreate.argtypes[1] is C.c_int and L.IGXProbeCreate.argtypes[2] is C.c_int64       # (iga, int order, int64_t npts, ...)
    assert L.IGXProbeEvaluate.argtypes[2] is C.c_int
    assert callable(P.IGX.probe) and all(hasattr(P.Probe, a) for a in ("evaluate", "geom_map", "local", "info", "close"))
    g = _box()
    info = g.probe(np.zeros((0, 3)), order=2).info()
    assert info == dict(npts=0, order=2, nsd=3, points_per_turn=P.PROBE_GRID_POINTS)      # the library's own figure, not a copy of it


def _box(setup=True, dim=3):
    import petiga_amd as P
    g = P.IGX(dim, 2)
    for i, (p, n) in enumerate(((2, 4), (3, 3), (1, 3))[:dim]):
        g.axis_uniform(i, p, n)
    if setup:
        g.setup()
    return g


def _create(g, order, npts, pts):
    import petiga_amd as P
    h = C.c_void_p()
    a = None if pts is None else np.ascontiguousarray(pts, dtype=np.float64)
    rc = P.lib().IGXProbeCreate(g.h if g is not None else None, order, npts, None if a is None else a.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
    return rc, P.lib().IGXGetLastError().decode(), h


def test_refusals_decided_before_any_hip_call():
    import petiga_amd as P
    L = P.lib()
    why = lambda: L.IGXGetLastError().decode()
    g = _box()
    ok = np.array([[0.5, 0.5, 0.5], [0.0, 1.0, 0.25]])
    # IGXProbeCreate
    for order in (-1, 4, 5, 100):
        rc, msg, _ = _create(g, order, 2, ok)
        assert rc == OUTOFRANGE and "probe" in msg and "order" in msg, (order, rc, msg)
    rc, msg, _ = _create(g, 4, 2, ok)
    assert "order 4" in msg and "0..3" in msg, msg                            # refused by name: the device keeps derivative slots 0..3
    rc, msg, _ = _create(g, 1, -1, ok)
    assert rc == OUTOFRANGE and "probe" in msg and "points" in msg, (rc, msg)
    rc, msg, _ = _create(g, 1, 2, None)
    assert rc == ARG_WRONG and "probe" in msg and "null" in msg, (rc, msg)
    rc, msg, _ = _create(None, 1, 2, ok)
    assert rc == ARG_WRONG and "probe" in msg, (rc, msg)
    assert L.IGXProbeCreate(g.h, 1, 0, None, None) == ARG_WRONG and "probe" in why()
    for bad, axis in ((float("nan"), 1), (-1e-9, 0), (1.0 + 1e-9, 2), (float("inf"), 1)):
        pts = np.tile(ok, (3, 1))
        pts[4, axis] = bad
        rc, msg, _ = _create(g, 1, 6, pts)
        assert rc == OUTOFRANGE and "probe" in msg and "point 4" in msg and "u[%d]" % axis in msg, (bad, axis, rc, msg)
    rc, msg, _ = _create(_box(setup=False), 1, 2, ok)
    assert rc == ORDER and "IGXSetUp" in msg and "probe" in msg, (rc, msg)
    with pytest.raises(P.IGXError) as e:
        _box().probe(ok, order=4)
    assert e.value.code == OUTOFRANGE and "probe" in str(e.value)

    # a probe of no points: legal, nothing launched; the calls on it
    rc, msg, h = _create(g, 2, 0, None)
    assert rc == 0 and h.value, (rc, msg)
    n = C.c_int64(-1)
    assert L.IGXProbeGetLocal(h, C.byref(n), None) == 0 and n.value == 0
    assert L.IGXProbeGeomMap(h, None) == 0
    for der in (-1, 3, 4):
        rc = L.IGXProbeEvaluate(h, None, der, None)
        assert rc == OUTOFRANGE and "probe" in why() and "der" in why(), (der, rc, why())
    rc = L.IGXProbeEvaluate(h, None, 1, None)
    assert rc == ARG_WRONG and "probe" in why() and "null" in why(), (rc, why())
    assert L.IGXProbeEvaluate(None, None, 0, None) == ARG_WRONG and "probe" in why()
    assert L.IGXProbeGetLocal(None, None, None) == ARG_WRONG and L.IGXProbeGeomMap(None, None) == ARG_WRONG
    assert L.IGXProbeGetInfo(None, None, None, None, None) == ARG_WRONG and L.IGXProbeGetInfo(h, None, None, None, None) == 0
    # stale after another IGXSetUp: every call
    g.setup()
    for rc in (L.IGXProbeGetLocal(h, C.byref(n), None), L.IGXProbeGeomMap(h, None), L.IGXProbeGetInfo(h, None, None, None, None), L.IGXProbeEvaluate(h, None, 0, None)):
        assert rc == ORDER
    assert "stale" in why() and "probe" in why() and "IGXSetUp" in why()
    assert L.IGXProbeDestroy(C.byref(h)) == 0 and not h.value
    assert L.IGXProbeDestroy(C.byref(h)) == 0 and L.IGXProbeDestroy(None) == 0
    # ... and a change of an axis without a new set-up
    p = g.probe(np.zeros((0, 3)), order=1)
    assert p.npts == 0 and p.local.shape == (0,) and p.geom_map().shape == (0, 3)
    g.axis_uniform(0, 2, 5)
    with pytest.raises(P.IGXError) as e:
        p.local
    assert e.value.code == ORDER
    p.close()
    p.close()


def test_degree_above_seven_never_reaches_a_probe():
    """IGX_ERR_SUP for a degree above 7: both set-up routes (IGXAxisSetDegree, IGXCreateFromTables) refuse it with that code, so no set-up
    space a probe could be made on holds one; IGXProbeCreate repeats the check under its own name for a route added later."""
    import petiga_amd as P
    g = P.IGX(1, 1)
    assert P.lib().IGXAxisSetDegree(g.h, 0, 8) == SUP
    assert P.lib().IGXAxisSetDegree(g.h, 0, 7) == 0
    g.axis_uniform(0, 7, 2)
    g.setup()
    p = g.probe(np.zeros((0, 1)), order=3)
    assert p.npts == 0
    p.close()
