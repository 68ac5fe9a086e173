"""Which walk an assembly of a scalar Gram form takes and how many launches it makes, counted from the colouring
(petiga_amd/csrc/pencil_launch.hpp): eng.coloring() gives the colours per axis and eng.element_color(axis, e) the colour of an element,
so a box of elements holds as many colours of an axis as its elements have distinct ones, and
  the pencil walk along axis w     one launch per non-empty pair of colours of the other two axes, per pass
  the patch walks                  one launch per colour of patches: min(SX, patches on axis 1) * min(SY, patches on axis 2), with
                                   SX x SY = 2 x 2 colours of 4 x 3 pencils at p = 2 and 2 x 3 colours of 4 x 2 pencils at p = 3
  gram_p3_element                  one launch per non-empty triple of colours
and eng.face_passes() the passes of a rank that forms the elements next to its upper faces first.  The shapes are the smallest at which
a plan can go wrong: a walk axis of 8 elements (the shortest that is walked), uneven colours (5 and 4 elements in 4 colours at p = 3,
in 3 at p = 2), meshes below the p = 3 patch walk's threshold, an axis 0 too short to walk, a mesh too short to walk at all, and a rank
with an upper neighbour on axis 2 that keeps 2 (p + 1) elements there.  Every test prints what it sees before it asserts (-s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CH = (3.0, 1.0 / (4 * np.pi ** 2 * 16))


def _engine(p, N, comm=None):
    import petiga_amd as P
    eng = P.IGX(3, 1)
    if comm:
        eng.set_comm(*comm)
    for i in range(3):
        eng.axis_uniform(i, p, N[i])
    eng.setup()
    return eng


def colours(eng, axis, lo=0, hi=None):
    """distinct colours of the rank's elements [lo, hi) of an axis"""
    hi = eng.sizes()["elem_width"][axis] if hi is None else hi
    return len({eng.element_color(axis, e) for e in range(lo, hi)})


def _colours_per_axis(eng):
    nc = eng.coloring()
    assert nc == [colours(eng, d) for d in range(3)]      # every colour of an axis holds an element
    return nc


def _run(eng, driver):
    A, b = eng.create_mat(), eng.create_vec()
    if driver == "system":
        eng.compute_system(A, b)
    else:
        eng.compute_matrix(A)
    eng.synchronize()
    return eng.last_timing()[2], eng.kernel_name()


def _say(what, N, nc, launches, want, name):
    print("%s on %s, colours %s: %d launches, the count %d; %s" % (what, "x".join(map(str, N)), nc, launches, want, name))


@pytest.mark.parametrize("driver", ["system", "matrix"])
def test_p3_pencil_walk_launches_once_per_colour_pair(driver):
    N = (8, 5, 4)
    eng = _engine(3, N)
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    launches, name = _run(eng, driver)
    _say("Poisson p = 3 %s" % driver, N, nc, launches, nc[1] * nc[2], name)
    assert name.startswith("gram_pencil(") and "p=3,walk=0" in name and "pencils per workgroup" not in name
    assert launches == nc[1] * nc[2]


@pytest.mark.parametrize("driver", ["system", "matrix"])
def test_p3_patch_walk_launches_once_per_patch_colour(driver, monkeypatch):
    monkeypatch.setenv("IGX_PATCH3", "2")
    N = (8, 9, 5)
    eng = _engine(3, N)
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    launches, name = _run(eng, driver)
    want = min(2, -(-N[1] // 4)) * min(3, -(-N[2] // 2))
    _say("Poisson p = 3 %s, IGX_PATCH3=2" % driver, N, nc, launches, want, name)
    assert name.startswith("gram_pencil(") and "p=3,walk=0,4x2 pencils per workgroup,one window" in name
    assert launches == want == 6


@pytest.mark.parametrize("N,count", [((8, 5, 4), 4), ((8, 4, 3), 1)])
def test_p2_patch_walk_skips_colours_without_a_patch(N, count):
    eng = _engine(2, N)
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    want = min(2, -(-N[1] // 4)) * min(2, -(-N[2] // 3))
    for driver in ("system", "matrix"):
        launches, name = _run(eng, driver)
        _say("Poisson p = 2 %s" % driver, N, nc, launches, want, name)
        assert name.startswith("gram_patch(") and "p=2,walk=0" in name and "4x3 pencils per workgroup" in name
        assert launches == want == count


def test_p2_pencil_walk_with_packed_tiles(monkeypatch):
    monkeypatch.setenv("IGX_PATCH", "0")
    N = (8, 5, 4)
    eng = _engine(2, N)
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    for driver in ("system", "matrix"):
        launches, name = _run(eng, driver)
        _say("Poisson p = 2 %s, IGX_PATCH=0" % driver, N, nc, launches, nc[1] * nc[2], name)
        assert name.startswith("gram_pencil(") and "p=2,walk=0" in name and "packed tiles" in name
        assert launches == nc[1] * nc[2]


def test_p3_walk_along_axis_2_when_axis_0_is_short():
    N = (5, 4, 8)
    eng = _engine(3, N)
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    launches, name = _run(eng, "matrix")
    _say("Poisson p = 3 matrix", N, nc, launches, nc[0] * nc[1], name)
    assert name.startswith("gram_pencil(") and "walk=2" in name and name.endswith("+gram_p3_element(faces)")
    assert launches == nc[0] * nc[1]


@pytest.mark.parametrize("driver", ["system", "matrix"])
def test_p3_element_kernel_when_no_axis_is_walkable(driver):
    N = (5, 4, 3)
    eng = _engine(3, N)
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    launches, name = _run(eng, driver)
    _say("Poisson p = 3 %s" % driver, N, nc, launches, nc[0] * nc[1] * nc[2], name)
    assert name.startswith("gram_p3_element(")
    assert launches == nc[0] * nc[1] * nc[2]


def test_p2_pencil_walk_on_a_mapped_net():
    from petiga_amd.geometry import greville
    N = (8, 5, 4)
    eng = _engine(2, N)
    gv = [greville(np.concatenate([[0.0] * 3, np.arange(1, n) / n, [1.0] * 3]), 2) for n in N]
    mesh = np.meshgrid(*gv[::-1], indexing="ij")[::-1]
    X = np.stack([m.copy() for m in mesh], axis=-1)
    X[..., 0] += 0.05 * np.sin(2 * np.pi * mesh[1]); X[..., 1] += 0.05 * np.sin(2 * np.pi * mesh[2])
    eng.set_geometry(X.reshape(-1, 3))
    eng.set_form("poisson")
    nc = _colours_per_axis(eng)
    for driver in ("system", "matrix"):
        launches, name = _run(eng, driver)
        _say("Poisson p = 2 %s, mapped" % driver, N, nc, launches, nc[1] * nc[2], name)
        assert name.startswith("gram_pencil(") and "p=2,walk=0,mapped geometry" in name
        assert launches == nc[1] * nc[2]


def test_tangent_walk_and_the_fused_residual(monkeypatch):
    monkeypatch.setenv("IGX_FUSE_RESID", "1")      # (read when the engine is created; the Jacobian driver alone does not look at it)
    N = (8, 5, 4)
    eng = _engine(2, N)
    eng.set_form("cahnhilliard", CH)
    nc = _colours_per_axis(eng)
    J, F = eng.create_mat(), eng.create_vec()
    U = eng.create_vec().set(0.63 + 0.05 * np.cos(0.37 * np.arange(F.n)))
    eng.compute_jacobian(U, J)
    eng.synchronize()
    launches, name = eng.last_timing()[2], eng.kernel_name()
    _say("Cahn-Hilliard p = 2 jacobian", N, nc, launches, nc[1] * nc[2], name)
    assert name.startswith("state_pencil<CahnHilliard>(") and "p=2,walk=0" in name and "packed tiles" in name
    assert launches == nc[1] * nc[2]
    eng.compute_function_jacobian(U, F, J)
    eng.synchronize()
    launches, name = eng.last_timing()[2], eng.kernel_name()
    _say("Cahn-Hilliard p = 2 function + jacobian", N, nc, launches, nc[1] * nc[2], name)
    assert name.startswith("state_pencil<CahnHilliard+Residual>(") and "p=2,walk=0" in name and "packed tiles" in name
    assert launches == nc[1] * nc[2]


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_upper_face_first_passes_of_a_rank(overlap, monkeypatch):
    monkeypatch.setenv("IGX_OVERLAP", overlap)
    N = (8, 5, 16)
    eng = _engine(3, N, comm=(2, 0))      # rank 0 of 2: the partition cuts axis 2, the rank keeps 8 = 2 (p + 1) elements there
    sz = eng.sizes()
    assert sz["proc_sizes"] == [1, 1, 2] and sz["elem_width"] == [8, 5, 8]
    eng.set_form("poisson")
    eng.comm_init_transport(lambda send, recv: None)      # a communicator is all the assembly looks at; nothing is exchanged here
    n2 = sz["elem_width"][2]
    cut = n2 // 2      # the upper half of the axis first, a multiple of p + 1
    boxes = [(cut, n2), (0, cut)] if overlap == "1" else [(0, n2)]
    want = sum(colours(eng, 1) * colours(eng, 2, lo, hi) for lo, hi in boxes)
    launches, name = _run(eng, "system")
    print("Poisson p = 3 system, rank 0 of 2 on %s, IGX_OVERLAP=%s, boxes of axis 2 %s: %d passes, %d launches, the count %d; %s" % (
        "x".join(map(str, N)), overlap, boxes, eng.face_passes(), launches, want, name))
    assert name.startswith("gram_pencil(") and "p=3,walk=0" in name
    assert eng.face_passes() == len(boxes)
    assert launches == want
    if overlap == "1":      # each box holds every colour of axis 2: twice the launches of the one pass
        assert all(colours(eng, 2, lo, hi) == eng.coloring()[2] for lo, hi in boxes) and launches == 2 * colours(eng, 1) * eng.coloring()[2]
