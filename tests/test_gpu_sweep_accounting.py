"""How many launches the two element kernels make, counted from the colouring (petiga_amd/csrc/element_sweep.hpp): the point-form kernel
(IGXSetKernel 1, generic_assemble) and the feature-GEMM kernel (IGXSetKernel 3, feature_assemble) launch one kernel per non-empty
combination of colours -- eng.coloring() gives the colours per axis, and every colour of an axis holds an element --
  interior sweep                 nc0 * nc1 * nc2
  each visited face on the rank  the product over the other two axes (the face axis is one element layer)
  functionals                    one sweep of all elements plus one per visited face (nothing is scattered, so no colours)
for built-in forms and for their run-time twins alike, and the kernel's name tells the family and where Phi lives (phi=LDS | phi=HBM) or
the chunks of points (chunks=).  The shapes are the smallest at which a sweep can go wrong: uneven colour sizes and an axis with fewer
elements than colours (p = 2 on 5 x 4 x 2), Phi in an HBM slice on the point-form kernel (p = 3 on 4 x 5 x 3), dim 2 and dim 1, and a
periodic axis of 4 elements at p = 2, where every element is its own colour.  Every test prints what it sees before it asserts (-s)."""
import os

import pytest

from test_rtc_boundary_scalar import FUNCTIONALS, NITSCHE
from test_rtc_forms import ADVECTION_DIFFUSION, USER_ELASTICITY

pytestmark = pytest.mark.gpu

A3 = dict(p=2, N=(5, 4, 2))
B3 = dict(p=3, N=(4, 5, 3))
C2 = dict(p=2, N=(5, 4))
D1 = dict(p=2, N=(5,))
E2 = dict(p=2, N=(4, 5), periodic=(True, False))
E3 = dict(p=2, N=(3, 4, 2), periodic=(False, True, False))


@pytest.fixture(scope="module", autouse=True)
def one_compile_per_struct(tmp_path_factory):
    """the code objects of the run-time structs are kept on disk for the module: every struct is compiled once per kernel instantiation"""
    old = os.environ.get("IGX_RTC_CACHE_DIR")
    os.environ["IGX_RTC_CACHE_DIR"] = str(tmp_path_factory.mktemp("rtc_cache"))
    yield
    if old is None:
        del os.environ["IGX_RTC_CACHE_DIR"]
    else:
        os.environ["IGX_RTC_CACHE_DIR"] = old


def _engine(dof, p, N, periodic=None, faces=()):
    import petiga_amd as P
    dim = len(N)
    eng = P.IGX(dim, dof)
    for i in range(dim):
        eng.axis_uniform(i, p, N[i], periodic=bool(periodic and periodic[i]))
    eng.setup()
    for a, s in faces:
        eng.set_boundary_form(a, s, True)
    return eng


def _two_faces(dim):
    return ((0, 1), (0, 0)) if dim == 1 else ((0, 1), (dim - 1, 0))


def sweep_count(nc, dim, faces, functional=False):
    """launches of one element kernel over the rank, from the colours per axis"""
    if functional:
        return 1 + len(faces)
    nc = list(nc[:dim]) + [1] * (3 - dim)
    count = nc[0] * nc[1] * nc[2]
    for a, _ in faces:
        count += nc[0] * nc[1] * nc[2] // nc[a]
    return count


def _family(name, kernel, phi):
    if kernel == 1:
        return "generic_assemble" in name and ("phi=" + phi) in name
    return "feature_assemble" in name and "chunks=" in name


def _assemble(eng, kernel, drivers):
    """(launches, kernel name) of every driver under that kernel choice"""
    eng.set_kernel(kernel)
    A, b = eng.create_mat(), eng.create_vec()
    seen = []
    for d in drivers:
        {"system": lambda: eng.compute_system(A, b), "matrix": lambda: eng.compute_matrix(A), "vector": lambda: eng.compute_vector(b)}[d]()
        eng.synchronize()
        seen.append((d, eng.last_timing()[2], eng.kernel_name()))
    return seen


FORMS = {
    # name: (dof, built-in form and parameters or None, run-time source, struct name by dim, parameters, visits two faces)
    "poisson": (1, ("poisson", ()), ADVECTION_DIFFUSION, "AdvDiff<%d>", (1.0, 0.5, 0.25), False),
    "mass2": (2, ("mass", ()), None, None, (), False),
    "elasticity": (3, ("elasticity", (2.5, 0.7)), USER_ELASTICITY, "UserElasticity<0>", (2.5, 0.7), False),
    "nitsche": (1, ("nitsche", (2.0,)), NITSCHE, "UserNitsche<%d>", (2.0,), True),
}


@pytest.mark.parametrize("form,shape", [("poisson", A3), ("poisson", B3), ("poisson", C2), ("poisson", D1), ("poisson", E2), ("poisson", E3),
                                        ("mass2", A3), ("mass2", C2), ("elasticity", A3), ("elasticity", B3),
                                        ("nitsche", A3), ("nitsche", B3), ("nitsche", C2), ("nitsche", D1), ("nitsche", E3)],
                         ids=lambda v: v if isinstance(v, str) else "p%d-%s%s" % (v["p"], "x".join(map(str, v["N"])), "-periodic" if v.get("periodic") else ""))
def test_element_sweeps_launch_once_per_colour_combination(form, shape):
    dof, builtin, source, struct, params, visits = FORMS[form]
    p, N, periodic = shape["p"], shape["N"], shape.get("periodic")
    dim = len(N)
    faces = _two_faces(dim) if visits else ()
    # Phi = nqp * nen * (1 + dim) doubles: 128 KiB at p = 3 in 3-D, an HBM slice; 23 KiB at most in the other shapes, in LDS next to a few KiB of element data
    phi = "HBM" if (p + 1) ** (2 * dim) * (1 + dim) * 8 > 64 * 1024 else "LDS"
    kernels = (1, 3) if dim >= 2 else (1,)      # the feature kernel needs dim >= 2
    counts = {}
    for twin in ("built-in", "run-time"):
        if twin == "run-time" and source is None:
            continue
        eng = _engine(dof, p, N, periodic, faces)
        if twin == "built-in":
            eng.set_form(*builtin)
        else:
            eng.set_form_source(source, struct % dim if "%d" in struct else struct, params)
        nc = eng.coloring()
        want = sweep_count(nc, dim, faces)
        for kernel in kernels:
            for driver, launches, name in _assemble(eng, kernel, ("system", "matrix", "vector")):
                print("%s %s, p = %d on %s%s, colours %s, faces %s, kernel %d, %s: %d launches, the count %d; %s" % (
                    form, twin, p, N, " periodic %s" % (periodic,) if periodic else "", nc[:dim], list(faces), kernel, driver, launches, want, name))
                assert launches == want
                assert _family(name, kernel, phi)
                assert ("hiprtc" in name) == (twin == "run-time")
                counts[(twin, kernel, driver)] = launches
    if periodic:      # every element of the wrapped axis is its own colour
        assert [nc[d] for d in range(dim) if periodic[d]] == [N[d] for d in range(dim) if periodic[d]]
    for (twin, kernel, driver), n in counts.items():      # both take the same family under a kernel choice: equal counts
        assert n == counts[("built-in", kernel, driver)]


@pytest.mark.parametrize("shape", [A3, C2, D1], ids=lambda v: "p%d-%s" % (v["p"], "x".join(map(str, v["N"]))))
def test_functionals_take_one_sweep_and_one_per_visited_face(shape):
    p, N = shape["p"], shape["N"]
    dim = len(N)
    for faces in ((), _two_faces(dim)):
        eng = _engine(1, p, N, None, faces)
        U = eng.create_vec().fill(0.5)
        want = sweep_count(eng.coloring(), dim, faces, functional=True)
        for kernel in (1, 3) if dim >= 2 else (1,):
            eng.set_kernel(kernel)
            v = eng.compute_scalar("volume")
            seen = [("volume built-in", eng.last_timing()[2], eng.kernel_name())]
            e = eng.compute_scalar("x2err", U)
            seen.append(("x2err built-in", eng.last_timing()[2], eng.kernel_name()))
            m = eng.compute_scalar_source(FUNCTIONALS, "UserMeasures<%d>" % dim, 3, U, (0.75,))
            seen.append(("UserMeasures run-time", eng.last_timing()[2], eng.kernel_name()))
            x = eng.compute_scalar_source(FUNCTIONALS, "UserX2Err<%d>" % dim, 1, U)
            seen.append(("UserX2Err run-time", eng.last_timing()[2], eng.kernel_name()))
            for what, launches, name in seen:
                print("%s, p = %d on %s, faces %s, kernel %d: %d launches, the count %d; %s" % (what, p, N, list(faces), kernel, launches, want, name))
                assert launches == want
                # a run-time functional has the point-form kernel alone
                assert _family(name, 1 if "run-time" in what else kernel, "LDS")
            assert abs(m[0] - v[0]) <= 1e-13 * abs(v[0]) and abs(m[1] - v[1]) <= 1e-13 * max(abs(v[1]), 1.0)
            assert abs(x[0] - e[0]) <= 1e-13 * abs(e[0])
