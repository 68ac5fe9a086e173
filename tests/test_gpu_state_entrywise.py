"""The state-dependent kernels at a state that VARIES, against the point-wise long double reference (pointwise_ref.py), row by row and
entry by entry: |E - R| <= c u S with the project's constants (C_ID on the identity geometry, C_MAP on an affine map; calibrated on the
CPU oracle by test_pointwise_reference.py).

The entry-wise Bratu cases of test_gpu_entrywise.py use U = const, where lambda e^u is the same at every quadrature point: a kernel
that reads another lane's, point's or element's interpolated state passes them.  With a varying state these kernels were compared only
with the oracle -- the same point loop restated, in double -- at 1e-11 / 1e-12 of the largest entry.  Here:
  * vec_sumfact, Function / IFunction: Bratu (graded, affine, periodic, Dirichlet values) and Cahn-Hilliard IFunction, every row;
  * state_pencil<Bratu> (p = 2, 3; Jacobian, IJacobian; identity; p = 2 affine) and state_patch<Bratu>: every entry, with the pattern;
  * the fused Function + Jacobian walk: F every row, J every entry;
  * state_pencil<CahnHilliard> IJacobian, for which there is no entry reference: the engine's coordinate list times X, formed on the
    host in long double, against the point-wise action, every row, for two X.
Each case pins its kernel (the IGX_* switches are read when the engine is created) and asserts it ran.

Worst ratios on an MI355X (u S): vec_sumfact Bratu 6.4 (4.2 on an affine map), Cahn-Hilliard IFunction 0.25; state_pencil<Bratu> 32.6
(Jacobian, p = 3 graded; 25.0 on the affine map at p = 2), state_patch<Bratu> 13.7; the fused walk F 2.6, J 9.5;
state_pencil<CahnHilliard> times X 2.1 (p = 3, C = 1, graded, the wide X)."""
import numpy as np
import pytest

import pointwise_ref as PW
import tensor_ref as T
from test_gpu_entrywise import _env
from test_pointwise_reference import wide

pytestmark = pytest.mark.gpu

LD = T.LD
LAM, SHIFT, CH_SHIFT = 3.5, 4.0, 250.0
CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0)
_k = T.graded_knots


def _bcs(kind="all"):
    return {(d, s, 0): 0.2 + 0.1 * d - 0.15 * s for d in range(3) for s in range(2) if kind == "all" or (d + s) % 2 == 0}


BC3 = {(0, 0, 0): 0.2, (1, 1, 0): -0.1, (2, 0, 0): 0.3}
BC_CH = {(0, 0, 0): 0.6, (0, 1, 0): 0.66, (1, 1, 0): 0.61, (2, 0, 0): 0.65}
G3 = [_k(3, 6, 100.0), _k(3, 5, 0.01), _k(3, 6, 100.0)]
G2 = [_k(2, 5, 100.0), _k(2, 4, 0.01), _k(2, 3, 1000.0)]

# ---- vector passes.  name: (setup_case keywords, form)
VEC = {
    "bratu-p3-graded": (dict(p=3, N=0, knots=G3, bcs=_bcs()), "bratu"),
    "bratu-p2-graded": (dict(p=2, N=0, knots=G2, bcs=_bcs("some")), "bratu"),
    "bratu-p3-affine": (dict(p=3, N=[5, 4, 4], geometry="affine", seed=1, bcs=BC3), "bratu"),
    "bratu-p2-affine": (dict(p=2, N=[5, 4, 3], geometry="affine", seed=5, bcs=_bcs()), "bratu"),
    "bratu-p2-periodic": (dict(p=2, N=[6, 4, 5], periodic=[True, False, True], bcs={(1, 0, 0): 0.25}), "bratu"),
    "ch-p2-odd": (dict(p=2, N=[5, 4, 3]), "cahnhilliard"),
    "ch-p2-periodic": (dict(p=2, N=[6, 4, 5], periodic=[True, True, True]), "cahnhilliard"),
    "ch-p2-graded": (dict(p=2, N=0, knots=G2, bcs={(0, 0, 0): 0.6, (1, 1, 0): 0.61}), "cahnhilliard"),
    "ch-p3-C1": (dict(p=3, N=[4, 5, 3], C=[1, 1, 1]), "cahnhilliard"),
}
VEC_TESTS = [(n, d) for n, (_, f) in VEC.items() for d in (("function", "ifunction") if f == "bratu" else ("ifunction",))]

# ---- Tangents of Bratu.  name: (setup_case keywords, driver, environment, kernel-name substrings)
MAT = {
    "state-pencil-bratu-jacobian-p3-graded": (dict(p=3, N=0, knots=[_k(3, 8, 100.0), _k(3, 5, 0.01), _k(3, 4, 100.0)], bcs=_bcs()), "jacobian", {}, ("state_pencil<Bratu>",)),
    "state-pencil-bratu-ijacobian-p3": (dict(p=3, N=[8, 4, 5], bcs=_bcs("some")), "ijacobian", {}, ("state_pencil<Bratu>",)),
    "state-pencil-bratu-jacobian-p2": (dict(p=2, N=[9, 5, 4], bcs=_bcs()), "jacobian", {}, ("state_pencil<Bratu>",)),
    "state-pencil-bratu-ijacobian-p2-graded": (dict(p=2, N=0, knots=[_k(2, 9, 100.0), _k(2, 5, 0.01), _k(2, 4, 1000.0)], bcs=_bcs("some")), "ijacobian", {}, ("state_pencil<Bratu>",)),
    "state-pencil-geo-bratu-p2": (dict(p=2, N=[10, 5, 6], geometry="affine", seed=5, bcs=BC3), "ijacobian", {}, ("state_pencil<Bratu>", "mapped geometry")),
    "state-patch-bratu-p2": (dict(p=2, N=[12, 9, 6], bcs=_bcs("some")), "jacobian", {"IGX_PATCH_STATE": "1"}, ("state_patch<Bratu>",)),
}

# ---- the Tangent of Cahn-Hilliard.  name: setup_case keywords (the walk follows axis 0, which needs full continuity and eight elements:
# C = 1 is on the two other axes)
CH_MAT = {
    "ch-p2-uniform-dirichlet": dict(p=2, N=[9, 4, 5], bcs=BC_CH),
    "ch-p2-graded": dict(p=2, N=0, knots=[_k(2, 8, 100.0), _k(2, 4, 0.01), _k(2, 3, 1000.0)]),
    "ch-p3-C1-uniform": dict(p=3, N=[8, 4, 4], C=[2, 1, 1]),
    "ch-p3-C1-graded": dict(p=3, N=0, knots=[_k(3, 8, 100.0), _k(3, 3, 0.01, C=1), _k(3, 3, 100.0, C=1)]),
}


def _vectors(form, n):
    rng = np.random.default_rng(13)
    V = rng.standard_normal(n)
    U = 0.63 + 0.05 * (2 * rng.random(n) - 1) if form == "cahnhilliard" else 0.3 * rng.standard_normal(n)
    return U, V


def _setup(kw, form, monkeypatch, env=None):
    _env(monkeypatch, env or {})
    orc, eng, A = T.setup_case(dim=3, dof=1, engine=True, **kw)
    eng.set_form(form, (LAM,) if form == "bratu" else CH)
    pw = PW.PointwiseRef(orc, A=A, bcs=kw.get("bcs"))
    U, V = _vectors(form, orc.global_size())
    return eng, pw, U, V, (T.C_MAP if A is not None else T.C_ID)


def _names(eng, names):
    kn = eng.kernel_name()
    for s in names:
        assert s in kn, kn
    return kn


def _poisoned_vec(eng, n):
    return eng.create_vec().set(np.full(n, np.nan))       # the drivers zero their output themselves


@pytest.mark.parametrize("name,driver", VEC_TESTS)
def test_vector_pass_row_by_row(name, driver, monkeypatch):
    kw, form = VEC[name]
    eng, pw, U, V, c = _setup(kw, form, monkeypatch)
    Uv, Vv, F = eng.create_vec().set(U), eng.create_vec().set(V), _poisoned_vec(eng, U.size)
    if driver == "function":
        eng.compute_function(Uv, F)
        R, S = pw.bratu_function(LAM, U)
    else:
        eng.compute_ifunction(SHIFT if form == "bratu" else CH_SHIFT, Vv, 0.0, Uv, F)
        R, S = pw.bratu_function(LAM, U, V) if form == "bratu" else pw.ch_ifunction(CH, U, V)
    eng.synchronize()
    kn = _names(eng, ("vec_sumfact",))
    worst = PW.compare_rows(F.get(), R, S, c, pw.tref, "%s %s" % (name, driver))
    print("%-20s %-10s %-80s worst %.2f u S (c = %g)" % (name, driver, kn[:80], worst, c))


def _matrix(eng, driver, U, V):
    Uv, Vv, J = eng.create_vec().set(U), eng.create_vec().set(V), eng.create_mat()
    if driver == "jacobian":
        eng.compute_jacobian(Uv, J)
    else:
        eng.compute_ijacobian(SHIFT, Vv, 0.0, Uv, J)
    eng.synchronize()
    return J.to_coo_global()


@pytest.mark.parametrize("name", list(MAT))
def test_bratu_tangent_entrywise(name, monkeypatch):
    kw, driver, env, names = MAT[name]
    eng, pw, U, V, c = _setup(kw, "bratu", monkeypatch, env)
    r, cc, v = _matrix(eng, driver, U, V)
    kn = _names(eng, names)
    R, S = pw.bratu_entries(LAM, U, r, cc, SHIFT if driver == "ijacobian" else 0.0)
    worst = T.compare_entrywise((r, cc, v), R, S, c, pw.tref, name)
    print("%-40s %-80s %d entries, worst %.2f u S (c = %g)" % (name, kn[:80], r.size, worst, c))


def test_fused_function_and_jacobian_entrywise(monkeypatch):
    """IGXComputeFunctionJacobian / IFunctionIJacobian on the fused walk (IGX_FUSE_RESID=1, p = 2): F row by row, J entry by entry."""
    kw = dict(p=2, N=[9, 5, 4], bcs=_bcs("some"))
    eng, pw, U, V, c = _setup(kw, "bratu", monkeypatch, {"IGX_FUSE_RESID": "1"})
    Uv, Vv = eng.create_vec().set(U), eng.create_vec().set(V)
    for tag, shift, Vr in (("function+jacobian", 0.0, None), ("ifunction+ijacobian", SHIFT, V)):
        F, J = _poisoned_vec(eng, U.size), eng.create_mat()
        if Vr is None:
            eng.compute_function_jacobian(Uv, F, J)
        else:
            eng.compute_ifunction_ijacobian(shift, Vv, 0.0, Uv, F, J)
        eng.synchronize()
        kn = _names(eng, ("+Residual>",))
        wF = PW.compare_rows(F.get(), *pw.bratu_function(LAM, U, Vr), c, pw.tref, tag + " F")
        r, cc, v = J.to_coo_global()
        wJ = T.compare_entrywise((r, cc, v), *pw.bratu_entries(LAM, U, r, cc, shift), c, pw.tref, tag + " J")
        print("%-20s %-80s worst F %.2f, J %.2f u S (c = %g)" % (tag, kn[:80], wF, wJ, c))


@pytest.mark.parametrize("name", list(CH_MAT))
def test_cahn_hilliard_tangent_times_x_row_by_row(name, monkeypatch):
    kw = CH_MAT[name]
    eng, pw, U, V, c = _setup(kw, "cahnhilliard", monkeypatch)
    n = U.size
    Uv, Vv, J = eng.create_vec().set(U), eng.create_vec().set(V), eng.create_mat()
    eng.compute_ijacobian(CH_SHIFT, Vv, 0.0, Uv, J)
    eng.synchronize()
    kn = _names(eng, ("state_pencil<CahnHilliard>",))
    r, cc, v = J.to_coo_global()
    assert np.unique(r * n + cc).size == r.size and pw.tref.coupled(r, cc).all()
    _, valid = pw.tref.stencil(np.arange(n))
    assert np.array_equal(np.bincount(r, minlength=n), valid.sum(axis=1))       # every row's whole stencil
    worst = {}
    for tag, X in (("X", np.random.default_rng(37).standard_normal(n)), ("Xwide", wide(n, seed=5))):
        Y = np.zeros(n, dtype=LD)
        np.add.at(Y, r, v.astype(LD) * X[cc])
        R, S = pw.ch_action(CH, CH_SHIFT, U, X)
        worst[tag] = T.compare_entrywise((np.arange(n), Y), R, S, c, pw.tref, "%s %s" % (name, tag))
    print("%-26s %-80s worst %s u S (c = %g)" % (name, kn[:80], "  ".join("%s %.2f" % kv for kv in worst.items()), c))
