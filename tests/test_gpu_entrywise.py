"""Every kernel family against the tensor-product reference (tensor_ref.py), ENTRY BY ENTRY: |E - R| <= c u S, with S the sum of the
absolute values of the point terms (c_id on the identity geometry, c_map on an affine map; both calibrated on the CPU oracle by
test_tensor_reference.py).  The global tolerance of compare_mats (1e-12 of the largest entry) cannot see a far-band tile, a walk-axis
sum or a seam element that is wrong in its small entries; this check resolves every entry to its own rounding.  Each case pins its
kernel (set_kernel / the IGX_* switches, read when the engine is created) and asserts it ran."""
import numpy as np
import pytest

import tensor_ref as T

pytestmark = pytest.mark.gpu

LAM, STATE, VDOT, SHIFT = 3.5, 0.3, 0.7, 4.0
ENV = ("IGX_KERNEL", "IGX_NSEG", "IGX_GRAM_SUMFACT", "IGX_PATCH", "IGX_P2_PACK", "IGX_PATCH_STATE", "IGX_BLOCK_PENCIL",
       "IGX_VEC_SUMFACT", "IGX_STATE_PENCIL", "IGX_WALK_AXIS", "IGX_FUSE_RESID")


def _bcs(dim, dof=1, kind="all"):
    out = {}
    for d in range(dim):
        for s in range(2):
            for f in range(dof):
                if kind == "all" or (d + s + f) % 2 == 0:
                    out[(d, s, f)] = 1.0 + 0.5 * d - 0.25 * s + 0.125 * f
    return out


BC_C = {(d, s, 0): STATE for d in range(3) for s in range(2)}       # Dirichlet value = the constant state: the state stays constant
_k = T.graded_knots
G3 = [_k(3, 9, 100.0), _k(3, 8, 0.01), _k(3, 10, 100.0)]          # graded 1:100 (p = 3)
G2 = [_k(2, 10, 100.0), _k(2, 9, 0.01), _k(2, 8, 1000.0)]         # graded 1:100 / 1:1000 (p = 2)


def _user_poisson():
    from test_rtc_forms import USER_POISSON
    return USER_POISSON


# name: (setup_case keywords, engine form, form params, driver, env, set_kernel, kernel-name substrings)
CASES = {
    # gram_pencil p = 3, walk along axis 0, the walk-axis contraction sum-factorised (default)
    "gram-p3-sf-graded-system": (dict(dim=3, dof=1, p=3, N=0, knots=G3, bcs=_bcs(3)), "poisson", (), "system", {}, 0, ("gram_pencil", "p=3", "walk=0")),
    "gram-p3-sf-C1-matrix": (dict(dim=3, dof=1, p=3, N=[10, 0, 9], knots=[None, _k(3, 5, 1.0, C=1), None], bcs=_bcs(3)), "poisson", (), "matrix", {}, 0, ("gram_pencil", "p=3", "walk=0")),
    "gram-p3-sf-nseg4": (dict(dim=3, dof=1, p=3, N=[8, 6, 5], bcs=_bcs(3, kind="some")), "poisson_f", (), "system", {"IGX_NSEG": "4"}, 0, ("gram_pencil", "p=3")),
    "gram-p3-mfma-graded-system": (dict(dim=3, dof=1, p=3, N=0, knots=G3, bcs=_bcs(3)), "poisson", (), "system", {"IGX_GRAM_SUMFACT": "0"}, 0, ("gram_pencil", "p=3", "walk=0")),
    "gram-p3-periodic0": (dict(dim=3, dof=1, p=3, N=[10, 8, 9], periodic=[True, False, False], bcs={(1, 0, 0): 0.5, (2, 1, 0): -1.5}), "poisson", (), "system", {}, 0, ("gram_pencil", "p=3", "walk=0")),
    "gram-p3-walk2-C1-axis0": (dict(dim=3, dof=1, p=3, N=[9, 8, 10], C=[1, 2, 2], bcs=_bcs(3, kind="some")), "poisson", (), "system", {}, 0, ("gram_pencil", "walk=2", "gram_p3_element(faces)")),
    "gram-p3-element": (dict(dim=3, dof=1, p=3, N=[7, 6, 5], bcs=_bcs(3)), "poisson", (), "system", {}, 0, ("gram_p3_element",)),
    # p = 2: the patch walk (default), the pencil walk with packed tiles and without
    "gram-patch-p2-graded-system": (dict(dim=3, dof=1, p=2, N=0, knots=G2, bcs=_bcs(3, kind="some"), loads={(0, 1, 0): 1.5}), "poisson", (), "system", {}, 0, ("gram_patch",)),
    "gram-patch-p2-matrix": (dict(dim=3, dof=1, p=2, N=[12, 9, 8], bcs=_bcs(3)), "poisson", (), "matrix", {}, 0, ("gram_patch",)),
    "gram-pencil-p2-packed": (dict(dim=3, dof=1, p=2, N=0, knots=G2, bcs=_bcs(3)), "poisson", (), "system", {"IGX_PATCH": "0"}, 0, ("gram_pencil", "p=2", "packed tiles")),
    "gram-pencil-p2-unpacked": (dict(dim=3, dof=1, p=2, N=0, knots=G2, bcs=_bcs(3)), "poisson", (), "system", {"IGX_PATCH": "0", "IGX_P2_PACK": "0"}, 0, ("gram_pencil", "p=2")),
    # mapped geometry (affine; constant NURBS weights)
    "gram-p3-affine": (dict(dim=3, dof=1, p=3, N=[9, 6, 5], geometry="affine", seed=1, bcs=_bcs(3)), "poisson", (), "system", {}, 2, ("gram_pencil", "mapped geometry")),
    "gram-p2-affine": (dict(dim=3, dof=1, p=2, N=[10, 6, 5], geometry="affine", seed=2, bcs=_bcs(3, kind="some")), "poisson_f", (), "system", {}, 2, ("gram_pencil", "mapped geometry")),
    "gram-p3-rational": (dict(dim=3, dof=1, p=3, N=[8, 5, 6], geometry="rational", seed=3), "poisson", (), "matrix", {}, 2, ("gram_pencil", "mapped geometry")),
    # a run-time form on the walk
    "form-pencil-user-poisson": (dict(dim=3, dof=1, p=3, N=0, knots=G3, bcs=_bcs(3, kind="some")), "user", (1.0,), "system", {}, 2, ("form_pencil<UserPoisson>",)),
    # the feature kernel
    "feature-nqp5": (dict(dim=3, dof=1, p=3, N=[6, 5, 4], nqp=5, bcs=_bcs(3)), "poisson", (), "system", {}, 3, ("feature_assemble",)),
    "feature-lobatto": (dict(dim=3, dof=1, p=2, N=[7, 5, 4], rule="lobatto", bcs=_bcs(3, kind="some")), "poisson", (), "system", {}, 3, ("feature_assemble",)),
    "feature-mass-dof2": (dict(dim=3, dof=2, p=3, N=[6, 5, 4], bcs=_bcs(3, 2, "some")), "mass", (), "system", {}, 3, ("feature_assemble",)),
    "feature-mass-dof4": (dict(dim=3, dof=4, p=2, N=[5, 4, 4], bcs=_bcs(3, 4, "some")), "mass", (), "system", {}, 3, ("feature_assemble",)),
    "feature-2d": (dict(dim=2, dof=1, p=3, N=0, knots=[_k(3, 9, 100.0), _k(3, 7, 0.01)], bcs=_bcs(2)), "poisson", (), "system", {}, 3, ("feature_assemble",)),
    # the generic kernel
    "generic-reduced": (dict(dim=3, dof=1, p=3, N=[7, 4, 5], rule="reduced", bcs=_bcs(3, kind="some")), "poisson", (), "system", {}, 1, ("generic_assemble",)),
    "generic-p4": (dict(dim=3, dof=1, p=4, N=[5, 4, 4], bcs=_bcs(3)), "poisson", (), "system", {}, 1, ("generic_assemble",)),
    "generic-1d": (dict(dim=1, dof=1, p=3, N=0, knots=[_k(3, 12, 1000.0)], bcs={(0, 0, 0): 0.5, (0, 1, 0): -2.0}), "poisson", (), "system", {}, 1, ("generic_assemble",)),
    "generic-2d": (dict(dim=2, dof=1, p=2, N=[7, 6], periodic=[False, True], bcs={(0, 1, 0): 2.0}), "poisson_f", (), "system", {}, 1, ("generic_assemble",)),
    # multi-field
    "block-pencil-elasticity": (dict(dim=3, dof=3, p=3, N=[8, 5, 4], bcs=_bcs(3, 3, "some")), "elasticity", (1.3, 0.7), "system", {}, 4, ("block_pencil",)),
    "block-pencil-elasticity_f": (dict(dim=3, dof=3, p=3, N=[9, 5, 6], bcs={(0, 0, 1): 0.5}), "elasticity_f", (1.3, 0.7, 0.5, -1.0, 2.0), "system", {}, 4, ("block_pencil",)),
    "band-pt-elasticity-affine": (dict(dim=3, dof=3, p=3, N=[9, 4, 5], geometry="affine", seed=4, bcs=_bcs(3, 3, "some")), "elasticity", (1.3, 0.7), "system", {}, 4, ("band_pt", "mapped geometry")),
    "band-pt-elasticity-p2": (dict(dim=3, dof=3, p=2, N=[8, 5, 4], bcs=_bcs(3, 3, "some")), "elasticity", (1.3, 0.7), "system", {}, 4, ("band_pt", "p=2")),
    # state forms at a constant state
    "state-pencil-bratu-jacobian-p3": (dict(dim=3, dof=1, p=3, N=0, knots=G3, bcs=BC_C), "bratu", (LAM,), "jacobian", {}, 0, ("state_pencil<Bratu>",)),
    "state-pencil-bratu-ijacobian-p2": (dict(dim=3, dof=1, p=2, N=0, knots=G2), "bratu", (LAM,), "ijacobian", {}, 0, ("state_pencil<Bratu>",)),
    "state-pencil-bratu-jacobian-p2": (dict(dim=3, dof=1, p=2, N=[11, 6, 5], bcs=BC_C), "bratu", (LAM,), "jacobian", {}, 0, ("state_pencil<Bratu>",)),
    "state-pencil-bratu-ijacobian-p3": (dict(dim=3, dof=1, p=3, N=[9, 5, 6]), "bratu", (LAM,), "ijacobian", {}, 0, ("state_pencil<Bratu>",)),
    "state-patch-bratu-p2": (dict(dim=3, dof=1, p=2, N=[12, 9, 6], bcs=BC_C), "bratu", (LAM,), "jacobian", {"IGX_PATCH_STATE": "1"}, 0, ("state_patch<Bratu>",)),
    "state-pencil-geo-bratu-p2": (dict(dim=3, dof=1, p=2, N=[10, 5, 6], geometry="affine", seed=5), "bratu", (LAM,), "ijacobian", {}, 0, ("state_pencil<Bratu>", "mapped geometry")),
    # vector passes
    "vec-sumfact-bratu-function": (dict(dim=3, dof=1, p=3, N=0, knots=G3, bcs=BC_C), "bratu", (LAM,), "function", {}, 0, ("vec_sumfact",)),
    "vec-sumfact-bratu-ifunction": (dict(dim=3, dof=1, p=2, N=0, knots=G2), "bratu", (LAM,), "ifunction", {}, 0, ("vec_sumfact",)),
    "vec-sumfact-poisson-vector": (dict(dim=3, dof=1, p=2, N=[0, 5, 0], knots=[_k(2, 8, 100.0), None, _k(2, 6, 1.0, C=0)]), "poisson", (), "vector", {}, 0, ("vec_sumfact",)),
}


def _engine_form(eng, form, params):
    if form == "user":
        eng.set_form_source(_user_poisson(), "UserPoisson", params)
    else:
        eng.set_form(form, params)


def _ref_form(dim, dof, form, params, driver):
    if form in ("poisson", "user"):
        return T.poisson(dim)
    if form == "poisson_f":
        return T.poisson_f(dim)
    if form == "mass":
        return T.mass(dim, dof)
    if form == "elasticity":
        return T.elasticity(*params)
    if form == "elasticity_f":
        return T.elasticity(params[0], params[1], list(params[2:]))
    return T.bratu(dim, LAM, STATE, shift=SHIFT if driver.startswith("i") else 0.0, v=VDOT if driver == "ifunction" else 0.0)


def _env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(eng, driver):
    """(matrix or None, vector or None) of one driver."""
    A = b = U = V = None
    if driver in ("system", "matrix", "jacobian", "ijacobian"):
        A = eng.create_mat()
    if driver in ("system", "vector", "function", "ifunction"):
        b = eng.create_vec()
    if driver in ("jacobian", "ijacobian", "function", "ifunction"):
        n = int(np.prod(eng.sizes()["node_sizes"][:eng.dim])) * eng.dof
        U, V = eng.create_vec().set(np.full(n, STATE)), eng.create_vec().set(np.full(n, VDOT))
    {"system": lambda: eng.compute_system(A, b), "matrix": lambda: eng.compute_matrix(A), "vector": lambda: eng.compute_vector(b),
     "jacobian": lambda: eng.compute_jacobian(U, A), "ijacobian": lambda: eng.compute_ijacobian(SHIFT, V, 0.0, U, A),
     "function": lambda: eng.compute_function(U, b), "ifunction": lambda: eng.compute_ifunction(SHIFT, V, 0.0, U, b)}[driver]()
    eng.synchronize()
    return A, b


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_entrywise(name, monkeypatch):
    kw, form, params, driver, env, kernel, names = CASES[name]
    _env(monkeypatch, env)
    kw = dict(kw)
    dim, dof = kw["dim"], kw["dof"]
    orc, eng, Amap = T.setup_case(engine=True, **kw)
    _engine_form(eng, form, params)
    if kernel:
        eng.set_kernel(kernel)
    A, b = _run(eng, driver)
    kn = eng.kernel_name()
    for s in names:
        assert s in kn, (name, kn)
    rdriver = {"matrix": "matrix", "vector": "matrix", "function": "function", "ifunction": "function"}.get(driver, "system")
    ref = T.reference(orc, dim, _ref_form(dim, dof, form, params, driver), A=Amap, bcs=kw.get("bcs"), loads=kw.get("loads"), driver=rdriver)
    c = T.C_MAP if Amap is not None else T.C_ID
    worst = 0.0
    if A is not None:
        r, cc, v = A.to_coo_global()
        R, S = ref.entries(r, cc)
        worst = max(worst, T.compare_entrywise((r, cc, v), R, S, c, ref, name + " K"))
    if b is not None:
        bv = b.get()
        rows = np.arange(bv.size)
        R, S = ref.vector(rows)
        worst = max(worst, T.compare_entrywise((rows, bv), R, S, c, ref, name + " F"))
    print("%-34s %-90s worst %.2f u S (c = %g)" % (name, kn[:90], worst, c))


@pytest.mark.parametrize("family", ["gram", "block"])
def test_rank_boxes_entrywise(family, monkeypatch):
    """The local rows of each rank of a 2-rank partition, before the ghost-row exchange (one process, as test_sumfact_on_a_partition):
    the reference is the rank's element box."""
    _env(monkeypatch, {})
    for rank in range(2):
        if family == "gram":
            kw = dict(dim=3, dof=1, p=3, N=[10, 9, 16], box=(2, rank), bcs=_bcs(3))
            form, params, kernel, want, tf = "poisson", (), 0, "gram_pencil", T.poisson(3)
        else:
            kw = dict(dim=3, dof=3, p=3, N=[8, 5, 10], box=(2, rank), bcs=_bcs(3, 3, "some"))
            form, params, kernel, want, tf = "elasticity", (1.3, 0.7), 4, "block_pencil", T.elasticity(1.3, 0.7)
        orc, eng, _ = T.setup_case(engine=True, **kw)
        es, ew = eng.sizes()["elem_start"][:3], eng.sizes()["elem_width"][:3]
        r_o = orc.ranges()
        assert list(es) == list(r_o["elem_start"]) and list(ew) == list(r_o["elem_width"]), (es, ew, r_o)
        eng.set_form(form, params)
        if kernel:
            eng.set_kernel(kernel)
        A, b = _run(eng, "system")
        assert want in eng.kernel_name(), eng.kernel_name()
        ref = T.reference(orc, 3, tf, bcs=kw["bcs"])
        r, cc, v = A.to_coo_global()
        assert ref.coupled(r, cc).all()
        R, S = ref.entries(r, cc)
        worst = T.compare_entrywise((r, cc, v), R, S, T.C_ID, None, "%s rank %d K" % (family, rank))
        print("%s rank %d: %d entries, worst %.2f u S" % (family, rank, r.size, worst))
