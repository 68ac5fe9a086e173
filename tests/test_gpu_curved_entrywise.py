"""Every kernel that evaluates a mapped geometry, on CURVED maps with varying rational weights, against the long double reference of
curved_ref.py, ENTRY BY ENTRY and ROW BY ROW: |E - R| <= c u S.

The entry-wise files beside this one draw their mapped cases from an affine map (constant NURBS weights included), where the Jacobian
is the same at every point, the map's second derivatives vanish and W is constant; the warped geometries of common.warped_geometry ran
through compare_mats only (1e-11 / 1e-12 of the largest free entry).  Here the geometry is warped_geometry's, polynomial ("poly") or
with random weights in [0.8, 1.2] ("nurbs"), and every entry of every matrix (to_coo_global) and every row of every vector is compared.
Each case pins its kernel (set_kernel, the IGX_* switches) and asserts it ran.  c is tensor_ref.C_MAP, calibrated on the CPU oracle
alone by test_curved_reference.py, which runs every case of this file through the oracle.

Every test prints `name, kernel, worst ratio` (lines starting CURVED).  Worst ratios on an MI355X (u S; c = 256): gram_pencil 1.31 on the
polynomial map (p = 3, Matrix), 0.11 on NURBS maps (0.09 graded 1:4, 0.07 with a periodic walk axis, 0.13 on one rank of two);
form_pencil<UserPoisson> 0.08; feature_assemble 0.47 (mass, two fields), 0.07 as the fallback of the refused p = 3 Tangent;
generic_assemble K 0.37, F 0.70 (reduced rule); band_pt 0.56 ("mapped geometry"), 0.08 ("NURBS geometry"); state_pencil<Bratu> 0.30
(polynomial), 0.04 (NURBS); state_pencil<CahnHilliard> probed below 0.005; vec_sumfact Function / IFunction 2.50 (a Dirichlet row
m (U - v); Poisson Vector 0.49, Cahn-Hilliard below 0.005); the actions row by row 2.99 (Poisson p = 3, the wide X), recovered entries
2.54, one workgroup per element below 0.005; the diagonals 0.03, the blocks 0.01.  The NURBS figures are smaller than the polynomial
ones because S grows with the abs-sums of the weight function's derivatives (curved_ref.py), not because the kernels differ.  The
oracle's own ratios on the same cases are in test_curved_reference.py; no kernel exceeds them by more than a factor of four."""
import numpy as np
import pytest

import curved_ref as CR
import pointwise_ref as PW
import tensor_ref as T
from common import warped_geometry
from test_gpu_entrywise import _bcs, _engine_form, _env, _ref_form, _run
from test_pointwise_reference import wide

pytestmark = pytest.mark.gpu

LD = T.LD
C_CURVED = T.C_MAP
LAM, SHIFT, CH_SHIFT = 3.5, 4.0, 250.0
CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0)
EL = (1.3, 0.7)
ELF = (1.3, 0.7, 0.5, -1.0, 2.0)
_k = T.graded_knots
G4 = [_k(3, 9, 4.0), _k(3, 5, 0.25), _k(3, 5, 4.0)]                # mildly graded, 1:4
BC3 = {(0, 0, 0): 0.2, (1, 1, 0): -0.1, (2, 0, 0): 0.3}
BC_S = {(d, s, 0): 0.2 + 0.1 * d - 0.15 * s for d in range(3) for s in range(2) if (d + s) % 2 == 0}
BC_CH = {(0, 0, 0): 0.6, (0, 1, 0): 0.66, (1, 1, 0): 0.61, (2, 0, 0): 0.65}
EL_BCS = {(0, 0, 0): 0.0, (0, 0, 1): 0.5, (0, 0, 2): -0.25, (2, 1, 0): 1.0, (1, 0, 2): 0.75}


def _spec(geo, seed, **kw):
    """(setup_case keywords, "poly" / "nurbs", seed of the warp)"""
    kw.setdefault("dof", 1)
    return kw, geo, seed


# ---- assembly.  name: (spec, engine form, form params, driver, environment, set_kernel, kernel-name substrings)
ASM = {
    # gram_pencil on a mapped geometry
    "gram-p3-nurbs-system": (_spec("nurbs", 1, p=3, N=[9, 6, 5], bcs=_bcs(3)), "poisson", (), "system", {}, 2, ("gram_pencil", "p=3", "mapped geometry")),
    "gram-p3-poly-matrix": (_spec("poly", 2, p=3, N=[8, 5, 6], bcs=_bcs(3)), "poisson", (), "matrix", {}, 2, ("gram_pencil", "p=3", "mapped geometry")),
    "gram-p2-nurbs-poisson_f": (_spec("nurbs", 3, p=2, N=[10, 6, 5], bcs=_bcs(3, kind="some")), "poisson_f", (), "system", {}, 2, ("gram_pencil", "p=2", "mapped geometry")),
    "gram-p3-graded4-nurbs": (_spec("nurbs", 4, p=3, N=0, knots=G4, bcs=_bcs(3, kind="some")), "poisson", (), "system", {}, 2, ("gram_pencil", "p=3", "mapped geometry")),
    "gram-p3-periodic0-nurbs": (_spec("nurbs", 5, p=3, N=[10, 5, 4], periodic=[True, False, False], bcs={(1, 0, 0): 0.5, (2, 1, 0): -1.5}), "poisson", (), "system", {}, 2, ("gram_pencil", "walk=0", "mapped geometry")),
    # a run-time form on the walk
    "form-pencil-user-poisson-nurbs": (_spec("nurbs", 6, p=3, N=[9, 5, 4], bcs=_bcs(3, kind="some")), "user", (1.0,), "system", {}, 2, ("form_pencil<UserPoisson>", "mapped geometry")),
    # the feature kernel
    "feature-nqp5-nurbs": (_spec("nurbs", 7, p=3, N=[6, 5, 4], nqp=5, bcs=_bcs(3)), "poisson", (), "system", {}, 3, ("feature_assemble",)),
    "feature-mass-dof2-nurbs": (_spec("nurbs", 8, dof=2, p=3, N=[6, 5, 4], bcs=_bcs(3, 2, "some")), "mass", (), "system", {}, 3, ("feature_assemble",)),
    # the generic kernel
    "generic-p4-nurbs": (_spec("nurbs", 9, p=4, N=[5, 4, 4], bcs=_bcs(3)), "poisson", (), "system", {}, 1, ("generic_assemble",)),
    "generic-reduced-poly": (_spec("poly", 10, p=3, N=[7, 4, 5], rule="reduced", bcs=_bcs(3, kind="some")), "poisson", (), "system", {}, 1, ("generic_assemble",)),
    # band_pt: both geometry instantiations
    "band-pt-elasticity-poly": (_spec("poly", 11, dof=3, p=3, N=[9, 4, 5], bcs=_bcs(3, 3, "some")), "elasticity", EL, "system", {}, 4, ("band_pt", "p=3", "mapped geometry")),
    "band-pt-elasticity-nurbs": (_spec("nurbs", 12, dof=3, p=3, N=[9, 4, 5], bcs=_bcs(3, 3, "some")), "elasticity", EL, "system", {}, 4, ("band_pt", "p=3", "NURBS geometry")),
    "band-pt-elasticity_f-p2-nurbs": (_spec("nurbs", 13, dof=3, p=2, N=[8, 5, 4], bcs={(0, 0, 1): 0.5}), "elasticity_f", ELF, "system", {}, 4, ("band_pt", "p=2", "NURBS geometry")),
}
RANKS = _spec("nurbs", 14, p=3, N=[10, 9, 16], bcs=_bcs(3))         # one rank of two: box=(2, rank)

# ---- Tangents of Bratu at a varying state (p = 2: state_pencil_geo).  name: (spec, driver)
STATE = {
    "state-pencil-geo-bratu-jacobian-poly": (_spec("poly", 15, p=2, N=[10, 5, 6], bcs=BC3), "jacobian"),
    "state-pencil-geo-bratu-ijacobian-poly": (_spec("poly", 15, p=2, N=[10, 5, 6], bcs=BC3), "ijacobian"),
    "state-pencil-geo-bratu-jacobian-nurbs": (_spec("nurbs", 16, p=2, N=[10, 5, 6], bcs=BC_S), "jacobian"),
    "state-pencil-geo-bratu-ijacobian-nurbs": (_spec("nurbs", 16, p=2, N=[10, 5, 6], bcs=BC_S), "ijacobian"),
}
CH_TANGENT = _spec("nurbs", 17, p=2, N=[8, 3, 4], bcs={(0, 0, 0): 0.6, (1, 1, 0): 0.61})       # state_pencil_geo<CahnHilliard>, probed
REFUSED = _spec("nurbs", 18, p=3, N=[8, 4, 4], bcs=BC3)            # a Tangent on a mapped geometry at p = 3: the walk refuses

# ---- vector passes (vec_sumfact, GEO).  name: (spec, form, driver)
VEC = {
    "bratu-p3-nurbs-function": (_spec("nurbs", 19, p=3, N=[5, 4, 4], bcs=BC3), "bratu", "function"),
    "bratu-p3-nurbs-ifunction": (_spec("nurbs", 19, p=3, N=[5, 4, 4], bcs=BC3), "bratu", "ifunction"),
    "bratu-p2-nurbs-function": (_spec("nurbs", 20, p=2, N=[5, 4, 3], bcs=BC_S), "bratu", "function"),
    "bratu-p2-nurbs-ifunction": (_spec("nurbs", 20, p=2, N=[5, 4, 3], bcs=BC_S), "bratu", "ifunction"),
    "poisson-p2-poly-vector": (_spec("poly", 21, p=2, N=[6, 5, 4]), "poisson", "vector"),
    "ch-p2-nurbs-ifunction": (_spec("nurbs", 22, p=2, N=[5, 4, 3], bcs=BC_CH), "cahnhilliard", "ifunction"),
}

# ---- matrix-free (vec_sumfact, ACTION / DIAGONAL / BLOCK).  name: (spec, form, driver, lanes per axis of a one-workgroup layout or 0)
FREE = {
    "poisson-p3-nurbs": (_spec("nurbs", 23, p=3, N=[4, 4, 3], bcs=BC3), "poisson", "matrix", 0),
    "bratu-p2-poly": (_spec("poly", 24, p=2, N=[5, 4, 3], bcs=BC3), "bratu", "jacobian", 0),
    "ch-p2-nurbs": (_spec("nurbs", 25, p=2, N=[5, 4, 3], bcs=BC_CH), "cahnhilliard", "ijacobian", 0),
    "elasticity-p2-nurbs": (_spec("nurbs", 26, dof=3, p=2, N=[4, 3, 3], bcs=EL_BCS), "elasticity", "matrix", 0),
    "poisson-p4-nurbs": (_spec("nurbs", 27, p=4, N=[2, 2, 2], bcs=BC_S), "poisson", "matrix", 6),
    "poisson-p6-nurbs": (_spec("nurbs", 28, p=6, N=[2, 2, 1], bcs=BC3), "poisson", "matrix", 8),
}
PROBE = ["poisson-p3-nurbs"]
DIAGONAL = ["elasticity-p2-nurbs", "poisson-p4-nurbs", "poisson-p6-nurbs"]
BLOCK = "elasticity-p2-nurbs"


# ---- set-up and references, shared with test_curved_reference.py (which runs them on the CPU oracle)
def setup(spec, engine, box=None, bcs=True):
    """(oracle, engine or None, X, W, bcs) of a spec on its warped geometry."""
    kw, geo, seed = spec
    kw = dict(kw)
    values = kw.pop("bcs", None)
    if not bcs:                                             # (the oracle has no Matrix / Vector driver: its System without values)
        values = None
    orc, eng, _ = T.setup_case(dim=3, engine=engine, box=box, **kw)
    X, W = warped_geometry(orc, 3, seed=seed, rational=(geo == "nurbs"), amp=0.15)
    for g in (orc, eng):
        if g is not None:
            g.set_geometry(X, W)
            for (d, s, f), v in (values or {}).items():
                g.set_boundary_value(d, s, f, v)
    return orc, eng, X, W, values


def vectors(form, n, seed=13):
    """(U, V) of a state form: the states of test_gpu_state_entrywise.py."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal(n)
    U = 0.63 + 0.05 * (2 * rng.random(n) - 1) if form == "cahnhilliard" else 0.3 * rng.standard_normal(n)
    return U, V


def linear_reference(cr, form, params, driver):
    """(K: curved_ref.Entries, F, FS) of a constant-coefficient form."""
    return cr.linear(_ref_form(3, cr.dof, form, params, driver), "matrix" if driver in ("matrix", "vector") else "system")


def free_reference(cr, form, driver, U):
    """(the matrix's curved_ref.Entries or None, action(X) -> (R, S)) of a matrix-free case."""
    if form in ("poisson", "elasticity"):
        K = cr.linear(T.poisson(3) if form == "poisson" else T.elasticity(*EL), "system")[0]
        return K, K.action
    if form == "bratu":
        shift = SHIFT if driver == "ijacobian" else 0.0
        return cr.bratu_matrix(LAM, U, shift), lambda X: cr.bratu_action(LAM, U, X, shift)
    return None, lambda X: cr.ch_action(CH, CH_SHIFT, U, X)


def vector_reference(cr, form, driver, U, V):
    if form == "poisson":
        return cr.linear(T.poisson(3), "matrix")[1:]
    if form == "bratu":
        return cr.bratu_function(LAM, U, V if driver == "ifunction" else None)
    return cr.ch_ifunction(CH, U, V)


def colour_indicators(cr):
    """(colour of every node, number of colours) such that no row couples with two columns of one colour."""
    colour, ncol, _ = PW.colouring(cr.tref.tabs, cr.dof)
    return colour, ncol


# ---- the tests
def _names(eng, names):
    kn = eng.kernel_name()
    for s in names:
        assert s in kn, kn
    return kn


def _report(name, kn, worst):
    print("CURVED %-40s %-72s worst %s u S (c = %g)" % (name, kn[:72], worst if isinstance(worst, str) else "%.2f" % worst, C_CURVED))


@pytest.mark.parametrize("name", list(ASM))
def test_assembly_entrywise(name, monkeypatch):
    spec, form, params, driver, env, kernel, names = ASM[name]
    _env(monkeypatch, env)
    orc, eng, X, W, bcs = setup(spec, True)
    _engine_form(eng, form, params)
    eng.set_kernel(kernel)
    A, b = _run(eng, driver)
    kn = _names(eng, names)
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    assert cr.detv.min() >= 0.5
    K, F, FS = linear_reference(cr, form, params, driver)
    r, cc, v = A.to_coo_global()
    worst = {"K": T.compare_entrywise((r, cc, v), *K.at(r, cc), C_CURVED, cr.tref, name + " K")}
    if b is not None:
        worst["F"] = PW.compare_rows(b.get(), F, FS, C_CURVED, cr.tref, name + " F")
    _report(name, kn, "  ".join("%s %.2f" % kv for kv in worst.items()))


@pytest.mark.parametrize("rank", [0, 1])
def test_rank_box_entrywise(rank, monkeypatch):
    """The local rows of one rank of two before the ghost-row exchange, as test_gpu_entrywise.test_rank_boxes_entrywise: the reference
    is the rank's element box."""
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(RANKS, True, box=(2, rank))
    es, ew, r_o = eng.sizes()["elem_start"][:3], eng.sizes()["elem_width"][:3], orc.ranges()
    assert list(es) == list(r_o["elem_start"]) and list(ew) == list(r_o["elem_width"]), (es, ew, r_o)
    eng.set_form("poisson")
    eng.set_kernel(2)
    A, b = _run(eng, "system")
    kn = _names(eng, ("gram_pencil", "mapped geometry"))
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    K = cr.linear(T.poisson(3), "system")[0]
    r, cc, v = A.to_coo_global()
    assert cr.tref.coupled(r, cc).all()
    worst = T.compare_entrywise((r, cc, v), *K.at(r, cc), C_CURVED, None, "rank %d K" % rank)
    _report("gram-p3-nurbs-rank%d" % rank, kn, worst)


def _tangent(eng, driver, U, V, shift):
    Uv, Vv, J = eng.create_vec().set(U), eng.create_vec().set(V), eng.create_mat()
    if driver == "jacobian":
        eng.compute_jacobian(Uv, J)
    else:
        eng.compute_ijacobian(shift, Vv, 0.0, Uv, J)
    eng.synchronize()
    return J.to_coo_global()


@pytest.mark.parametrize("name", list(STATE))
def test_bratu_tangent_entrywise(name, monkeypatch):
    spec, driver = STATE[name]
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(spec, True)
    eng.set_form("bratu", (LAM,))
    U, V = vectors("bratu", orc.global_size())
    r, cc, v = _tangent(eng, driver, U, V, SHIFT)
    kn = _names(eng, ("state_pencil<Bratu>", "mapped geometry"))
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    J = cr.bratu_matrix(LAM, U, SHIFT if driver == "ijacobian" else 0.0)
    _report(name, kn, T.compare_entrywise((r, cc, v), *J.at(r, cc), C_CURVED, cr.tref, name))


def test_cahn_hilliard_tangent_probed_entrywise(monkeypatch):
    """state_pencil_geo<CahnHilliard>: every entry of the IJacobian.  The columns are coloured so that no row couples with two columns
    of one colour; the engine's coordinate list times a colour's indicator vector, formed on the host in long double, is then one entry
    per row, compared with ch_action on the same indicator."""
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(CH_TANGENT, True)
    eng.set_form("cahnhilliard", CH)
    n = orc.global_size()
    U, V = vectors("cahnhilliard", n)
    r, cc, v = _tangent(eng, "ijacobian", U, V, CH_SHIFT)
    kn = _names(eng, ("state_pencil<CahnHilliard>", "mapped geometry"))
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    assert np.unique(r * n + cc).size == r.size and cr.tref.coupled(r, cc).all()
    _, valid = cr.tref.stencil(np.arange(n))
    assert np.array_equal(np.bincount(r, minlength=n), valid.sum(axis=1))       # every row's whole stencil
    colour, ncol = colour_indicators(cr)
    worst = 0.0
    for k in range(ncol):
        ind = (colour == k).astype(np.float64)
        Y = np.zeros(n, dtype=LD)
        np.add.at(Y, r, v.astype(LD) * ind[cc])
        R, S = cr.ch_action(CH, CH_SHIFT, U, ind)
        worst = max(worst, T.compare_entrywise((np.arange(n), Y), R, S, C_CURVED, cr.tref, "colour %d" % k))
    _report("state-pencil-geo-ch-ijacobian-nurbs", kn, worst)


def test_tangent_at_p3_is_refused_and_the_fallback_checked(monkeypatch):
    """Asked for by name, the walk refuses a Tangent on a mapped geometry at p = 3 (PETSC_ERR_SUP); the automatic choice takes the
    feature kernel, whose entries are checked."""
    import petiga_amd as P
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(REFUSED, True)
    eng.set_form("bratu", (LAM,))
    U, V = vectors("bratu", orc.global_size())
    r, cc, v = _tangent(eng, "ijacobian", U, V, SHIFT)
    kn = _names(eng, ("feature_assemble",))
    assert "state_pencil" not in kn, kn
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    J = cr.bratu_matrix(LAM, U, SHIFT)
    _report("feature-bratu-ijacobian-p3-nurbs", kn, T.compare_entrywise((r, cc, v), *J.at(r, cc), C_CURVED, cr.tref, "fallback"))
    eng.set_kernel(2)
    with pytest.raises(P.IGXError) as e:
        eng.compute_ijacobian(SHIFT, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), eng.create_mat())
    assert e.value.code == 56 and "p = 2 only" in str(e.value), str(e.value)


@pytest.mark.parametrize("name", list(VEC))
def test_vector_pass_row_by_row(name, monkeypatch):
    spec, form, driver = VEC[name]
    _env(monkeypatch, {})
    orc, eng, X, W, bcs = setup(spec, True)
    eng.set_form(form, {"poisson": (), "bratu": (LAM,), "cahnhilliard": CH}[form])
    n = orc.global_size()
    U, V = vectors(form, n)
    Uv, Vv, F = eng.create_vec().set(U), eng.create_vec().set(V), eng.create_vec().set(np.full(n, np.nan))      # the drivers zero F
    if driver == "vector":
        eng.compute_vector(F)
    elif driver == "function":
        eng.compute_function(Uv, F)
    else:
        eng.compute_ifunction(SHIFT if form == "bratu" else CH_SHIFT, Vv, 0.0, Uv, F)
    eng.synchronize()
    kn = _names(eng, ("vec_sumfact", "vector only"))
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    _report(name, kn, PW.compare_rows(F.get(), *vector_reference(cr, form, driver, U, V), C_CURVED, cr.tref, name))


class _Free:
    """One engine with its form set and the state on the device, and the case's reference (test_gpu_action_entrywise._Action)."""

    def __init__(self, name):
        spec, form, driver, self.lanes = FREE[name]
        self.orc, self.eng, X, W, bcs = setup(spec, True)
        eng = self.eng
        eng.set_form(form, {"poisson": (), "elasticity": EL, "bratu": (LAM,), "cahnhilliard": CH}[form])
        self.n, self.form, self.driver, self.p = self.orc.global_size(), form, driver, spec[0]["p"]
        self.U, self.V = vectors(form, self.n, seed=29)
        self.Uv, self.Vv, self.Xv, self.Y = (eng.create_vec() for _ in range(4))
        self.Uv.set(self.U)
        self.Vv.set(self.V)
        self.Y.set(np.full(self.n, np.nan))                 # the driver zeroes Y itself
        self.shift = CH_SHIFT if form == "cahnhilliard" else SHIFT
        self.cr = CR.CurvedRef(self.orc, X, W, bcs=bcs)
        self.matrix, self.action = free_reference(self.cr, form, driver, self.U)

    def __call__(self, X):
        eng = self.eng
        self.Xv.set(X)
        if self.driver == "matrix":
            eng.compute_matrix_action(self.Xv, self.Y)
        elif self.driver == "jacobian":
            eng.compute_jacobian_action(self.Uv, self.Xv, self.Y)
        else:
            eng.compute_ijacobian_action(self.shift, self.Vv, 0.0, self.Uv, self.Xv, self.Y)
        eng.synchronize()
        return self.Y.get().copy()

    def layout(self, kn):
        if self.lanes:
            assert "one workgroup per element" in kn and "%d x %d x %d lanes" % ((self.lanes,) * 3) in kn, kn
        else:
            assert ("two elements per wavefront" if self.p <= 2 else "one wavefront per element") in kn, kn
        return kn


@pytest.mark.parametrize("name", list(FREE))
def test_action_row_by_row(name):
    act = _Free(name)
    worst = {}
    for tag, X in (("X", np.random.default_rng(31).standard_normal(act.n)), ("Xwide", wide(act.n))):
        Y = act(X)
        kn = act.layout(_names(act.eng, ("vec_sumfact", "matrix action")))
        worst[tag] = PW.compare_rows(Y, *act.action(X), C_CURVED, act.cr.tref, "%s %s" % (name, tag))
    _report("action " + name, kn, "  ".join("%s %.2f" % kv for kv in worst.items()))


@pytest.mark.parametrize("name", PROBE)
def test_operator_recovered_from_the_action(name):
    """test_gpu_action_entrywise.test_operator_recovered_from_the_action on a curved map: one column per colour and row, a distinct
    amplitude on every probed column, every uncoupled row exactly 0.0."""
    act = _Free(name)
    ref, n = act.cr.tref, act.n
    rows = np.arange(n)
    cols, valid = ref.stencil(rows)
    rr, cc = np.nonzero(valid)
    er, ec = rows[rr], cols[rr, cc]
    R, S = act.matrix.at(er, ec)
    diag = ref.fixed(er)[0] & (er == ec)
    S[diag] = R[diag]                                    # a fixed row: m a_i, added once per element -- rounded, bound m |a_i|
    colour, ncol = colour_indicators(act.cr)
    rng = np.random.default_rng(17)
    amp = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    order = np.argsort(colour[ec], kind="stable")
    start = np.searchsorted(colour[ec][order], np.arange(ncol + 1))
    worst, probed = 0.0, 0
    for k in range(ncol):
        Y = act(np.where(colour == k, amp, 0.0))
        if k == 0:
            kn = act.layout(_names(act.eng, ("vec_sumfact", "matrix action")))
        e = order[start[k]:start[k + 1]]
        assert np.unique(er[e]).size == e.size         # no row couples with two columns of this colour
        a = amp[ec[e]]
        worst = max(worst, T.compare_entrywise((er[e], ec[e], Y[er[e]]), LD(1) * a * R[e], np.abs(a) * S[e], C_CURVED, ref,
                                               "%s colour %d" % (name, k), pattern=False))
        rest = np.ones(n, dtype=bool)
        rest[er[e]] = False
        bad = np.flatnonzero(rest & ~(Y == 0.0))
        assert bad.size == 0, "%s colour %d: row %d couples with no probed column and is %r" % (name, k, bad[0], Y[bad[0]])
        probed += e.size
    assert probed == er.size
    _report("probe " + name, kn, worst)


@pytest.mark.parametrize("name", DIAGONAL)
def test_diagonal_row_by_row(name):
    act = _Free(name)
    act.eng.compute_matrix_diagonal(act.Y)                  # (NaN-poisoned: the driver zeroes it)
    act.eng.synchronize()
    kn = act.layout(_names(act.eng, ("vec_sumfact", "matrix diagonal")))
    rows = np.arange(act.n)
    R, S = act.matrix.at(rows, rows)
    fx = act.cr.tref.fixed(rows)[0]
    assert fx.any() and np.all(S[fx] == 0) and np.all(S[~fx] > 0)
    _report("diagonal " + name, kn, T.compare_entrywise((rows, rows, act.Y.get()), R, S, C_CURVED, act.cr.tref, name, pattern=False))


def test_block_diagonal_entry_by_entry():
    from test_gpu_matrix_block_diagonal import host_blocks
    act = _Free(BLOCK)
    eng, dof = act.eng, act.cr.dof
    B = [eng.create_vec().set(np.full(act.n, np.nan)) for _ in range(dof)]      # (the driver zeroes the columns)
    eng.compute_matrix_block_diagonal(B)
    eng.synchronize()
    kn = act.layout(_names(eng, ("vec_sumfact", "matrix block diagonal")))
    node, i, j = np.meshgrid(np.arange(act.n // dof), np.arange(dof), np.arange(dof), indexing="ij")
    rows, cols = (node * dof + i).ravel(), (node * dof + j).ravel()
    R, S = act.matrix.at(rows, cols)
    fx = act.cr.tref.fixed(rows)[0] | act.cr.tref.fixed(cols)[0]
    assert fx.any() and np.all(S[fx] == 0) and np.all(S[~fx & (rows == cols)] > 0)
    _report("block diagonal " + BLOCK, kn, T.compare_entrywise((rows, cols, host_blocks(B, dof).ravel()), R, S, C_CURVED, act.cr.tref, BLOCK,
                                                                pattern=False))
