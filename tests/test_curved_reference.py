"""The long double reference on a general NURBS map (curved_ref.py): its reduction to the references that exist, its calibration on the
CPU oracle, and what it sees that an affine map and the global tolerances do not.

REDUCTION.  On an affine map, with unit weights and with constant weights 1.7, the curved R of every form equals the R of TensorRef /
PointwiseRef, and scaling all weights of a curved rational net by 1.7 leaves R unchanged, to long double rounding: C_ID / 16 / 64 u S
(the bound test_tensor_reference.py sets for the long double tables), with S the bound of the reference that exists (the smaller one:
the curved S is never below it).  The affine map and its net are chosen exactly representable (see A_EX): TensorRef inverts A in double
and a net A g + b rounded to double is another map, u away.

CALIBRATION.  Every (form, driver, discretisation, geometry) of test_gpu_curved_entrywise.py runs through the CPU oracle here; the
matrix-free references take the oracle's matrix times X.  The rule is the project's: 4 x the worst oracle ratio must stay within the
constant the GPU file uses, which is the EXISTING tensor_ref.C_MAP (256); no new constant is introduced.  det J >= 0.5 at every point
of every case.  Worst oracle ratios met here (printed by the tests; u S):
    assembly (System / Matrix of Poisson, Poisson_f, mass, elasticity, elasticity_f)   K 0.71 (elasticity p = 3, polynomial map), F 0.69 (reduced rule);
                                                                                       on NURBS maps K 0.48 (mass, two fields), 0.10 otherwise
    one rank of two (the box's rows)                                                   K 0.06
    Bratu Jacobian / IJacobian entries at a varying state                              0.33 (polynomial), 0.02 (NURBS), 0.04 at p = 3
    Cahn-Hilliard Tangent probed colour by colour, IFunction                           below 0.005
    Bratu Function / IFunction, Poisson Vector                                         2.50 (a Dirichlet row m (U - v)), 0.74
    the oracle's matrix times X row by row (X and the wide X)                          0.96 (a Dirichlet row m X); its entries 0.27
so 4 x 2.5 = 10 against c = 256.  The ratios are small because S carries the first-order sensitivity of the geometry chain to the
rounding of its interpolated sums: on these meshes that term is 10^2 (polynomial) to 10^4 (rational) times the plain absolute-value
bound, against which the oracle sits at 10 to 30 u S.  The teeth tests below show what the bound still rejects.
"""
import ctypes as C

import numpy as np
import pytest

import curved_ref as CR
import oracle_api as O
import pointwise_ref as PW
import tensor_ref as T
import test_gpu_curved_entrywise as G
from common import compare_mats, warped_geometry
from test_pointwise_reference import wide
from test_tensor_reference import _El, _Shim

LD = T.LD
BIG = 2.0 ** 12          # the comparisons measure; the assertion is 4 * worst <= c, on every row and entry
LDR = T.C_ID / 16 / 64   # long double rounding, in u S
LAM, SHIFT, CH_SHIFT, CH = G.LAM, G.SHIFT, G.CH_SHIFT, G.CH


def _calibrated(name, worst):
    print("CALIBRATION %-42s %s" % (name, "  ".join("%s %.2f" % kv for kv in worst.items())))
    for what, w in worst.items():
        assert 4 * w <= G.C_CURVED <= 2 ** 12, (name, what, w, G.C_CURVED)


def _curved(orc, X, W, bcs):
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    assert cr.detv.min() >= 0.5, float(cr.detv.min())
    return cr


def _oracle_system(orc, form, params):
    ctx = _El(*params) if form == "elasticity" else (C.c_double * 5)(*params) if form == "elasticity_f" else None
    return orc.compute_system("orc_form_" + {"user": "poisson"}.get(form, form), ctx)


def _oracle_tangent(orc, form, driver, U, V):
    if form == "cahnhilliard":
        return orc.compute_ijacobian("orc_form_ch_tangent", O.CahnHilliardCtx(*CH), CH_SHIFT, V, 0.0, U)
    if driver == "jacobian":
        return orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(LAM), U)
    return orc.compute_ijacobian("orc_form_bratu_ijacobian", C.c_double(LAM), SHIFT, V, 0.0, U)


# ---- calibration: every case of the GPU file on the CPU oracle
@pytest.mark.parametrize("name", list(G.ASM))
def test_assembly_cases_on_the_oracle(name):
    spec, form, params, driver = G.ASM[name][:4]
    orc, _, X, W, bcs = G.setup(spec, False, bcs=driver == "system")
    cr = _curved(orc, X, W, bcs)
    K, F, FS = G.linear_reference(cr, form, params, driver)
    Ao, bo = _oracle_system(orc, form, params)
    r, c, v = T.matrix_coo(Ao)
    worst = {"K": T.compare_entrywise((r, c, v), *K.at(r, c), BIG, cr.tref, name + " K")}
    if driver == "system":
        worst["F"] = PW.compare_rows(np.asarray(bo), F, FS, BIG, cr.tref, name + " F")
    _calibrated(name, worst)


@pytest.mark.parametrize("rank", [0, 1])
def test_rank_box_on_the_oracle(rank):
    orc, _, X, W, bcs = G.setup(G.RANKS, False, box=(2, rank))
    cr = _curved(orc, X, W, bcs)
    K = cr.linear(T.poisson(3), "system")[0]
    r, c, v = T.matrix_coo(orc.compute_system("orc_form_poisson")[0])
    _calibrated("rank %d" % rank, {"K": T.compare_entrywise((r, c, v), *K.at(r, c), BIG, None, "rank %d" % rank)})


@pytest.mark.parametrize("name", list(G.STATE) + ["refused-p3"])
def test_bratu_tangent_cases_on_the_oracle(name):
    spec, driver = G.STATE[name] if name in G.STATE else (G.REFUSED, "ijacobian")
    orc, _, X, W, bcs = G.setup(spec, False)
    cr = _curved(orc, X, W, bcs)
    U, V = G.vectors("bratu", orc.global_size())
    r, c, v = T.matrix_coo(_oracle_tangent(orc, "bratu", driver, U, V))
    J = cr.bratu_matrix(LAM, U, SHIFT if driver == "ijacobian" else 0.0)
    _calibrated(name, {"J": T.compare_entrywise((r, c, v), *J.at(r, c), BIG, cr.tref, name)})


def test_cahn_hilliard_probing_on_the_oracle():
    """The oracle's Tangent times every colour's indicator vector against ch_action on it: the reference of the GPU file's probing."""
    orc, _, X, W, bcs = G.setup(G.CH_TANGENT, False)
    cr = _curved(orc, X, W, bcs)
    n = orc.global_size()
    U, V = G.vectors("cahnhilliard", n)
    M = _oracle_tangent(orc, "cahnhilliard", "ijacobian", U, V).scipy()
    colour, ncol = G.colour_indicators(cr)
    worst = 0.0
    for k in range(ncol):
        ind = (colour == k).astype(np.float64)
        worst = max(worst, PW.compare_rows(M @ ind, *cr.ch_action(CH, CH_SHIFT, U, ind), BIG, cr.tref, "colour %d" % k))
    _calibrated("ch tangent probed, %d colours" % ncol, {"entries": worst})


@pytest.mark.parametrize("name", list(G.VEC))
def test_vector_cases_on_the_oracle(name):
    spec, form, driver = G.VEC[name]
    orc, _, X, W, bcs = G.setup(spec, False, bcs=driver != "vector")
    cr = _curved(orc, X, W, bcs)
    U, V = G.vectors(form, orc.global_size())
    if driver == "vector":
        Fo = orc.compute_system("orc_form_poisson")[1]
    elif form == "cahnhilliard":
        Fo = orc.compute_ifunction("orc_form_ch_residual", O.CahnHilliardCtx(*CH), CH_SHIFT, V, 0.0, U)
    elif driver == "function":
        Fo = orc.compute_function("orc_form_bratu_function", C.c_double(LAM), U)
    else:
        Fo = orc.compute_ifunction("orc_form_bratu_ifunction", C.c_double(LAM), SHIFT, V, 0.0, U)
    _calibrated(name, {"F": PW.compare_rows(np.asarray(Fo), *G.vector_reference(cr, form, driver, U, V), BIG, cr.tref, name)})


@pytest.mark.parametrize("name", list(G.FREE))
def test_matrix_free_cases_on_the_oracle(name):
    """The oracle's matrix times X (a standard-normal X and the wide one) row by row, and its entries where the GPU file recovers
    entries, diagonals or blocks."""
    spec, form, driver, _ = G.FREE[name]
    orc, _, X, W, bcs = G.setup(spec, False)
    cr = _curved(orc, X, W, bcs)
    n = orc.global_size()
    U, V = G.vectors(form, n, seed=29)
    if form in ("poisson", "elasticity"):
        Mo = _oracle_system(orc, form, G.EL if form == "elasticity" else ())[0]
    else:
        Mo = _oracle_tangent(orc, form, driver, U, V)
    matrix, action = G.free_reference(cr, form, driver, U)
    M = Mo.scipy()
    worst = {}
    for tag, Xv in (("X", np.random.default_rng(31).standard_normal(n)), ("Xwide", wide(n))):
        worst[tag] = PW.compare_rows(M @ Xv, *action(Xv), BIG, cr.tref, "%s %s" % (name, tag))
    if matrix is not None:
        r, c, v = T.matrix_coo(Mo)
        worst["entries"] = T.compare_entrywise((r, c, v), *matrix.at(r, c), BIG, cr.tref, name + " entries")
    _calibrated("free " + name, worst)


# ---- reduction to the references that exist
# TensorRef and PointwiseRef take the affine map's matrix A, invert it in double and know nothing of a control net; CurvedRef takes the
# net.  For the two to describe the SAME operator to long double rounding both inputs must be exact: A = L D U with dyadic unit-triangular
# L, U and D = diag(1, 2, 1) has an exactly representable inverse and determinant, and on meshes whose Greville points are dyadic
# (p = 2 with 2^k elements on [0, 1]; p = 3 with spans of 3/4 on [0, 3]) the net A g + b is exact in double.
A_EX = np.array([[1, 0, 0], [.5, 1, 0], [.25, .5, 1]]) @ np.diag([1.0, 2.0, 1.0]) @ np.array([[1, .5, .25], [0, 1, .5], [0, 0, 1]])
B_EX = np.array([0.5, -0.25, 0.125])
K3 = [np.r_[[0.0] * 4, 0.75, 1.5, 2.25, [3.0] * 4], np.r_[[0.0] * 4, 1.5, [3.0] * 4], np.r_[[0.0] * 4, 0.75, 1.5, [3.0] * 4]]
AFFINE = {"poisson": dict(dof=1, p=3, N=0, knots=K3, bcs=G._bcs(3)), "mass": dict(dof=2, p=2, N=[4, 2, 4], bcs=G._bcs(3, 2, "some")),
          "elasticity_f": dict(dof=3, p=2, N=[4, 4, 2], bcs=G.EL_BCS)}


def _exact_affine(kw, A=A_EX, b=B_EX):
    """(oracle, the net A g + b), both exact."""
    orc, _, _ = T.setup_case(dim=3, **kw)
    X = T.affine_geometry(orc, 3, A, b)
    g = np.linalg.solve(A, (X - b).T).T
    assert np.array_equal(np.linalg.inv(A) @ A, np.eye(3)) and np.array_equal(g.astype(LD) @ A.T.astype(LD) + b.astype(LD), X.astype(LD))
    return orc, X


def _same(tag, R, Rt, S, St):
    """|R - Rt| <= LDR u St entry by entry (St: the bound of the reference that exists), the same exact zeros, and S >= St."""
    R, Rt, S, St = (np.asarray(a, dtype=LD).ravel() for a in (R, Rt, S, St))
    assert np.array_equal(S == 0, St == 0), tag
    nz = St > 0
    assert np.all(R[~nz] == Rt[~nz]), tag
    ratio = float((np.abs(R - Rt)[nz] / (LD(T.U_RND) * St[nz])).max()) if nz.any() else 0.0
    assert ratio <= LDR, (tag, ratio)
    assert np.all(S >= St * (1 - LD(2.0) ** -40)), tag
    return ratio


@pytest.mark.parametrize("weights", [None, 1.7])
@pytest.mark.parametrize("name", list(AFFINE))
def test_affine_map_reduces_to_the_tensor_reference(name, weights):
    kw = AFFINE[name]
    orc, Xa = _exact_affine(kw)
    cr = CR.CurvedRef(orc, Xa, None if weights is None else np.full(len(Xa), weights), bcs=kw["bcs"])
    tf = {"poisson": T.poisson(3), "mass": T.mass(3, 2), "elasticity_f": T.elasticity(1.25, 0.75, [0.5, -1.0, 2.0])}[name]      # (dyadic Lame parameters: TensorRef contracts them with A^-1 in double)
    ref = T.reference(orc, 3, tf, A=A_EX, bcs=kw["bcs"], driver="system")
    K, F, FS = cr.linear(tf, "system")
    n = orc.global_size()
    rows = np.arange(n)
    cols, valid = ref.stencil(rows)
    rr, cc = np.nonzero(valid)
    er, ec = rows[rr], cols[rr, cc]
    Rt, St = ref.entries(er, ec)
    R, S = K.at(er, ec)
    wK = _same(name + " K", R, Rt, S, St)
    assert np.count_nonzero(K.S) == np.count_nonzero(S)      # nothing outside the pattern
    Rt, St = ref.vector(rows)
    print("affine %-14s weights %-4s |R - R_tensor|: K %.3g, F %.3g u S" % (name, weights, wK, _same(name + " F", F, Rt, FS, St)))


@pytest.mark.parametrize("weights", [None, 1.7])
def test_affine_map_reduces_to_the_pointwise_reference(weights):
    """Bratu (Function, IFunction, entries, actions) on an affine map; Cahn-Hilliard, which PointwiseRef has on the identity geometry
    only, on the Greville net."""
    kw = dict(dof=1, p=2, N=[4, 4, 2], bcs=G.BC3)
    orc, Xa = _exact_affine(kw)
    Wa = None if weights is None else np.full(len(Xa), weights)
    cr, pw = CR.CurvedRef(orc, Xa, Wa, bcs=kw["bcs"]), PW.PointwiseRef(orc, A=A_EX, bcs=kw["bcs"])
    n = orc.global_size()
    U, V = G.vectors("bratu", n)
    Xv = wide(n)
    worst = {}
    for tag, a, b in (("F", cr.bratu_function(LAM, U), pw.bratu_function(LAM, U)), ("IF", cr.bratu_function(LAM, U, V), pw.bratu_function(LAM, U, V)),
                      ("J X", cr.bratu_action(LAM, U, Xv), pw.bratu_action(LAM, U, Xv)),
                      ("IJ X", cr.bratu_action(LAM, U, Xv, SHIFT), pw.bratu_action(LAM, U, Xv, SHIFT))):
        worst[tag] = _same(tag, a[0], b[0], a[1], b[1])
    r, c, _ = T.matrix_coo(orc.create_mat())
    R, S = cr.bratu_matrix(LAM, U, SHIFT).at(r, c)
    Rt, St = pw.bratu_entries(LAM, U, r, c, SHIFT)
    worst["IJ"] = _same("IJ", R, Rt, S, St)
    # Cahn-Hilliard on the identity map given as a geometry
    kw = dict(dof=1, p=2, N=[4, 4, 2], bcs=G.BC_CH)
    orc, Xi = _exact_affine(kw, np.eye(3), np.zeros(3))
    cr, pw = CR.CurvedRef(orc, Xi, Wa, bcs=G.BC_CH), PW.PointwiseRef(orc, bcs=G.BC_CH)
    U, V = G.vectors("cahnhilliard", n)
    for tag, a, b in (("CH IF", cr.ch_ifunction(CH, U, V), pw.ch_ifunction(CH, U, V)),
                      ("CH T X", cr.ch_action(CH, CH_SHIFT, U, Xv), pw.ch_action(CH, CH_SHIFT, U, Xv))):
        worst[tag] = _same(tag, a[0], b[0], a[1], b[1])
    print("affine, weights %-4s |R - R_pointwise| (u S): %s" % (weights, "  ".join("%s %.3g" % kv for kv in worst.items())))


def test_scaling_the_weights_leaves_the_reference_unchanged():
    """A curved rational net with all weights times 1.7: the same basis, the same map."""
    orc, _, X, W, bcs = G.setup(G._spec("nurbs", 31, p=2, N=[5, 4, 3], bcs=G.BC_CH), False)
    a, b = CR.CurvedRef(orc, X, W, bcs=bcs), CR.CurvedRef(orc, X, 1.7 * W, bcs=bcs)
    n = orc.global_size()
    U, V = G.vectors("cahnhilliard", n)
    Xv = wide(n)
    worst = {}
    for tag, f in (("Poisson K", lambda r: (lambda K: (K.R, K.S))(r.linear(T.poisson(3))[0])), ("Poisson F", lambda r: r.linear(T.poisson_f(3))[1:]),
                   ("Bratu IF", lambda r: r.bratu_function(LAM, U - 0.4, V)), ("CH IF", lambda r: r.ch_ifunction(CH, U, V)),
                   ("CH T X", lambda r: r.ch_action(CH, CH_SHIFT, U, Xv))):
        (Ra, Sa), (Rb, Sb) = f(a), f(b)
        nz = Sa > 0
        assert np.array_equal(nz, Sb > 0) and np.all(Ra[~nz] == Rb[~nz])
        worst[tag] = float((np.abs(Ra - Rb)[nz] / (LD(T.U_RND) * Sa[nz])).max())
        assert worst[tag] <= LDR, (tag, worst[tag])
    print("weights x 1.7, |R - R'| (u S): %s" % "  ".join("%s %.3g" % kv for kv in worst.items()))


# ---- teeth: the wrong kernels an affine map hides
TEETH = G._spec("nurbs", 33, p=3, N=[5, 3, 3], bcs=G.BC3)
TEETH_CH = G._spec("nurbs", 34, p=2, N=[5, 4, 3], bcs=G.BC_CH)


def _rejected(E, R, S, ref):
    with pytest.raises(AssertionError, match="u S"):
        if len(E) == 3:
            T.compare_entrywise(E, R, S, G.C_CURVED, ref)
        else:
            PW.compare_rows(E, R, S, G.C_CURVED, ref)


def _affine_twin(spec, wrong, weights):
    """(right, wrong) references of the spec's discretisation on an AFFINE map with constant weights."""
    orc, _, _, _, bcs = G.setup(spec, False)
    Xa = T.affine_geometry(orc, 3, *T.affine_map(3, 2))
    Wa = np.full(len(Xa), weights)
    return CR.CurvedRef(orc, Xa, Wa, bcs=bcs), CR.CurvedRef(orc, Xa, Wa, bcs=bcs, wrong=wrong)


@pytest.mark.parametrize("wrong", ["point", "element", "dW", "net"])
def test_teeth_poisson_matrix(wrong):
    """The metric of the neighbouring point along axis 0; one element's metric used for the element after it; dW / W dropped; the
    control net read one node off along axis 0: each passes on an affine map (the last on a uniform Greville net without the offset
    b: a translation) and is rejected, entry by entry, on the curved one."""
    orc, _, X, W, bcs = G.setup(TEETH, False)
    cr = CR.CurvedRef(orc, X, W, bcs=bcs)
    K, F, FS = cr.linear(T.poisson(3))
    r, c, _ = T.matrix_coo(orc.create_mat())
    R, S = K.at(r, c)
    T.compare_entrywise((r, c, R.astype(np.float64)), R, S, G.C_CURVED, cr.tref)
    if wrong == "net":
        n = cr.n
        Xg, Wg = X.reshape(n[2], n[1], n[0], 3), W.reshape(n[2], n[1], n[0])
        Xs = np.concatenate([Xg[:, :, 1:], 2 * Xg[:, :, -1:] - Xg[:, :, -2:-1]], axis=2)       # node i0 reads node i0 + 1 (the last one continued)
        Ws = np.concatenate([Wg[:, :, 1:], Wg[:, :, -1:]], axis=2)
        bad = CR.CurvedRef(orc, Xs.reshape(-1, 3), Ws.reshape(-1), bcs=bcs)
        assert bad.detv.min() > 0.25
    else:
        bad = CR.CurvedRef(orc, X, W, bcs=bcs, wrong=wrong)
        # ... which an affine map with constant weights does not see
        right_a, wrong_a = _affine_twin(TEETH, wrong, 1.7)
        T.compare_entrywise((r, c, wrong_a.linear(T.poisson(3))[0].at(r, c)[0].astype(np.float64)), *right_a.linear(T.poisson(3))[0].at(r, c),
                            G.C_CURVED, right_a.tref)
    Kb, Fb, _ = bad.linear(T.poisson(3))
    _rejected((r, c, Kb.at(r, c)[0].astype(np.float64)), R, S, cr.tref)
    _rejected(Fb.astype(np.float64), F, FS, cr.tref)


def test_teeth_far_band_passes_the_global_tolerance():
    """A net whose weights are nearly constant (1 +- 2e-9) and a kernel that drops dW / W in the far-band pairs alone (|i0 - j0| = p):
    compare_mats at 1e-11 of the largest free entry against the oracle accepts its matrix, the entry-wise check rejects it."""
    orc, _, X, W, bcs = G.setup(TEETH, False)
    W = 1.0 + 2e-9 * (W - 1.0) / 0.2
    orc.set_geometry(X, W)
    cr, bad = CR.CurvedRef(orc, X, W, bcs=bcs), CR.CurvedRef(orc, X, W, bcs=bcs, wrong="dW")
    Ao = orc.compute_system("orc_form_poisson")[0]
    r, c, v = T.matrix_coo(Ao)
    R, S = cr.linear(T.poisson(3))[0].at(r, c)
    Rb = bad.linear(T.poisson(3))[0].at(r, c)[0]
    far = (np.abs(cr.tref.split(r)[0][0] - cr.tref.split(c)[0][0]) == 3) & (S > 0)
    E = np.where(far, v + (Rb - R).astype(np.float64), v)                        # the oracle's own rounding plus the wrong term
    assert far.sum() >= 100 and np.count_nonzero(E != v) >= far.sum() // 2
    T.compare_entrywise((r, c, v), R, S, G.C_CURVED, cr.tref)
    print("far-band mutation: %d entries, %.3g of the largest free entry (the oracle itself %.3g)"
          % (far.sum(), compare_mats(_Shim(r, c, E), Ao, 1e-11), compare_mats(_Shim(r, c, v), Ao, 1e-11)))
    _rejected((r, c, E), R, S, cr.tref)


@pytest.mark.parametrize("wrong", ["hess", "dW"])
def test_teeth_cahn_hilliard_rows(wrong):
    """The map's second derivatives dropped from the physical Laplacian (and dW / W from the quotient rule) in the Cahn-Hilliard rows."""
    orc, _, X, W, bcs = G.setup(TEETH_CH, False)
    cr, bad = CR.CurvedRef(orc, X, W, bcs=bcs), CR.CurvedRef(orc, X, W, bcs=bcs, wrong=wrong)
    right_a, wrong_a = _affine_twin(TEETH_CH, wrong, 1.7)
    n = orc.global_size()
    U, V = G.vectors("cahnhilliard", n)
    Xv = np.random.default_rng(3).standard_normal(n)
    for f in (lambda r: r.ch_ifunction(CH, U, V), lambda r: r.ch_action(CH, CH_SHIFT, U, Xv)):
        R, S = f(cr)
        PW.compare_rows(R.astype(np.float64), R, S, G.C_CURVED, cr.tref)
        PW.compare_rows(f(wrong_a)[0].astype(np.float64), *f(right_a), G.C_CURVED, right_a.tref)      # invisible on the affine map
        _rejected(f(bad)[0].astype(np.float64), R, S, cr.tref)
