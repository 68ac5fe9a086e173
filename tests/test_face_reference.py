"""The long double reference of the boundary-form passes (face_ref.py): its calibration on the CPU oracle, what it sees that the global
tolerances do not, and the divergence theorem on the reference alone.

CALIBRATION.  Every case of test_gpu_face_entrywise.py runs through the CPU oracle here, entry by entry and row by row with the pattern
check on.  The rule is the project's: the constant is measured, not chosen.  The oracle's worst ratio over all face cases is 2.34 u S (a
Dirichlet row m (U - v) of Bratu's Function; 1.28 on the rows of a linear form), within C_MAP / 4 = 64, the margin
test_gpu_curved_entrywise.py documents between oracle and kernels: face_ref.C_FACE is the EXISTING tensor_ref.C_MAP (256) and no new
constant is introduced.  The oracle's ratios (printed by the tests, lines starting CALIBRATION; u S):
    six faces                         six-p2-nurbs K 0.05 F 0.05;  six-p3-poly K 0.65 F 1.21;  six-p321-nurbs K 0.08 F 0.06;
                                      graded 1:100 without a geometry K 0.87 F 0.99
    each face alone (six cases)       K 0.03 to 0.05, F 0.06 to 0.09
    BoundaryIntegral (six cases)      poly K 0.30 to 0.46 F 0.13 to 0.23;  nurbs K 0.03 to 0.05 F 0.01 to 0.02
    one element along axis 0          K 0.03 F 0.09;   periodic axis 1 with five elements K 0.04 F 0.08
    mass, two fields, p = 3           K 0.74 F 0.27;   Poisson over a face K 0.03 F 0.11
    the point-form kernel's cases     p = 4 (125 functions) K 0.08 F 0.08;  p = 2 K 0.04 F 0.04
    run-time forms                    UserNitsche<3> K 0.04 F 0.02;  the face-only form K 0.17 F 0.02 (orc_form_nitsche_face: S holds face
                                      terms alone)
    Matrix / Vector                   K 0.46 F 1.28    (the oracle has no Matrix / Vector driver: its System without values)
    Bratu Function / Jacobian         F 2.34, J 0.03   (the oracle makes the face passes in these drivers too: no System stand-in)
    one rank of two                   the cut between the two visited faces K 0.06 F 0.11;  across the visited face K 0.03 F 0.20
    functionals                       volume 0.08, area 0.01, int x . n dS 0.003
The NURBS figures are smaller than the polynomial ones because S grows with the abs-sums of the weight function's derivatives
(curved_ref.py), not because the passes differ.

TEETH.  One perturbation of the reference at a time (face_ref's wrong=): the oracle fails the bound against each, on the matrix and on
the vector.  The same perturbations added to the oracle's own matrix are also measured against compare_mats at the tolerances of
test_boundary_forms.py (2e-11 of the largest free entry on a geometry, 1e-12 without one): at full strength none of the five passes it
(they are off by 0.03 to 0.85 of the largest free entry); scaled down as the far-band test of test_curved_reference.py does --
weights 1 +- 2e-9, dW / W dropped in the face pairs that are p apart along an in-face axis -- compare_mats accepts the matrix and the
entry-wise check rejects it.

DIVERGENCE.  Over all six faces sum int x . n dS = 3 V on the reference alone, within the summed bounds.  On the polynomial warp the
integrands have degree 5 per axis at p = 2 and the p + 1 point rule is exact.  On the NURBS warp they are rational and the rule is not
exact (at 3 points per axis the two sides differ by 1.2e-5, at 5 by 2.5e-8, at 7 by 3.6e-11: quadrature error, the same in the oracle), so
the identity is held at 9 points per axis, where that error (4e-14) is below the rounding bound (1.1e-12).
"""
import ctypes as C

import numpy as np
import pytest

import face_ref as FR
import pointwise_ref as PW
import tensor_ref as T
import test_gpu_face_entrywise as G
from common import compare_mats
from test_tensor_reference import _Shim

LD = T.LD
BIG = 2.0 ** 12          # the comparisons measure; the assertion is 4 * worst <= c, on every row and entry
LAM = G.LAM


def _calibrated(name, worst):
    print("CALIBRATION %-30s %s" % (name, "  ".join("%s %.3f" % kv for kv in worst.items())))
    for what, w in worst.items():
        assert 4 * w <= FR.C_FACE <= 2 ** 12, (name, what, w, FR.C_FACE)


def _oracle_system(orc, case):
    form = {"user_nitsche": "nitsche", "face_only": "nitsche_face"}.get(case["form"], case["form"])
    return orc.compute_system("orc_form_" + form, C.c_int(case["k"]))


def _linear_on_the_oracle(name, case, box=None):
    orc, _, X, W, bcs = G.setup(case, False, box=box)
    fr = G.reference(orc, X, W, bcs, case)
    K, F, FS = G.linear_reference(fr, case)
    Ao, bo = _oracle_system(orc, case)
    r, c, v = T.matrix_coo(Ao)
    _calibrated(name, {"K": T.compare_entrywise((r, c, v), *K.at(r, c), BIG, fr.tref if box is None else None, name + " K"),
                       "F": PW.compare_rows(np.asarray(bo), F, FS, BIG, fr.tref, name + " F")})
    return fr


# ---- calibration: every case of the GPU file on the CPU oracle
@pytest.mark.parametrize("name", list(G.CASES))
def test_face_cases_on_the_oracle(name):
    fr = _linear_on_the_oracle(name, G.CASES[name])
    assert len(fr.faces) == len(G.CASES[name]["faces"])


@pytest.mark.parametrize("axis,side", G.ALL)
def test_each_face_alone_on_the_oracle(axis, side):
    _linear_on_the_oracle("alone-%d%d" % (axis, side), G.ALONE[axis, side])


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("run", list(G.RANKS))
def test_rank_boxes_on_the_oracle(run, rank):
    fr = _linear_on_the_oracle("rank%d-%s" % (rank, run), G.RANKS[run], box=(2, rank))
    assert sorted(fr.faces) == ([(2, rank)] if run == "cut-axis" else [(0, 1)])


def test_bratu_with_a_visited_face_on_the_oracle():
    orc, _, X, W, bcs = G.setup(G.BRATU, False)
    fr = G.reference(orc, X, W, bcs, G.BRATU)
    U = G.state(orc.global_size())
    Fo = orc.compute_function("orc_form_bratu_function", C.c_double(LAM), U)
    r, c, v = T.matrix_coo(orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(LAM), U))
    _calibrated("bratu-face10-p2-nurbs", {"F": PW.compare_rows(np.asarray(Fo), *fr.bratu_function(LAM, U), BIG, fr.tref, "bratu F"),
                                          "J": T.compare_entrywise((r, c, v), *fr.bratu_jacobian(LAM, U).at(r, c), BIG, fr.tref, "bratu J")})
    # the face pass is there: without it the rows on the face are rejected
    bare = G.reference(orc, X, W, bcs, G.BRATU, faces=[])
    with pytest.raises(AssertionError, match="u S"):
        PW.compare_rows(np.asarray(Fo), *bare.bratu_function(LAM, U), FR.C_FACE, fr.tref)


def test_functionals_on_the_oracle():
    worst = {}
    for faces in [[f] for f in G.ALL] + [G.ALL]:
        orc, _, X, W, _ = G.setup(G.SCALAR, False, faces=faces)
        ref = G.scalar_references(G.reference(orc, X, W, None, G.SCALAR, faces=faces))
        So = orc.compute_scalar("orc_scalar_volume", 2, full=True)
        Sf = orc.compute_scalar("orc_scalar_flux", 2, full=True)
        for tag, val in (("volume", So[0]), ("area", So[1]), ("flux", Sf[0]), ("volume (flux)", Sf[1])):
            R, S = ref[tag.split(" ")[0]]
            worst[tag] = max(worst.get(tag, 0.0), float(abs(LD(val) - R) / (LD(T.U_RND) * S)))
    _calibrated("functionals", worst)


# ---- the divergence theorem on the reference alone
@pytest.mark.parametrize("geo,nqp", [("poly", None), ("nurbs", 9)])
def test_divergence_theorem_on_the_reference(geo, nqp):
    case = G._case(geo, 82, G.ALL, "volume", p=2, N=[4, 3, 5], nqp=nqp)
    orc, _, X, W, _ = G.setup(case, False)
    fr = G.reference(orc, X, W, None, case)
    assert len(fr.faces) == 6
    (f, fs), (v, vs) = fr.flux_of_x(), fr.volume()
    bound = LD(T.U_RND) * (fs + 3 * vs)
    print("divergence %-5s sum int x . n dS - 3 V = %.3g, summed bound %.3g (V = %.6f)" % (geo, float(f - 3 * v), float(bound), float(v)))
    assert abs(f - 3 * v) <= bound
    # the sign of one face, or one face's tangent pair, breaks it
    for wrong in ("normal", "detS"):
        bad = G.reference(orc, X, W, None, case, wrong=wrong)
        assert abs(bad.flux_of_x()[0] - 3 * v) > 1e6 * bound


# ---- teeth: the wrong kernels the global tolerances cannot be trusted with
TEETH = {"normal": G.ALONE[1, 0], "detS": G.ALONE[1, 0], "dW": G.ALONE[1, 0], "inward": G.ALONE[1, 0], "h": G.CASES["six-p2-graded100-nogeo"]}


def _rejected(E, R, S, ref):
    with pytest.raises(AssertionError, match="u S"):
        if len(E) == 3:
            T.compare_entrywise(E, R, S, FR.C_FACE, ref)
        else:
            PW.compare_rows(E, R, S, FR.C_FACE, ref)


@pytest.mark.parametrize("wrong", list(TEETH))
def test_teeth_perturbed_reference_rejects_the_oracle(wrong):
    """The normal from the next axis's tangent pair, detS of the neighbouring face point, h from the neighbouring element's L, dW / W
    dropped from the face's quotient rule, the face row's first derivative one knot span inward: the oracle is within the bound of the
    right reference and outside the bound of each wrong one, on the matrix and on the vector."""
    case = TEETH[wrong]
    orc, _, X, W, bcs = G.setup(case, False)
    fr, bad = G.reference(orc, X, W, bcs, case), G.reference(orc, X, W, bcs, case, wrong=wrong)
    Ao, bo = _oracle_system(orc, case)
    r, c, v = T.matrix_coo(Ao)
    (K, F, FS), (Kb, Fb, FSb) = G.linear_reference(fr, case), G.linear_reference(bad, case)
    R, S = K.at(r, c)
    T.compare_entrywise((r, c, v), R, S, FR.C_FACE, fr.tref)
    PW.compare_rows(np.asarray(bo), F, FS, FR.C_FACE, fr.tref)
    _rejected((r, c, v), *Kb.at(r, c), fr.tref)
    _rejected(np.asarray(bo), Fb, FSb, fr.tref)
    # the same error in a kernel (the oracle's own rounding plus the wrong term) against the global tolerance
    E = v + (Kb.at(r, c)[0] - R).astype(np.float64)
    tol = 2e-11 if case["geo"] else 1e-12
    try:
        seen = "passes compare_mats at %g (%.3g)" % (tol, compare_mats(_Shim(r, c, E), Ao, tol))
    except AssertionError as e:
        seen = "fails compare_mats at %g: %s" % (tol, e)
    print("teeth %-7s %d entries changed; %s" % (wrong, np.count_nonzero(E != v), seen))
    _rejected((r, c, E), R, S, fr.tref)


def test_teeth_far_face_pairs_pass_the_global_tolerance():
    """Weights that are nearly constant (1 +- 2e-9) and a face pass that drops dW / W only in the pairs that are p apart along an
    in-face axis: compare_mats at 2e-11 of the largest free entry accepts the matrix, the entry-wise check rejects it."""
    case = G.ALONE[1, 0]
    orc, _, X, W, bcs = G.setup(case, False)
    W = 1.0 + 2e-9 * (W - 1.0) / 0.2
    orc.set_geometry(X, W)
    fr, bad = G.reference(orc, X, W, bcs, case), G.reference(orc, X, W, bcs, case, wrong="dW")
    Ao = _oracle_system(orc, case)[0]
    r, c, v = T.matrix_coo(Ao)
    R, S = G.linear_reference(fr, case)[0].at(r, c)
    Rb = G.linear_reference(bad, case)[0].at(r, c)[0]
    far = (np.abs(fr.tref.split(r)[0][0] - fr.tref.split(c)[0][0]) == 2) & (S > 0)
    E = np.where(far, v + (Rb - R).astype(np.float64), v)
    assert np.count_nonzero(E != v) >= 20
    T.compare_entrywise((r, c, v), R, S, FR.C_FACE, fr.tref)
    print("far face pairs: %d entries changed, %.3g of the largest free entry" % (np.count_nonzero(E != v), compare_mats(_Shim(r, c, E), Ao, 2e-11)))
    _rejected((r, c, E), R, S, fr.tref)
