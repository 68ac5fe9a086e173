"""The matrix-free actions and diagonals above four basis functions or points per axis, in IGXCheckFormSource (gram = 7 the ACTION,
gram = 8 the DIAGONAL instantiation of vec_sumfact for a run-time struct; hiprtc for gfx950: no GPU needed): the one-workgroup-per-
element instantiations (6 x 6 x 6 and 8 x 8 x 8 lanes) compile for the degrees and quadrature sizes set so far, and the call answers
IGX_ERR_SUP with the driver's own reason where the driver would refuse: nen or nqp above 8."""
import pytest

from common import make_pair, warped_geometry
from test_gpu_matrix_action import USER_DIFFUSION
from test_matrix_diagonal_abi import USER_BIHARMONIC


@pytest.mark.parametrize("gram", [7, 8])
@pytest.mark.parametrize("setup", ["p4-identity", "p6-rational", "p3-nqp5"])
def test_high_degree_instantiations_of_a_run_time_struct_compile(setup, gram):
    """vec_sumfact<UserDiffusion, GEO, 6 or 8, ACTION / DIAGONAL>: 6 lanes per axis at p = 4 and at p = 3 with five points, 8 at p = 6"""
    p, nqp, geo = {"p4-identity": (4, None, False), "p6-rational": (6, None, True), "p3-nqp5": (3, 5, False)}[setup]
    orc, g = make_pair(3, 1, p, [2, 2, 2], nqp=nqp)
    if geo:
        X, W = warped_geometry(orc, 3, seed=2, rational=True, amp=0.05)
        g.set_geometry(X, W)
    g.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
    g.check_form_source(True, gram)


@pytest.mark.parametrize("gram", [7, 8])
def test_more_than_eight_points_per_axis_is_refused_as_the_driver_refuses_it(gram):
    """p = 3 with nine points per axis: the driver refuses it, and so does the check, with the driver's words (before this kernel the
    check compiled the 4 x 4 x 4 instantiation and returned 0)"""
    import petiga_amd as P
    _, g = make_pair(3, 1, 3, [2, 2, 2], nqp=9)
    g.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
    with pytest.raises(P.IGXError) as e:
        g.check_form_source(True, gram)
    assert e.value.code == 56 and "nen <= 8" in str(e.value) and "nqp <= 8" in str(e.value), str(e.value)
    assert ("diagonal" in str(e.value)) or gram == 7


@pytest.mark.parametrize("gram", [7, 8])
def test_degree_8_is_refused(gram):
    """p = 8 (nen = 9) answers IGX_ERR_SUP (56).  The library as a whole stops at degree 7: IGXAxisSetDegree refuses 8 with "degree > 7
    not supported" before a form or a driver is reached, so that is the text seen here; a space that could hold nen = 9 would get the
    matrix-free drivers' own "nen <= 8" (matfree_refusal), which the nine-point case above reaches through nqp."""
    import petiga_amd as P
    with pytest.raises(P.IGXError) as e:
        g = P.IGX(3, 1)
        for i in range(3):
            g.axis_uniform(i, 8, 2)
        g.set_form_source(USER_DIFFUSION, "UserDiffusion", (0.7,))
        g.check_form_source(True, gram)
    assert e.value.code == 56 and ("nen <= 8" in str(e.value) or "degree > 7" in str(e.value)), str(e.value)


def test_second_order_struct_at_p4():
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 4, 2)
    g.set_form_source(USER_BIHARMONIC, "UserBiharmonic", ())
    g.check_form_source(True, 7)                    # (the action takes it)
    with pytest.raises(P.IGXError) as e:
        g.check_form_source(True, 8)
    assert "second-order" in str(e.value), str(e.value)
