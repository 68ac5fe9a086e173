"""The instantiations of one run-time struct side by side (petiga_amd/csrc/rtc.hpp): every kernel family the drivers route a struct to
keeps its compiled instantiations in the same RtcForm, so a call of one family must neither lose nor replace what another one built.

  families on one IGX   the user Poisson struct of test_rtc_forms.py through the pencil walk, vec_sumfact (Vector and its three matrix-free
                        modes), the feature kernel and the point-form kernel, twice round: the first round against the oracle at the
                        tolerance each family's own test uses (1e-12, 1e-11 on a mapped geometry), the second round against the first --
                        same kernel name and launch count call by call, the same bits where the kernel uses no atomics (vec_sumfact,
                        feature, point-form), the same tolerance for the pencil walk
  check, then run       IGXCheckFormSource(kind) leaves an entry that holds code but no module; the driver that follows on the same IGX
                        must launch the same kernel as often and compute the same as on an IGX that never ran the check
                        (form_pencil, vec_sumfact, state_pencil, block_pencil, band_pt at the smallest row of each family's own GPU test)"""
import numpy as np
import pytest

from common import compare_mats, make_pair, rel_err, warped_geometry
from test_gpu_matrix_action import _check as check_action, _products
from test_gpu_matrix_diagonal import _check as check_diagonal
from test_rtc_band_pt import DT, FX, NU, _problem, builtin_text_as_source
from test_rtc_boundary_scalar import BRATU3, BRATU3_WALK, ELASTICITY_BANDS
from test_rtc_forms import USER_POISSON, _dirichlet

pytestmark = pytest.mark.gpu


def _calls(eng, X, verify=None):
    """the seven calls of one round, each as (what, atomics, result arrays, kernel name, launches); verify(what, A, arrays) after each"""
    out = []
    A, b, Xv, Y = eng.create_mat(), eng.create_vec(), eng.create_vec().set(X), eng.create_vec()

    def done(what, fragment, atomics, arrays):
        eng.synchronize()
        assert fragment in eng.kernel_name(), (what, eng.kernel_name())
        out.append((what, atomics, [np.array(a) for a in arrays], eng.kernel_name(), eng.last_timing()[2]))
        print("%-15s %3d launches  %s" % (what, out[-1][4], out[-1][3]))
        assert out[-1][4] >= 1
        if verify:
            verify(what, A, out[-1][2])

    eng.set_kernel(0)
    eng.compute_system(A, b)
    done("system-pencil", "form_pencil<UserPoisson>", True, (A.host(True), b.get()))
    eng.compute_vector(b)
    done("vector", "vec_sumfact<UserPoisson>(hiprtc", False, (b.get(),))
    eng.set_kernel(3)
    eng.compute_system(A, b)
    done("system-feature", "feature_assemble<UserPoisson>", False, (A.host(True), b.get()))
    eng.set_kernel(1)
    eng.compute_system(A, b)
    done("system-point", "generic_assemble<UserPoisson>", False, (A.host(True), b.get()))
    eng.set_kernel(0)
    eng.compute_matrix_action(Xv, Y)
    done("action", "vec_sumfact<UserPoisson>(hiprtc", False, (Y.get(),))
    eng.compute_matrix_diagonal(Y)
    done("diagonal", "vec_sumfact<UserPoisson>(hiprtc", False, (Y.get(),))
    eng.compute_matrix_block_diagonal([Y])
    done("block-diagonal", "vec_sumfact<UserPoisson>(hiprtc", False, (Y.get(),))
    return out


@pytest.mark.parametrize("p,N,geo", [(2, (8, 6, 5), False), (3, (8, 4, 5), True)])
def test_families_side_by_side_on_one_igx(p, N, geo):
    orc, eng = make_pair(3, 1, p, list(N))
    if geo:
        Xg, Wg = warped_geometry(orc, 3, seed=sum(N), rational=True, amp=0.1)
        orc.set_geometry(Xg, Wg)
        eng.set_geometry(Xg, Wg)
    _dirichlet((orc, eng), "all")
    tol = 1e-11 if geo else 1e-12
    A_o, b_o = orc.compute_system("orc_form_poisson")
    M = A_o.scipy()
    orc.clear_boundary()
    _, b_free = orc.compute_system("orc_form_poisson")
    X = np.random.default_rng(31).standard_normal(orc.global_size())
    R, S, fixed, diag = _products(M, X)
    eng.set_form_source(USER_POISSON, "UserPoisson", (1.0,))

    def against_the_oracle(what, A, arrays):
        if what.startswith("system"):
            compare_mats(A, A_o, tol)
            assert np.abs(arrays[1] - b_o).max() <= tol * max(np.abs(b_o).max(), 1e-300)
        elif what == "vector":
            assert rel_err(arrays[0], b_free) < tol
        elif what == "action":
            check_action(arrays[0], X, R, S, fixed, diag, tol)
        else:
            check_diagonal(arrays[0], np.asarray(diag), fixed, 1, tol, what)

    first = _calls(eng, X, against_the_oracle)
    names = {c[0]: c[3] for c in first}
    assert "action" in names["action"] and "matrix diagonal" in names["diagonal"] and "block" in names["block-diagonal"], names
    second = _calls(eng, X)
    for (what, atomics, a1, n1, l1), (_, _, a2, n2, l2) in zip(first, second):
        assert n1 == n2 and l1 == l2, (what, n1, n2, l1, l2)
        for x, y in zip(a1, a2):
            if atomics:
                assert np.abs(x - y).max() <= tol * np.abs(x).max(), what
            else:
                assert np.array_equal(x, y), what


def _run_pencil(eng):
    _dirichlet((eng,), "all")
    eng.set_form_source(USER_POISSON, "UserPoisson", (1.0,))
    eng.set_kernel(2)
    A, b = eng.create_mat(), eng.create_vec()
    return (lambda: eng.check_form_source(True, 2)), (lambda: eng.compute_system(A, b)), (lambda: (A.host(True), b.get())), "form_pencil<UserPoisson>"


def _run_vecsf(eng):
    for d in range(3):
        eng.set_boundary_value(d, 1, 0, 0.1 * d)
    eng.set_form_source(BRATU3, "UserBratu3", (3.5,))
    U, F = eng.create_vec(), eng.create_vec()
    U.set(np.random.default_rng(8).standard_normal(U.n) * 0.3)
    return (lambda: eng.check_form_source(False, 3)), (lambda: eng.compute_function(U, F)), (lambda: (F.get(),)), "vec_sumfact<UserBratu3>(hiprtc"


def _run_state(eng):
    for d in range(3):
        eng.set_boundary_value(d, 0, 0, 0.2 * d)
    eng.set_form_source(BRATU3_WALK, "UserBratu3Walk", (3.5,))
    U, J = eng.create_vec(), eng.create_mat()
    U.set(np.random.default_rng(8).standard_normal(U.n) * 0.3)
    return (lambda: eng.check_form_source(True, 4)), (lambda: eng.compute_jacobian(U, J)), (lambda: (J.host(True),)), "state_pencil<UserBratu3Walk,hiprtc>"


def _run_block(eng):
    for f in range(3):
        eng.set_boundary_value(0, 0, f, 0.0)
    eng.set_boundary_value(0, 1, 0, 1.0)
    eng.set_form_source(ELASTICITY_BANDS, "UserElasticityBands", (1.5, 0.8))
    A, b = eng.create_mat(), eng.create_vec()
    return (lambda: eng.check_form_source(True, 5)), (lambda: eng.compute_system(A, b)), (lambda: (A.host(True), b.get())), "block_pencil<UserElasticityBands>(hiprtc"


def _run_band(eng):
    src, name = builtin_text_as_source()
    eng.set_form_source(src, name, (NU, FX, 0.0, 0.0, DT))
    U, V, J = eng.create_vec(), eng.create_vec(), eng.create_mat()
    rng = np.random.default_rng(31)
    U.set(rng.standard_normal(U.n) * 0.3)
    V.set(rng.standard_normal(V.n) * 0.1)
    return (lambda: eng.check_form_source(True, 6)), (lambda: eng.compute_ijacobian(2.0 / DT, V, 0.0, U, J)), (lambda: (J.host(True),)), "band_pt<%s>(hiprtc" % name


# family -> (the space of its own GPU test's smallest row, set-up, bit for bit, tolerance of that test)
FAMILIES = {"form_pencil": (lambda: make_pair(3, 1, 2, [8, 6, 5])[1], _run_pencil, False, 1e-12),
            "vec_sumfact": (lambda: make_pair(3, 1, 2, [5, 4, 6])[1], _run_vecsf, True, 1e-12),
            "state_pencil": (lambda: make_pair(3, 1, 2, [9, 4, 5])[1], _run_state, False, 1e-12),
            "block_pencil": (lambda: make_pair(3, 3, 3, [9, 4, 4])[1], _run_block, False, 1e-12),
            "band_pt": (lambda: _problem((8, 4, 4), (False, False, False), None, 3)[1], _run_band, False, 1e-11)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_check_first_then_run(family):
    space, setup, exact, tol = FAMILIES[family]
    seen = []
    for with_check in (False, True):
        eng = space()
        check, run, result, fragment = setup(eng)
        if with_check:
            check()
        run()
        eng.synchronize()
        assert fragment in eng.kernel_name(), eng.kernel_name()
        seen.append((eng.kernel_name(), eng.last_timing()[2], result()))
    (n0, l0, r0), (n1, l1, r1) = seen
    print("%s: %d launches  %s" % (family, l0, n0))
    assert n0 == n1 and l0 == l1 and l0 >= 1
    for x, y in zip(r0, r1):
        assert np.all(np.isfinite(x)) and np.abs(x).max() > 0
        if exact:
            assert np.array_equal(x, y)
        else:
            assert np.abs(x - y).max() <= tol * np.abs(x).max()
