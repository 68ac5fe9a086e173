"""What IGXGetLastTiming reports after IGXSolve, IGXSolveNonlinear and IGXTimeStep (petiga_amd/csrc/solve_loops.hpp): the EXACT number of
launches of a call, counted from the loops as they are written, and whose figures the next call to last_timing() returns.  The operators'
own counts are measured in the same test from a direct driver call -- L_A for one action, L_F for one residual, L_D for one diagonal -- so
the counts hold on every space; the loops' own launches are the kernels of krylov.hpp, newton.hpp and timestep.hpp (copies and memsets on
the stream are not launches):
  CG, k >= 1 iterations        L_A + kr_resid0 + (kr_dot | kr_jacobi_rz) + kr_record, then per iteration L_A + kr_dot + kr_cg_update +
                               (kr_dot | kr_jacobi_rz) + kr_record, and kr_cg_p from the second iteration on: (k + 1) L_A + 3 + 4 k + (k - 1);
                               with Jacobi the diagonal driver's L_D once on top
  BiCGStab, k iterations       L_A + kr_resid0 + kr_dot + kr_record, then per iteration kr_bicg_p + L_A + (kr_dot, kr_bicg_s) + L_A +
                               (kr_dot2, kr_bicg_xr, kr_bicg_record): L_A + 3 + k (2 L_A + 6)
  Newton, basic line search    nw_state for an IFunction, L_F + kr_dot + kr_record, then per iteration kr_set + the inner solve's count +
                               nw_first_trial + L_F + 2
  IGXTimeStep, fixed steps     per attempt ts_stage + the Newton solve's count + ts_update + kr_record
Every test prints what it sees before it asserts (run with -s)."""
import numpy as np
import pytest

from test_gpu_newton import _bratu_pair
from test_gpu_timestep import _case as timestep_case

pytestmark = pytest.mark.gpu


def cg_count(L_A, k, L_D=0):
    assert k >= 1
    return L_D + (k + 1) * L_A + 3 + 4 * k + (k - 1)


def bicgstab_count(L_A, k):
    return L_A + 3 + k * (2 * L_A + 6)


def newton_count(L_F, inner_counts, ifunction):
    return (1 if ifunction else 0) + L_F + 2 + sum(1 + c + 1 + L_F + 2 for c in inner_counts)


def _launches(eng, call):
    call()
    return eng.last_timing()[2]


def _bratu():
    """Bratu p = 2 on 3 x 3 x 3 elements with a state, a right-hand side and the drivers' own counts (L_A of the Jacobian action, L_D of its
    diagonal, L_F of the Function)"""
    _, eng = _bratu_pair(2, (3, 3, 3), 3.5)
    n = eng.create_vec().n
    rng = np.random.default_rng(41)
    U, b, x, Y = eng.create_vec().set(0.3 * rng.standard_normal(n)), eng.create_vec().set(rng.standard_normal(n)), eng.create_vec(), eng.create_vec()
    L_A = _launches(eng, lambda: eng.compute_jacobian_action(U, b, Y))
    L_D = _launches(eng, lambda: eng.compute_jacobian_diagonal(U, Y))
    L_F = _launches(eng, lambda: eng.compute_function(U, Y))
    print("Bratu p = 2, 3 x 3 x 3 elements, n = %d: L_A = %d, L_D = %d, L_F = %d" % (n, L_A, L_D, L_F))
    assert L_A > 0 and L_D > 0 and L_F > 0
    return eng, U, b, x, Y, L_A, L_D, L_F


def _timed_figures_hold(eng, launches, driver):
    """With timing on, after a loop: last_timing() returns what the loop stored -- its launches, the whole call and the SUM of its operators'
    kernel times -- and not a reading of the engine's events, which hold the last driver call made inside the loop.  `driver` makes one
    call of that driver; the smallest of three such calls is the yardstick.  Every loop timed here makes five driver calls at the least (CG
    with Jacobi at three iterations: four actions and a diagonal; the Newton solve nine; the stepper hundreds), so its figures exceed
    twice one call's, and one call's own figures do not."""
    total, kernel, n = eng.last_timing()
    assert eng.last_timing() == (total, kernel, n)
    one = []
    for _ in range(3):
        driver()
        one.append(eng.last_timing()[:2])
    t1, k1 = min(t for t, _ in one), min(k for _, k in one)
    print("  timed: %.3f ms, operators %.3f ms, %d launches; one driver call %.3f ms, %.3f ms" % (total, kernel, n, t1, k1))
    assert n == launches and 0 < kernel <= total
    assert 0 < k1 <= t1 and kernel > 2 * k1 and total > 2 * t1


@pytest.mark.parametrize("k", [1, 3])
def test_krylov_launch_counts(k):
    eng, U, b, x, Y, L_A, L_D, _ = _bratu()
    for method, pc, want in (("cg", "none", cg_count(L_A, k)), ("cg", "jacobi", cg_count(L_A, k, L_D)), ("bicgstab", "none", bicgstab_count(L_A, k))):
        info = eng.solve(b, x.fill(0.0), method=method, op="jacobian", U=U, pc=pc, rtol=0.0, atol=0.0, maxit=k)
        launches, name = eng.last_timing()[2], eng.kernel_name()
        print("%s, pc %s, %d iterations (reason %s): %d launches, the count %d; %s" % (method, pc, info["iterations"], info["reason_name"], launches, want, name))
        assert info["iterations"] == k and info["reason_name"] == "diverged_its"
        assert launches == want
        assert name.startswith("krylov(%s, pc=%s, " % (method, pc)) and name.endswith(", %d iterations)" % k)


def test_newton_launch_count_and_whose_figures_last_timing_returns():
    eng, U, b, x, Y, L_A, L_D, L_F = _bratu()
    x0 = U.get().copy()
    kw = dict(method="cg", pc="none", lin_rtol=0.0, lin_maxit=2, rtol=0.0, maxit=2)
    info = eng.solve_nonlinear(x.set(x0), **kw)
    launches, name = eng.last_timing()[2], eng.kernel_name()
    want = newton_count(L_F, [cg_count(L_A, int(k)) for k in info["linear_its"]], ifunction=False)
    print("Newton (basic): %d iterations, inner %s, reason %s, %d backtracks: %d launches, the count %d; %s" % (
        info["iterations"], info["linear_its"], info["reason_name"], info["backtracks"], launches, want, name))
    assert info["iterations"] == 2 and list(info["linear_its"]) == [2, 2] and info["backtracks"] == 0 and info["function_evaluations"] == 3
    assert launches == want
    assert name.startswith("newton(basic, krylov(cg, pc=none, ") and name.endswith(", 2 iterations)")
    # a plain driver call after the solve: its figures
    assert _launches(eng, lambda: eng.compute_jacobian_action(U, b, Y)) == L_A and not eng.kernel_name().startswith("newton(")
    # with timing on: the solves' own figures, then the driver's, then -- after IGXSetUp and a new assembly -- the assembly's
    eng.set_timing(True)
    eng.solve(b, x.fill(0.0), method="cg", op="jacobian", U=U, pc="jacobi", rtol=0.0, atol=0.0, maxit=3)
    _timed_figures_hold(eng, cg_count(L_A, 3, L_D), lambda: eng.compute_jacobian_action(U, b, Y))
    eng.solve_nonlinear(x.set(x0), **kw)
    _timed_figures_hold(eng, want, lambda: eng.compute_function(U, Y))
    eng.compute_jacobian_action(U, b, Y)
    total, kernel, n = eng.last_timing()
    print("  the action after the solves: %.3f ms, %.3f ms, %d launches; %s" % (total, kernel, n, eng.kernel_name()))
    assert n == L_A and 0 < kernel <= total and not eng.kernel_name().startswith("newton(")
    eng.solve_nonlinear(x.set(x0), **kw)
    solve_name = eng.kernel_name()
    eng.setup()
    U2, Z = eng.create_vec().set(x0), eng.create_vec()
    eng.compute_function(U2, Z)
    total, kernel, n = eng.last_timing()
    print("  the residual's assembly after IGXSetUp: %.3f ms, %.3f ms, %d launches; %s" % (total, kernel, n, eng.kernel_name()))
    assert solve_name.startswith("newton(") and eng.kernel_name() != solve_name
    assert n == L_F and 0 < kernel <= total
    eng.set_timing(False)


def test_time_step_launch_count():
    eng, U0, V0, h, alpha, kw = timestep_case("ch-p2")
    assert kw["method"] == "bicgstab" and kw["pc"] == "none"
    U, V, X, Y = eng.create_vec().set(U0), eng.create_vec().set(V0), eng.create_vec().set(U0), eng.create_vec()
    L_A = _launches(eng, lambda: eng.compute_ijacobian_action(1e4, V, 0.0, U, X, Y))
    L_F = _launches(eng, lambda: eng.compute_ifunction(1e4, V, 0.0, U, Y))
    steps = 2

    def count(info):
        per_attempt = [newton_count(L_F, [], True) + int(r["newton_iterations"]) * (1 + bicgstab_count(L_A, 0) + 1 + L_F + 2) + int(r["linear_iterations"]) * (2 * L_A + 6) for r in info["log"]]
        return sum(1 + c + 2 for c in per_attempt)

    info = eng.time_step(U, V, h, alpha=alpha, max_steps=steps, **kw)
    launches, name = eng.last_timing()[2], eng.kernel_name()
    want = count(info)
    print("Cahn-Hilliard p = 2, n = %d: L_A = %d, L_F = %d; %d steps, %d attempts, per attempt (newton, inner) %s: %d launches, the count %d; %s" % (
        U0.size, L_A, L_F, info["steps"], info["attempts"], [(int(r["newton_iterations"]), int(r["linear_iterations"])) for r in info["log"]], launches, want, name))
    assert info["steps"] == steps == info["attempts"] and info["rejections"] == 0 and all(r["newton_reason"] > 0 for r in info["log"])
    assert launches == want
    assert name.startswith("timestep(") and ", newton(basic, krylov(bicgstab, pc=none, " in name and name.endswith(", %d steps, 0 rejections)" % steps)
    eng.set_timing(True)
    info = eng.time_step(U.set(U0), V.set(V0), h, alpha=alpha, max_steps=steps, **kw)
    _timed_figures_hold(eng, count(info), lambda: eng.compute_ifunction(1e4, V, 0.0, U, Y))
    eng.compute_ifunction(1e4, V, 0.0, U, Y)
    total, kernel, n = eng.last_timing()
    print("  the residual after the steps: %.3f ms, %.3f ms, %d launches; %s" % (total, kernel, n, eng.kernel_name()))
    assert n == L_F and 0 < kernel <= total and not eng.kernel_name().startswith("timestep(")
    eng.set_timing(False)
