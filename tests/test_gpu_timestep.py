"""IGXTimeStep on the GPU (include/petiga_amd.h; petiga_amd/csrc/timestep.hpp): the generalized-alpha time loop on the device-resident
Newton solve.  The yardstick of every run is the loop of tests/timestep_ref.py on the SAME engine's IGXSolveNonlinear (one host copy each
way per stage).  The Newton solve is bit-repeatable and the host forms W, U1 and V1 with one rounding per operation as the two sweeps do,
so the device's U and V are the host loop's BIT FOR BIT; unorm and wlte differ by the summation order alone and are held to
krylov_ref.norm_bound / krylov_ref.gamma of the exactly rounded values.  In an adaptive run the restatement is fed the device's wlte of
each attempt (it checks it against its own and takes the decision from it with the same host formula), so the dt sequence stays the
device's and the vectors can be compared bit for bit to the end.  The physics is held against the CPU oracle: the mass of Cahn-Hilliard
through the oracle's Mass matrix, Bratu's backward-Euler steps against the restatement on the oracle's IFunction with direct solves.
Every test prints what it sees before it asserts (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import krylov_ref as K
import newton_ref as N
import timestep_ref as T
from common import make_pair
from test_gpu_matrix_action import CASES, CH, DT, NS
from test_gpu_matrix_action import _pair as action_pair
from test_gpu_matrix_action import _reference as action_reference
from test_gpu_newton import _bratu_pair

pytestmark = pytest.mark.gpu

RHO = T.alphas(0.5)
BRATU_NEWTON = dict(method="bicgstab", pc="jacobi", lin_rtol=1e-8, lin_maxit=400, rtol=1e-10, maxit=12)


def _device(eng, U0, V0, dt, alpha=RHO, **kw):
    U, V = eng.create_vec().set(U0), eng.create_vec().set(V0)
    info = eng.time_step(U, V, dt, alpha=alpha, **kw)
    return U.get().copy(), V.get().copy(), info


STEPPER_KEYS = ("max_time", "max_steps", "t0", "adapt", "adapt_rtol", "adapt_atol", "dt_min", "dt_max", "max_rejections")


def _host(eng, U0, V0, dt, alpha=RHO, prev=None, device_wlte=None, **kw):
    """the host loop on the engine's Newton solve"""
    stepper = {k: kw.pop(k) for k in STEPPER_KEYS if k in kw}
    return T.integrate(T.engine_callables(eng, **kw), U0, V0, dt, alpha=alpha, prev=prev, device_wlte=device_wlte, **stepper)


def _host_chain(eng, U0, V0, h, steps, alpha=RHO, **kw):
    """the host loop one step at a time, each continuing the one before (t0, prev): [(U_k, V_k, the run's info up to step k)], k = 1 .. steps.
    With fixed steps that is one long run bit for bit, at the cost of `steps` stages."""
    out, U, V, t, prev, merged = [], U0, V0, 0.0, None, None
    for _ in range(steps):
        U, V, ref = _host(eng, U, V, h, alpha=alpha, max_steps=1, t0=t, prev=prev, **kw)
        t, prev = ref["t"], ref["prev"]
        if merged is None:
            merged = dict(ref)
        else:
            merged = dict(ref, log=merged["log"] + ref["log"], **{k: merged[k] + ref[k] for k in ("steps", "rejections", "attempts", "newton_iterations", "linear_iterations", "function_evaluations")})
        out.append((U, V, merged))
    return out


def _same_log(info, ref, wlte_bound=None):
    """the device's log against the restatement's: decisions, steps and the Newton counts equal; wlte within the bound of the host's own"""
    log, rlog = info["log"], ref["log"]
    assert len(log) == len(rlog) == info["attempts"] == ref["attempts"], (len(log), len(rlog))
    for d, r in zip(log, rlog):
        for key in ("t", "dt", "accepted", "newton_iterations", "newton_reason", "linear_iterations"):
            assert d[key] == r[key], (key, d, r)
        if r["host_wlte"] < 0:
            assert d["wlte"] == -1.0
        else:
            assert abs(d["wlte"] - r["host_wlte"]) <= K.gamma(wlte_bound) * r["host_wlte"], (d["wlte"], r["host_wlte"])
    for key in ("steps", "reason", "rejections", "newton_iterations", "linear_iterations", "function_evaluations", "t", "dt_last", "dt_next"):
        assert info[key] == ref[key], (key, info[key], ref[key])


def _unorm_holds(info, U):
    root = np.sqrt(K.exact_dot(U, U)[0])
    assert abs(info["unorm"] - root) <= K.norm_bound(U.size, root), (info["unorm"], root)


def _pinned(eng, x0, a=50.0, **newton_kw):
    """a state that holds the Dirichlet values and a derivative that goes with it: one backward-Euler stage of the device's Newton solve from
    x0 (U = the stage solution, V = a (U - x0))"""
    x = eng.create_vec().set(x0)
    info = eng.solve_nonlinear(x, op="ijacobian", a=a, W=eng.create_vec().set(-a * x0), **newton_kw)
    assert info["reason"] > 0, info
    U = x.get().copy()
    return U, a * (U - x0)


# ---- 1. the host loop on the same engine, bit for bit
def _case(name):
    """(engine, U0, V0, h, alpha, Newton keywords); the Cahn-Hilliard and NS-VMS states are those of tests/test_gpu_matrix_action.py with the
    Dirichlet rows pinned by one stage solve, h makes the stage's shift the a the Newton tests run at"""
    if name.startswith("bratu"):
        _, eng = _bratu_pair(2, (5, 4, 3), 3.5)
        U0, V0 = _pinned(eng, 0.3 * np.random.default_rng(29).standard_normal(eng.create_vec().n), **BRATU_NEWTON)
        alpha = T.BACKWARD_EULER if name.endswith("+be") else RHO
        return eng, U0, V0, 0.02, alpha, dict(BRATU_NEWTON)
    case = name.split("+")[0]
    _, eng = action_pair(case)
    form = CASES[case][0]
    eng.set_form(form, {"cahnhilliard": CH, "nsvms": NS}[form])
    ref = action_reference(case)
    U, V, fixed = np.array(ref[1]), np.array(ref[2]), ref[5]
    if form == "nsvms":
        alpha, a = T.BACKWARD_EULER, 2.0 / DT
        kw = dict(method="bicgstab", pc="pbjacobi", lin_rtol=1e-6, lin_maxit=300, rtol=1e-6, maxit=12)
        V0 = np.where(fixed, 0.0, V)
    else:
        alpha, a = RHO, 1e4
        kw = dict(method="bicgstab", pc="none", forcing="ew2", lin_rtol=1e-6, lin_maxit=300, rtol=1e-8, maxit=12)
        V0 = np.zeros_like(U)
    h = alpha[0] / (alpha[1] * alpha[2] * a)
    x, _ = _pinned(eng, U, a=a, **kw)
    return eng, np.where(fixed, x, U), V0, h, alpha, kw


@pytest.mark.parametrize("name", ["bratu-p2", "bratu-p2+be", "ch-p2", "ch-p2-dirichlet", "nsvms-p2"])
def test_states_are_the_host_loops_bit_for_bit(name):
    eng, U0, V0, h, alpha, kw = _case(name)
    chain = _host_chain(eng, U0, V0, h, 4, alpha=alpha, **kw)
    Ur, Vr, ref = chain[-1]
    print("%s: alpha %s, h %.4g; host loop %d steps, reason %d, per attempt (newton iterations, reason, inner) %s" % (
        name, alpha, h, ref["steps"], ref["reason"], [(r["newton_iterations"], r["newton_reason"], r["linear_iterations"]) for r in ref["log"]]))
    assert ref["steps"] == 4 and ref["reason"] == T.CONVERGED_STEPS and all(r["newton_reason"] > 0 for r in ref["log"])
    assert not np.array_equal(Ur, U0) and not np.array_equal(Vr, V0)
    for steps in (1, 2, 3, 4):
        U, V, info = _device(eng, U0, V0, h, alpha=alpha, max_steps=steps, **kw)
        print("  %d step(s): reason %d, t %.17g, unorm %.17g; %s" % (steps, info["reason"], info["t"], info["unorm"], eng.kernel_name()))
        Uk, Vk, refk = chain[steps - 1]
        assert np.array_equal(U, Uk), "U after %d steps is not the host loop's" % steps
        assert np.array_equal(V, Vk), "V after %d steps is not the host loop's" % steps
        _same_log(info, refk)
        _unorm_holds(info, U)
        assert all(r["wlte"] == -1.0 and r["accepted"] == 1 for r in info["log"])


# ---- 2. the sweeps past one workgroup and at odd lengths
@pytest.mark.parametrize("n,p,Nel", [(175, 2, (5, 3, 3)), (1025, 2, (3, 3, 39)), (1331, 3, (8, 8, 8)), (274625, 2, (63, 63, 63))])
def test_sweep_lengths(n, p, Nel):
    """the lengths tests/test_gpu_krylov_lengths.py derives: the tail, a full workgroup 0, a second workgroup, a second trip of the grid-stride
    loop with all 256 partials non-zero.  Two steps with adapt = 1 and loose tolerances: both are accepted, the second runs
    ts_update<true> with Uprev.  U_0 is random, so the Dirichlet rows (the last entry is a corner) move in the first step too."""
    _, eng = _bratu_pair(p, Nel, 3.5)
    assert eng.create_vec().n == n and n % 2 == 1
    rng = np.random.default_rng(n)
    U0, V0 = 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    kw = dict(method="bicgstab", pc="jacobi", lin_rtol=1e-6, lin_maxit=400, rtol=1e-6, maxit=12)
    run = dict(max_steps=2, adapt=True, adapt_rtol=1e3, adapt_atol=1e3, dt_max=0.0375)
    h = 0.0375                       # a = 50
    U, V, info = _device(eng, U0, V0, h, **run, **kw)
    U2, V2, info2 = _device(eng, U0, V0, h, **run, **kw)
    Ur, Vr, ref = _host(eng, U0, V0, h, device_wlte=info["log"]["wlte"], **run, **kw)
    print("n = %d: %d steps, reason %d, log %s; host wlte %s" % (n, info["steps"], info["reason"], info["log"], [r["host_wlte"] for r in ref["log"]]))
    assert info["steps"] == 2 and info["attempts"] == 2 and info["rejections"] == 0
    assert info["log"]["wlte"][0] == -1.0 and 0.0 < info["log"]["wlte"][1] < 1.0
    assert np.array_equal(U, Ur) and np.array_equal(V, Vr)
    _same_log(info, ref, wlte_bound=n)
    _unorm_holds(info, U)
    far = n - 1 if n < 262144 else 262144 + 4097
    for at in (n - 1, far):
        assert U[at] != U0[at] and V[at] != V0[at], at
    assert np.array_equal(U, U2) and np.array_equal(V, V2) and info["log"].tobytes() == info2["log"].tobytes() and info["unorm"] == info2["unorm"], "two runs differ"


# ---- 3. an adaptive run
# Bratu as an IFunction beyond the fold (lambda = 20: no steady state, the solution accelerates towards its blow-up near t = 0.058), from the
# harmonic extension of the Dirichlet values with its own derivative.  Found with the restatement on the CPU oracle (direct and BiCGStab
# stage solves give the same sequence): from dt0 = 1e-5 the step grows 1e-5, 1e-5, 1e-4, 1e-3 (twice by the cap of 10), then with
# wlte near 0.56 up to 7.1e-3 at t = 0.033; from t = 0.040 on Newton with maxit = 3 and rtol = 1e-10 fails at the proposed step
# (IGX_NEWTON_DIVERGED_MAX_IT at 6.5e-3, 3.7e-3, 3.0e-3, 2.0e-3) and the estimate rejects (wlte 1.44 at 5.5e-3, 1.07 at 4.2e-3, 1.10 at
# 2.3e-3 later on); max_time = 0.0505 cuts the last step (proposed 3.0e-3) to 3.3e-4.  24 attempts, 2 failures and 2 rejections by the
# estimate among them; no wlte closer to 1 than 0.955 and 1.07.  On an MI355X the device and the host loop on the engine take the same
# sequence as the oracle.
ADAPTIVE = dict(p=2, N=(5, 4, 3), lam=20.0, dt=1e-5, max_time=0.0505, max_steps=40, adapt=True, adapt_rtol=3e-3, adapt_atol=3e-3, max_rejections=6)
ADAPTIVE_NEWTON = dict(method="bicgstab", pc="jacobi", lin_rtol=1e-8, lin_maxit=400, rtol=1e-10, maxit=3)


@functools.lru_cache(maxsize=None)
def _adaptive_state():
    """(U0, V0): the harmonic extension of the Dirichlet values (Bratu with lambda = 0 is linear) and V0 = -M^-1 F(U0) on the free rows, on the oracle"""
    import scipy.sparse.linalg as spla
    c = ADAPTIVE
    orc, _ = _bratu_pair(c["p"], c["N"], c["lam"], engine=False)
    n = orc.global_size()
    fun, lin = N.oracle_callables(orc, "orc_form_bratu_function", "orc_form_bratu_jacobian", C.c_double(0.0))
    U0, _ = N.newton(fun, lin, np.zeros(n), rtol=1e-12, maxit=3)
    F = orc.compute_function("orc_form_bratu_function", C.c_double(c["lam"]), U0)
    M = orc.compute_system("orc_form_mass")[0].scipy().tocsr()
    off = abs(M)
    off.setdiag(0.0)
    free = np.asarray(off.sum(axis=1)).ravel() != 0.0
    V0 = np.zeros(n)
    V0[free] = spla.spsolve(M[free][:, free].tocsc(), -F[free])
    for a in (U0, V0):
        a.setflags(write=False)
    return U0, V0


def _adaptive_engine():
    c = ADAPTIVE
    _, eng = _bratu_pair(c["p"], c["N"], c["lam"])
    return eng, {k: c[k] for k in ("max_time", "max_steps", "adapt", "adapt_rtol", "adapt_atol", "max_rejections")}


def test_adaptive_run_follows_the_host_loop():
    U0, V0 = _adaptive_state()
    eng, run = _adaptive_engine()
    n, dt0 = U0.size, ADAPTIVE["dt"]
    U, V, info = _device(eng, U0, V0, dt0, **run, **ADAPTIVE_NEWTON)
    Ur, Vr, ref = _host(eng, U0, V0, dt0, device_wlte=info["log"]["wlte"], **run, **ADAPTIVE_NEWTON)
    kinds = "".join("+" if r["accepted"] else ("N" if r["newton_reason"] < 0 else "E") for r in ref["log"])
    print("adaptive: %d steps, %d attempts, %d rejections, reason %d, t %.17g, dt_next %.6e; attempts %s" % (info["steps"], info["attempts"], info["rejections"], info["reason"], info["t"], info["dt_next"], kinds))
    for d, r in zip(info["log"], ref["log"]):
        print("   t %.6e dt %.6e wlte %.17g (host %.17g) accepted %d newton (%d, %d, %d)" % (d["t"], d["dt"], d["wlte"], r["host_wlte"], d["accepted"], d["newton_iterations"], d["newton_reason"], d["linear_iterations"]))
    # the condition: no attempt of the case is decided within the bound of 1 (host_wlte is the host loop's own value on vectors that are the
    # device's bit for bit, so the host loop left to itself takes every decision the same way)
    for r in ref["log"]:
        if r["host_wlte"] >= 0:
            assert abs(r["host_wlte"] - 1.0) > K.gamma(n) * r["host_wlte"], r
    # what the run must show
    rejected_by_estimate = [r for r in ref["log"] if not r["accepted"] and r["newton_reason"] > 0]
    failed = [r for r in ref["log"] if r["newton_reason"] < 0]
    accepted = [r for r in ref["log"] if r["accepted"]]
    assert len(rejected_by_estimate) >= 1 and all(r["wlte"] > 1.0 for r in rejected_by_estimate)
    assert len(failed) >= 1 and all(r["newton_reason"] == N.DIVERGED_MAX_IT and r["wlte"] == -1.0 and not r["accepted"] for r in failed)
    assert any(b["dt"] == 10.0 * a["dt"] for a, b in zip(accepted[:-1], accepted[1:])), "no growth by the cap"
    assert info["reason"] == T.CONVERGED_TIME and info["t"] == ADAPTIVE["max_time"] and info["dt_last"] < info["dt_next"], "the last step was not shortened"
    assert info["rejections"] == len(rejected_by_estimate) + len(failed) and info["attempts"] == info["steps"] + info["rejections"]
    # decisions, the dt sequence, U and V bit for bit; each device wlte within the bound of the host's
    _same_log(info, ref, wlte_bound=n)
    assert np.array_equal(U, Ur) and np.array_equal(V, Vr)
    _unorm_holds(info, U)


# ---- 4. outcomes
def _nan_equal(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_failures_hand_back_the_last_accepted_state():
    U0, V0 = _adaptive_state()
    eng, _ = _adaptive_engine()
    hopeless = dict(ADAPTIVE_NEWTON, maxit=1, rtol=1e-12)      # one Newton iteration never reaches 1e-12 |F_0| on a nonlinear residual
    # a failed attempt without adapt
    U, V, info = _device(eng, U0, V0, 1e-3, max_steps=3, **hopeless)
    print("no adapt:", {k: v for k, v in info.items() if k != "log"}, info["log"])
    assert info["reason"] == T.DIVERGED_NONLINEAR_SOLVE and info["steps"] == 0 and info["attempts"] == 1 and info["rejections"] == 0 and info["t"] == 0.0
    assert info["log"]["newton_reason"][0] == N.DIVERGED_MAX_IT and np.array_equal(U, U0) and np.array_equal(V, V0) and info["unorm"] == 0.0
    # ... after two good steps: the state of those two
    good = dict(ADAPTIVE_NEWTON, maxit=12)
    U2, V2, two = _device(eng, U0, V0, 1e-3, max_steps=2, **good)
    assert two["reason"] == T.CONVERGED_STEPS and two["steps"] == 2
    # max_rejections exhausted by Newton failures
    U, V, info = _device(eng, U0, V0, 1e-3, max_steps=3, adapt=True, max_rejections=2, **hopeless)
    print("max_rejections, Newton:", {k: v for k, v in info.items() if k != "log"}, info["log"]["dt"])
    assert info["reason"] == T.DIVERGED_NONLINEAR_SOLVE and info["attempts"] == 3 and info["rejections"] == 3 and np.array_equal(U, U0) and np.array_equal(V, V0)
    assert list(info["log"]["dt"]) == [1e-3, 1e-3 / 4, 1e-3 / 4 / 4]
    # dt_min reached by a Newton failure
    U, V, info = _device(eng, U0, V0, 1e-3, max_steps=3, adapt=True, max_rejections=9, dt_min=5e-4, **hopeless)
    assert info["reason"] == T.DIVERGED_NONLINEAR_SOLVE and info["attempts"] == 1 and info["rejections"] == 1 and np.array_equal(U, U0)
    # an estimate that never passes: max_rejections, then dt_min; the first (estimate-free) step is kept
    tight = dict(adapt=True, adapt_rtol=1e-14, adapt_atol=1e-14, max_steps=2)
    U1, V1, one = _device(eng, U0, V0, 1e-3, max_steps=1, **good)
    U, V, info = _device(eng, U0, V0, 1e-3, max_rejections=2, **tight, **good)
    print("max_rejections, estimate:", {k: v for k, v in info.items() if k != "log"}, info["log"]["wlte"])
    assert info["reason"] == T.DIVERGED_STEP_REJECTED and info["steps"] == 1 and info["rejections"] == 3 and info["attempts"] == 4 and info["t"] == 1e-3
    assert np.array_equal(U, U1) and np.array_equal(V, V1) and info["unorm"] == one["unorm"] and np.all(info["log"]["wlte"][1:] > 1.0)
    U, V, info = _device(eng, U0, V0, 1e-3, max_rejections=50, dt_min=2e-5, **tight, **good)
    print("dt_min:", {k: v for k, v in info.items() if k != "log"}, info["log"]["dt"])
    assert info["reason"] == T.DIVERGED_STEP_REJECTED and info["steps"] == 1 and info["rejections"] == 2 and np.array_equal(U, U1) and np.array_equal(V, V1)
    assert list(info["log"]["dt"]) == [1e-3, 1e-3, 0.1 * 1e-3]
    # a NaN in V_0: the state is handed back as it came, and the next clean call on the poisoned work vectors is what it was
    bad = np.array(V0)
    bad[108] = np.nan      # an interior control point
    U, V, info = _device(eng, U0, bad, 1e-3, max_steps=2, **good)
    print("NaN in V_0: reason %d, newton reason %s" % (info["reason"], info["log"]["newton_reason"]))
    assert info["reason"] in (T.DIVERGED_NAN, T.DIVERGED_NONLINEAR_SOLVE) and info["steps"] == 0 and np.array_equal(U, U0) and _nan_equal(V, bad)
    U, V, info = _device(eng, U0, bad, 1e-3, max_steps=2, adapt=True, max_rejections=1, **good)
    assert info["reason"] in (T.DIVERGED_NAN, T.DIVERGED_NONLINEAR_SOLVE) and info["steps"] == 0 and np.array_equal(U, U0) and _nan_equal(V, bad)
    U, V, again = _device(eng, U0, V0, 1e-3, max_steps=2, **good)
    assert np.array_equal(U, U2) and np.array_equal(V, V2) and again["log"].tobytes() == two["log"].tobytes() and again["unorm"] == two["unorm"]


def test_nothing_to_do_and_refusals_that_need_vectors():
    import petiga_amd as P
    U0, V0 = _adaptive_state()
    eng, _ = _adaptive_engine()
    U, V = eng.create_vec().set(U0), eng.create_vec().set(V0)
    for kw, reason in ((dict(max_steps=0), T.CONVERGED_STEPS), (dict(max_steps=3, t0=0.5, max_time=0.5), T.CONVERGED_TIME)):
        info = eng.time_step(U, V, 1e-3, **kw)
        assert info["reason"] == reason and info["steps"] == 0 and info["attempts"] == 0 and info["dt_next"] == 1e-3 and info["log"].size == 0
        assert np.array_equal(U.get(), U0) and np.array_equal(V.get(), V0)
    with pytest.raises(P.IGXError) as e:      # no previous call on this IGX
        eng.time_step(U, V, 1e-3, resume=True)
    assert e.value.code == 58 and "resume" in str(e.value), str(e.value)
    _, other = make_pair(3, 1, 2, [4, 4, 4])
    other.set_form("bratu", (3.5,))
    for args, word in (((U, U), "different"), ((None, V), "null"), ((U, None), "null"), ((other.create_vec(), V), "another IGX"), ((U, other.create_vec()), "another IGX")):
        with pytest.raises(P.IGXError) as e:
            eng.time_step(args[0], args[1], 1e-3)
        assert e.value.code == 62 and word in str(e.value), str(e.value)
    # a vector made before IGXSetUp ran again on other axes has another size than the space's
    stale = other.create_vec()
    other.axis_uniform(0, 2, 5)
    other.setup()
    other.set_form("bratu", (3.5,))
    fits = other.create_vec()
    assert stale.n != fits.n
    for args in ((stale, fits), (fits, stale), (stale, stale)):
        with pytest.raises(P.IGXError) as e:
            other.time_step(args[0], args[1], 1e-3)
        assert e.value.code == 62, str(e.value)
    # IGXSolve's refusal in the loop arrives under the stepper's name, with U and V as they were
    _, ch = action_pair("ch-p2")
    ch.set_form("cahnhilliard", CH)
    Uc = np.array(action_reference("ch-p2")[1])
    Uv, Vv = ch.create_vec().set(Uc), ch.create_vec().fill(0.0)
    with pytest.raises(P.IGXError) as e:      # the diagonal does not cover Cahn-Hilliard
        ch.time_step(Uv, Vv, 1e-4, pc="jacobi")
    assert e.value.code == 56 and "IGXTimeStep" in str(e.value) and "Newton solve" in str(e.value), str(e.value)
    assert np.array_equal(Uv.get(), Uc) and not Vv.get().any()
    info = eng.time_step(U, V, 1e-3, max_steps=1, **dict(ADAPTIVE_NEWTON, maxit=12))
    assert info["reason"] == T.CONVERGED_STEPS and info["steps"] == 1


def test_resume_equals_one_long_run():
    U0, V0 = _adaptive_state()
    eng, _ = _adaptive_engine()
    kw = dict(adapt=True, adapt_rtol=3e-3, adapt_atol=3e-3, max_rejections=6, **dict(ADAPTIVE_NEWTON, maxit=12))
    U6, V6, six = _device(eng, U0, V0, 1e-5, max_steps=6, **kw)
    U, V = eng.create_vec().set(U0), eng.create_vec().set(V0)
    a = eng.time_step(U, V, 1e-5, alpha=RHO, max_steps=3, **kw)
    # a caller's Newton solve and Krylov solve between the two calls leave what resume continues from alone
    x = eng.create_vec().set(U0)
    eng.solve_nonlinear(x, op="ijacobian", a=50.0, W=eng.create_vec().set(-50.0 * U0), pc="jacobi", maxit=3)
    eng.solve(eng.create_vec().set(V0), eng.create_vec().fill(0.0), method="bicgstab", op="jacobian", U=x, pc="jacobi", rtol=1e-6)
    b = eng.time_step(U, V, a["dt_next"], alpha=RHO, max_steps=3, t0=a["t"], resume=True, **kw)
    print("six: dt %s wlte %s\n3 + 3: dt %s wlte %s" % (six["log"]["dt"], six["log"]["wlte"], np.r_[a["log"]["dt"], b["log"]["dt"]], np.r_[a["log"]["wlte"], b["log"]["wlte"]]))
    assert six["steps"] == 6 and a["steps"] == b["steps"] == 3
    assert np.array_equal(U.get(), U6) and np.array_equal(V.get(), V6)
    assert (a["log"].tobytes() + b["log"].tobytes()) == six["log"].tobytes() and b["t"] == six["t"] and b["dt_next"] == six["dt_next"] and b["unorm"] == six["unorm"]
    assert b["log"]["wlte"][0] >= 0.0                       # the estimate is available at once
    # ... and the restatement does the same from the kept (U_{n-1}, h_{n-1})
    Ua, Va, ra = _host(eng, U0, V0, 1e-5, max_steps=3, device_wlte=a["log"]["wlte"], **kw)
    Ub, Vb, rb = _host(eng, Ua, Va, ra["dt_next"], max_steps=3, t0=ra["t"], prev=ra["prev"], device_wlte=b["log"]["wlte"], **kw)
    assert np.array_equal(Ub, U6) and np.array_equal(Vb, V6)
    # IGXSetUp drops the kept state
    import petiga_amd as P
    eng.setup()
    eng.set_form("bratu", (ADAPTIVE["lam"],))
    with pytest.raises(P.IGXError) as e:
        eng.time_step(eng.create_vec().set(U6), eng.create_vec().set(V6), 1e-5, resume=True)
    assert e.value.code == 58


def test_kernel_name_and_timing():
    eng, U0, V0, h, alpha, kw = _case("bratu-p2")
    eng.set_timing(True)
    U, V, info = _device(eng, U0, V0, h, max_steps=3, **kw)
    total, kernel, launches = eng.last_timing()
    name = eng.kernel_name()
    eng.set_timing(False)
    print("%s: %.3f ms, operators %.3f ms, %d launches" % (name, total, kernel, launches))
    assert name.startswith("timestep(am=0.833333, af=0.666667, g=0.666667, newton(basic, krylov(bicgstab, pc=jacobi, vec_sumfact") and name.endswith(", 3 steps, 0 rejections)")
    assert total > 0 and 0 < kernel <= total and launches > 3 * 3


# ---- 5. physics, against something other than the engine
def test_cahn_hilliard_conserves_mass():
    """no Dirichlet face: the row sums of the residual's divergence terms vanish, so 1 . M V = 0 at every stage and m . U_n, m = M 1 from the
    oracle's Mass matrix on the same discretisation, stays what it was"""
    eng, U0, V0, h, alpha, kw = _case("ch-p2")
    orc, _ = action_pair("ch-p2")
    m = orc.compute_system("orc_form_mass")[0].scipy() @ np.ones(U0.size)
    mass0 = K.exact_dot(m, U0)[0]
    drift = []
    Uv, Vv, t, dt = eng.create_vec().set(U0), eng.create_vec().set(V0), 0.0, h
    for step in range(5):      # one call per step, each continuing the one before, to see every U_n
        info = eng.time_step(Uv, Vv, dt, alpha=alpha, max_steps=1, t0=t, resume=step > 0, **kw)
        assert info["steps"] == 1 and info["reason"] == T.CONVERGED_STEPS
        t, dt, U = info["t"], info["dt_next"], Uv.get().copy()
        drift.append(abs(K.exact_dot(m, U)[0] - mass0))
    Ur, Vr, ref = _host_chain(eng, U0, V0, h, 5, alpha=alpha, **kw)[-1]
    assert np.array_equal(U, Ur)
    drift_host = abs(K.exact_dot(m, Ur)[0] - mass0)
    tol = max(8 * drift_host, 1e-13 * abs(mass0))
    print("Cahn-Hilliard: m . U_0 = %.17g; |m . U_n - m . U_0| = %s; the host loop's after 5 steps %.3e; tolerance %.3e; |U_5 - U_0| = %.3e" % (
        mass0, ["%.3e" % d for d in drift], drift_host, tol, np.abs(U - U0).max()))
    assert np.abs(U - U0).max() > 1e-6 and max(drift) <= tol


def test_bratu_backward_euler_against_the_oracle():
    orc, eng = _bratu_pair(2, (5, 4, 3), 3.5)
    U0, V0 = _pinned(eng, 0.3 * np.random.default_rng(29).standard_normal(orc.global_size()), **BRATU_NEWTON)
    h, rtol = 0.02, 1e-10
    kw = dict(BRATU_NEWTON, rtol=rtol)
    cpu = T.oracle_callables(orc, "orc_form_bratu_ifunction", "orc_form_bratu_ijacobian", C.c_double(3.5), rtol=rtol, maxit=20)
    Uc, Vc, ref_c = T.integrate(cpu, U0, V0, h, max_steps=3, alpha=T.BACKWARD_EULER)
    Uh, Vh, ref_h = _host(eng, U0, V0, h, alpha=T.BACKWARD_EULER, max_steps=3, **kw)
    U, V, info = _device(eng, U0, V0, h, alpha=T.BACKWARD_EULER, max_steps=3, **kw)
    err, err_host = np.abs(U - Uc).max(), np.abs(Uh - Uc).max()
    bound = max(8 * err_host, 10 * rtol * np.abs(Uc).max())
    print("Bratu, 3 backward-Euler steps: max|U - U_cpu| = %.3e, the host loop's %.3e, bound %.3e; |U_3 - U_0| = %.3e" % (err, err_host, bound, np.abs(Uc - U0).max()))
    assert info["steps"] == ref_c["steps"] == 3 and info["reason"] == T.CONVERGED_STEPS
    assert np.abs(Uc - U0).max() > 1e-3 and err <= bound
