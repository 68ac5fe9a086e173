"""IGXSolve's fused kernels (petiga_amd/csrc/krylov.hpp: kr_resid0, kr_cg_update, kr_jacobi_rz, kr_cg_p, kr_bicg_p, kr_bicg_s, kr_dot2, kr_bicg_xr,
kr_bicg_record) at the lengths where their indexing can go wrong.  512 threads take two entries each, so one workgroup covers 1024 entries and
the capped grid of 256 workgroups 262 144:
  175       Poisson p = 2 (5, 3, 3): odd, one workgroup: the scalar tails of the CG kernels
  1025      Poisson p = 2 (3, 3, 39): 512 pairs fill workgroup 0 exactly, kr_grid = 1, and the tail
  1029      elasticity p = 2 (5, 5, 5), dof 3: 514 pairs, workgroup 1 holds two of them, kr_grid = 2, a second non-zero partial, and the tail
  1331      Bratu p = 3 (8, 8, 8), JacobianAction: BiCGStab with two workgroups and the tail
  1372      NS-VMS p = 2 (5, 5, 5), dof 4, IJacobianAction: BiCGStab, two workgroups, point-block Jacobi, a nonsymmetric operator
  274625    Poisson and Bratu p = 2 (63, 63, 63): 137 312 pairs over 131 072 threads, so 6 240 threads take a second trip of the grid-stride
            loop, all 256 partials are non-zero, and the tail
The yardstick is the host loop of tests/krylov_ref.py on the SAME engine operators (krylov_ref.engine_callables), in three summation orders;
no matrix is assembled.  b is the engine's action on a fixed random x_true, so the error is max|x - x_true|, and the true residual is
b - A x by one more call of the action (held to the oracle by tests/test_gpu_action_entrywise.py and its siblings).  Dirichlet value 0 on
the faces, identity geometry, rtol 1e-10 for CG and 1e-9 for BiCGStab, maxit 600.  u = 2^-53.
  reason, bookkeeping   CONVERGED_RTOL on both sides, history.size == iterations + 1, rnorm == history[-1], rnorm0 == history[0], the kernel name
  bnorm, history[0]     x0 = 0, so r0 = b: both within (gamma_n / 2 + gamma_n^2 + 2u) sqrt(exact) of the root of the exactly rounded sum of
                        squares (derived, tests/test_gpu_vec_algebra.py); one dropped or doubled entry at n = 274 625 moves the sum by 4e-6
  iteration count       within [lo - m, hi + m], lo / hi the host loop's counts over the three orders and m = max(1, hi - lo)
  head of the history   entries 1 to 5 deviate from the np.dot host loop's by 8 x the spread of the three host orders on those entries at the
                        most (the spread floored at 4u)
  true residual, error  |b - A x| <= max(2 rtol |b|, 8 x the host loop's), max|x - x_true| <= max(8 x the host loop's, 1e-13 max|x_true|)
  first iterate (CG)    maxit = 1 from a non-zero x0, entry by entry within the derived bound of the quotient alpha
  prefix, repeatability, outcomes: exact, bit for bit
Every test prints what it sees before it asserts (run with -s; DESIGN.md 3.12 holds the figures)."""
import functools
import math
import time

import numpy as np
import pytest

import krylov_ref as K
from test_gpu_matrix_action import DT, EL, NS

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("krylov_lengths")]      # one worker: the engines and the host loops are made once

U_ROUND = K.U_ROUND
MAXIT = 600
GRID_ENTRIES = 2 * 256 * 512        # the entries one trip of the capped grid covers: an index from here on is written by a second trip
# the amplitude of the Bratu state U = BRATU_AMP x standard normal: the first of 0.3, 0.15, ... at which the host loop (BiCGStab + Jacobi)
# on the large Bratu case reaches rtol within MAXIT
BRATU_AMP = 0.3
# K - lambda e^U M with this lambda is negative on the interior: the first of 1e4, 1e5, ... at which the host loop's CG reports a breakdown
BRATU_LAMBDA_NEGATIVE = 1e4
ZERO6 = [(d, s, 0, 0.0) for d, s in K.ALL6]
# name -> (form, parameters, dof, p, N, Dirichlet values, operator)
CASES = {
    "poisson-175": ("poisson", (), 1, 2, (5, 3, 3), ZERO6, "matrix"),
    "poisson-1025": ("poisson", (), 1, 2, (3, 3, 39), ZERO6, "matrix"),
    "elasticity-1029": ("elasticity", EL, 3, 2, (5, 5, 5), K.SMALL_LENGTHS[1029][4], "matrix"),
    "bratu-1331": ("bratu", (3.5,), 1, 3, (8, 8, 8), ZERO6, "jacobian"),
    "bratu-1331-negative": ("bratu", (BRATU_LAMBDA_NEGATIVE,), 1, 3, (8, 8, 8), ZERO6, "jacobian"),
    "nsvms-1372": ("nsvms", NS, 4, 2, (5, 5, 5), [(1, s, f, 0.1 * f - 0.05 * s) for s in range(2) for f in range(3)], "ijacobian"),
    "poisson-274625": ("poisson", (), 1, 2, (63, 63, 63), ZERO6, "matrix"),
    "bratu-274625": ("bratu", (3.5,), 1, 2, (63, 63, 63), ZERO6, "jacobian"),
}
# (case, method, preconditioner) of section 1
SOLVES = [("poisson-175", "cg", "none"), ("poisson-175", "cg", "jacobi"), ("poisson-1025", "cg", "none"), ("poisson-1025", "cg", "jacobi"),
          ("poisson-1025", "cg", "fastdiag"), ("elasticity-1029", "cg", "jacobi"), ("elasticity-1029", "cg", "pbjacobi"),
          ("bratu-1331", "bicgstab", "jacobi"), ("nsvms-1372", "bicgstab", "pbjacobi"),
          ("poisson-274625", "cg", "none"), ("poisson-274625", "cg", "jacobi"), ("bratu-274625", "bicgstab", "jacobi")]
LOOPS = {"cg": (K.cg, 1e-10), "bicgstab": (K.bicgstab, 1e-9)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(engine, nodes per axis, state keywords of solve() and engine_callables(), x_true, b = A x_true) of a case: made once, never written to"""
    import petiga_amd as P
    form, params, dof, p, N, bcs, op = CASES[name]
    eng = P.IGX(3, dof)
    for i in range(3):
        eng.axis_uniform(i, p, N[i])
    eng.setup()
    for bc in bcs:
        eng.set_boundary_value(*bc)
    eng.set_form(form, params)
    nodes = tuple(N[i] + p for i in range(3))
    n = nodes[0] * nodes[1] * nodes[2] * dof
    rng = np.random.default_rng(29)
    state = dict(op=op)
    if op == "jacobian":
        state["U"] = eng.create_vec().set(BRATU_AMP * rng.standard_normal(n))
    elif op == "ijacobian":
        state.update(a=2.0 / DT, t=0.0, V=eng.create_vec().set(0.1 * rng.standard_normal(n)), U=eng.create_vec().set(0.3 * rng.standard_normal(n)))
    if name == "poisson-1025":
        eng.fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    xt = K.x_true(n)
    b = K.engine_callables(eng, pc="none", **state)[0](xt)
    assert b.size == n == int(name.split("-")[1])
    for a in (xt, b):
        a.setflags(write=False)
    return eng, nodes, state, xt, b


@functools.lru_cache(maxsize=None)
def _callables(name, pc):
    eng, _, state, _, _ = _problem(name)
    return K.engine_callables(eng, pc=pc, **state)


def _orders(n):
    """the three summation orders of the host loop; the chunks grow with the length so that the Python loop over them stays cheap"""
    chunk = 37 if n < 100000 else 4099
    return [np.dot, K.dot_reversed, functools.partial(K.dot_pairwise_chunks, chunk=chunk)]


@functools.lru_cache(maxsize=None)
def _host(name, method, pc):
    """[(x, info)] of the host loop in the three orders (np.dot first) from x0 = 0, and the wall time of the three"""
    _, _, _, _, b = _problem(name)
    op, prec = _callables(name, pc)
    loop, rtol = LOOPS[method]
    t0 = time.perf_counter()
    runs = [loop(op, prec, np.array(b), rtol=rtol, maxit=MAXIT, dot=dot) for dot in _orders(b.size)]
    return runs, time.perf_counter() - t0


def _solve(name, rhs, x0=None, **kw):
    eng, _, state, _, _ = _problem(name)
    b, x = eng.create_vec().set(np.asarray(rhs)), eng.create_vec()
    if x0 is not None:
        x.set(x0)
    info = eng.solve(b, x, history=True, **dict(state, **kw))
    info["name"] = eng.kernel_name()
    return x.get().copy(), info


@functools.lru_cache(maxsize=None)
def _device(name, method, pc):
    """the full device solve from x0 = 0"""
    return _solve(name, _problem(name)[4], method=method, pc=pc, rtol=LOOPS[method][1], maxit=MAXIT)


def _x0(name):
    """a fixed non-zero starting vector"""
    return np.random.default_rng(97).standard_normal(_problem(name)[4].size)


def _same(a, b):
    """bit for bit, NaN included"""
    return np.array_equal(a, b, equal_nan=True)


# ---- 1, 2. the lengths
@pytest.mark.parametrize("name,method,pc", SOLVES)
def test_solve_against_the_host_loop(name, method, pc):
    eng, _, _, xt, b = _problem(name)
    n, rtol = b.size, LOOPS[method][1]
    op, _ = _callables(name, pc)
    runs, t_host = _host(name, method, pc)
    t0 = time.perf_counter()
    x, info = _device(name, method, pc)
    t_dev = time.perf_counter() - t0
    (x_ref, ref) = runs[0]
    k, counts = info["iterations"], [r[1]["iterations"] for r in runs]
    lo, hi, m = K.count_window(counts)
    spread = max(max(K.head_deviation(r[1]["history"], ref["history"]) for r in runs[1:]), 4 * U_ROUND)
    dev = K.head_deviation(info["history"], ref["history"])
    bn = np.linalg.norm(b)
    res, res_ref = np.linalg.norm(b - op(x)), np.linalg.norm(b - op(x_ref))
    err, err_ref = np.abs(x - xt).max(), np.abs(x_ref - xt).max()
    root = math.sqrt(K.exact_dot(b, b)[0])
    nb = K.norm_bound(n, root)
    print("%s, %s, pc %s: %d iterations (host loop %s: lo %d, hi %d, m %d), reason %d; head deviates by %.3e (host orders spread %.3e); "
          "true residual / |b| %.3e (host loop %.3e); max|x - x_true| %.3e (host loop %.3e); |bnorm - exact| %.3e, |history[0] - exact| %.3e "
          "(bound %.3e); host loops %.1f s, device %.2f s; %s"
          % (name, method, pc, k, counts, lo, hi, m, info["reason"], dev, spread, res / bn, res_ref / bn, err, err_ref,
             abs(info["bnorm"] - root), abs(info["history"][0] - root), nb, t_host, t_dev, info["name"]))
    assert all(r[1]["reason"] == K.CONVERGED_RTOL for r in runs), "the host loop does not converge: the case tests nothing"
    assert info["reason"] == K.CONVERGED_RTOL
    assert info["history"].size == k + 1 and info["rnorm"] == info["history"][-1] and info["rnorm0"] == info["history"][0]
    assert info["rnorm"] <= rtol * info["bnorm"]
    assert info["name"].startswith("krylov(%s, pc=%s, vec_sumfact" % (method, pc)) and info["name"].endswith(", %d iterations)" % k), info["name"]
    assert abs(info["bnorm"] - root) <= nb and abs(info["history"][0] - root) <= nb
    assert lo - m <= k <= hi + m
    assert dev <= 8 * spread
    assert res <= max(2 * rtol * bn, 8 * res_ref)
    assert err <= max(8 * err_ref, 1e-13 * np.abs(xt).max())


def _first_iterate_bound(op, prec, b, x0):
    """(the bound on |x - x_ref| entry by entry, |alpha p|) of CG's first iterate from x0, device against host loop; derived in
    test_first_cg_iterate_from_a_nonzero_guess_entry_by_entry"""
    r = b - op(x0)
    p = prec(r)
    Ap = op(p)
    step = np.abs(((r @ p) / (p @ Ap)) * p)
    g = K.gamma(b.size)
    return (2 * g * (1 + np.abs(p * Ap).sum() / abs(p @ Ap)) + 4 * U_ROUND) * step + 4 * U_ROUND * np.abs(x0), step


@pytest.mark.parametrize("name", ["poisson-175", "poisson-1025", "elasticity-1029", "poisson-274625"])
def test_first_cg_iterate_from_a_nonzero_guess_entry_by_entry(name):
    _, _, _, _, b = _problem(name)
    op, prec = _callables(name, "jacobi")
    b, x0 = np.array(b), _x0(name)
    n = b.size
    x_ref, ref = K.cg(op, prec, b, x0=x0, rtol=1e-10, maxit=1)
    x, info = _solve(name, b, x0=x0, method="cg", pc="jacobi", rtol=1e-10, maxit=1)
    assert info["reason"] == K.DIVERGED_ITS == ref["reason"] and info["iterations"] == 1 and info["history"].size == 2
    # x = x0 + alpha p with alpha = r.z / p.Ap and the same r = b - A x0, p = r ./ D and A p bit for bit (the same kernels on the same
    # input, a correctly rounded difference and quotient).  Either loop's r.z (positive terms) is within gamma_n of the exact value and its
    # p.Ap within gamma_n sum|p_i Ap_i| / |p.Ap|; the quotient and the product alpha p round once each on either side: the bound of
    # test_maxit_one_gives_the_host_loops_first_iterate on x - x0 = alpha p.  The sum x0 + alpha p rounds once on either side, u |x| each
    # with |x| <= |x0| + |alpha p|: 4u |x0| once |alpha p| <= |x0|, and where it is not, 2u |alpha p| more, which the first term (gamma_n >=
    # 175u) covers with the sums' orders as they are (np.dot adds pairwise, the device by lanes: neither comes near gamma_n).
    bound, step = _first_iterate_bound(op, prec, b, x0)
    moved = [n - 1] + ([GRID_ENTRIES + int(np.argmax(step[GRID_ENTRIES:]))] if n > GRID_ENTRIES else [])
    print("%s, first iterate from x0 != 0: max|x - x_ref| / bound = %.4f; entries %s moved by %s"
          % (name, (np.abs(x - x_ref) / bound).max(), moved, [abs(x[i] - x0[i]) for i in moved]))
    assert np.all(np.abs(x - x_ref) <= bound)
    assert all(x[i] != x0[i] and x_ref[i] != x0[i] for i in moved), "the tail or a second-trip entry stayed at x0"
    assert name != "poisson-274625" or len(moved) == 2
    root = math.sqrt(K.exact_dot(b - op(x0), b - op(x0))[0])
    assert abs(info["history"][0] - root) <= K.norm_bound(n, root), "|b - A x0| of kr_resid0 with w != 0"


@pytest.mark.parametrize("name,method", [("elasticity-1029", "cg"), ("bratu-1331", "bicgstab")])
def test_a_solve_cut_at_maxit_is_a_prefix_of_the_full_solve(name, method):
    _, _, _, _, b = _problem(name)
    x0, rtol = _x0(name), LOOPS[method][1]
    _, full = _solve(name, b, x0=x0, method=method, pc="jacobi", rtol=rtol, maxit=MAXIT)
    assert full["reason"] == K.CONVERGED_RTOL and full["iterations"] > 3
    for k in range(4):
        x, info = _solve(name, b, x0=x0, method=method, pc="jacobi", rtol=rtol, maxit=k)
        print("%s, %s, maxit %d: reason %d, %d iterations, history %s" % (name, method, k, info["reason"], info["iterations"], info["history"]))
        assert info["reason"] == K.DIVERGED_ITS and info["iterations"] == k
        assert np.array_equal(info["history"], full["history"][:k + 1])
        assert info["rnorm"] == info["history"][-1] and info["rnorm0"] == info["history"][0]
        if k == 0:
            assert np.array_equal(x, x0), "maxit = 0 moved x"


@pytest.mark.parametrize("name,method", [("poisson-274625", "cg"), ("bratu-274625", "bicgstab")])
def test_two_large_solves_give_the_same_bits(name, method):
    x, info = _device(name, method, "jacobi")
    x2, info2 = _solve(name, _problem(name)[4], method=method, pc="jacobi", rtol=LOOPS[method][1], maxit=MAXIT)
    assert info2["iterations"] == info["iterations"] and np.array_equal(info2["history"], info["history"]) and np.array_equal(x2, x)


# ---- 3. outcomes: the host loop is asked first, so that a case cannot test nothing
def _corner_rhs():
    _, nodes, _, _, _ = _problem("poisson-175")
    b = np.zeros(175)
    b[K.corner_dofs(nodes)] = np.random.default_rng(8).standard_normal(8)
    op, _ = _callables("poisson-175", "none")
    assert np.count_nonzero(b) == 8 and np.array_equal(op(b), b), "A b = b does not hold exactly on the corners"
    return b, op


def test_cg_is_exact_after_one_step_on_a_corner_supported_right_hand_side():
    b, op = _corner_rhs()
    x_ref, ref = K.cg(op, lambda v: v.copy(), b, rtol=1e-10)
    assert ref["reason"] == K.CONVERGED_RTOL and ref["iterations"] == 1 and ref["rnorm"] == 0.0 and np.array_equal(x_ref, b)
    x, info = _solve("poisson-175", b, method="cg", pc="none", rtol=1e-10)
    print("corner right-hand side, CG: reason %d, %d iterations, history %s" % (info["reason"], info["iterations"], info["history"]))
    assert info["reason"] == K.CONVERGED_RTOL and info["iterations"] == 1
    assert info["rnorm"] == 0.0 and info["history"].size == 2
    assert np.array_equal(x, b)


def test_bicgstab_breaks_down_at_iteration_zero_and_leaves_x_alone():
    b, op = _corner_rhs()
    x0 = 0.375 * b
    x_ref, ref = K.bicgstab(op, lambda v: v.copy(), b, x0=x0, rtol=1e-9)
    assert ref["reason"] == K.DIVERGED_BREAKDOWN and ref["iterations"] == 0 and ref["history"].size == 1 and np.array_equal(x_ref, x0)
    x, info = _solve("poisson-175", b, x0=x0, method="bicgstab", pc="none", rtol=1e-9)
    print("corner residual, BiCGStab: reason %d, %d iterations, history %s (host loop %s)" % (info["reason"], info["iterations"], info["history"], ref["history"]))
    assert info["reason"] == K.DIVERGED_BREAKDOWN and info["iterations"] == 0 and info["history"].size == 1
    assert info["rnorm"] == info["history"][0] and abs(info["history"][0] - ref["history"][0]) <= 8 * U_ROUND * ref["history"][0]      # eight terms
    assert np.array_equal(x, x0), "x is not the iterate whose norm was tested"


def test_cg_reports_a_negative_curvature_with_the_host_loops_count():
    name = "bratu-1331-negative"
    _, _, _, _, b = _problem(name)
    op, prec = _callables(name, "none")
    b, x0 = np.array(b), _x0(name)
    x_ref, ref = K.cg(op, prec, b, x0=x0, rtol=1e-10, maxit=MAXIT)
    assert ref["reason"] == K.DIVERGED_BREAKDOWN, "lambda = %g does not make the host loop break down" % BRATU_LAMBDA_NEGATIVE
    x, info = _solve(name, b, x0=x0, method="cg", pc="none", rtol=1e-10, maxit=MAXIT)
    k = ref["iterations"]
    print("Bratu, lambda = %g, CG: reason %d after %d iterations (host loop: %d after %d)" % (BRATU_LAMBDA_NEGATIVE, info["reason"], info["iterations"], ref["reason"], k))
    assert info["reason"] == K.DIVERGED_BREAKDOWN and info["iterations"] == k and info["history"].size == k + 1
    if k == 0:
        assert np.array_equal(x, x0)
    else:
        bn, res, res_ref = np.linalg.norm(b), np.linalg.norm(b - op(x)), np.linalg.norm(b - op(x_ref))
        print("   true residual / |b| %.3e (host loop %.3e)" % (res / bn, res_ref / bn))
        assert res <= max(2e-10 * bn, 8 * res_ref)
        if k == 1:      # the iterate is the first one: entry by entry as well
            bound, _ = _first_iterate_bound(op, prec, b, x0)
            print("   max|x - x_ref| / bound = %.4f" % (np.abs(x - x_ref) / bound).max())
            assert np.all(np.abs(x - x_ref) <= bound)


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_a_nan_is_reported_and_does_not_poison_the_next_solve(method):
    name = "elasticity-1029"
    _, _, _, _, b = _problem(name)
    op, prec = _callables(name, "jacobi")
    loop, rtol = LOOPS[method]
    x0 = _x0(name)
    before = _solve(name, b, x0=x0, method=method, pc="jacobi", rtol=rtol, maxit=MAXIT)
    assert before[1]["reason"] == K.CONVERGED_RTOL
    for at in (b.size - 1, 1026):      # the tail entry; an entry of workgroup 1
        bad = np.array(b)
        bad[at] = np.nan
        x_ref, ref = loop(op, prec, bad, x0=x0, rtol=rtol, maxit=MAXIT)
        assert ref["reason"] == K.DIVERGED_NAN and ref["iterations"] == 0 and np.array_equal(x_ref, x0)
        x, info = _solve(name, bad, x0=x0, method=method, pc="jacobi", rtol=rtol, maxit=MAXIT)
        print("NaN in b[%d], %s: reason %d, %d iterations, bnorm %r, history %s" % (at, method, info["reason"], info["iterations"], info["bnorm"], info["history"]))
        assert info["reason"] == K.DIVERGED_NAN and info["iterations"] == 0 and info["history"].size == 1
        assert np.array_equal(x, x0), "x moved"
    # the kept work vectors hold NaN now
    after = _solve(name, b, x0=x0, method=method, pc="jacobi", rtol=rtol, maxit=MAXIT)
    assert after[1]["iterations"] == before[1]["iterations"] and after[1]["reason"] == before[1]["reason"]
    assert _same(after[1]["history"], before[1]["history"]) and _same(after[0], before[0]), "a solve depends on what the one before left in the work vectors"


def test_changing_the_kept_work_vectors_changes_nothing():
    name = "poisson-175"
    _, _, _, _, b = _problem(name)
    runs = [_solve(name, b, method=method, pc=pc, rtol=LOOPS[method][1], maxit=MAXIT)
            for method, pc in (("cg", "jacobi"), ("bicgstab", "none"), ("cg", "none"), ("cg", "jacobi"))]
    print("CG + Jacobi, BiCGStab, CG, CG + Jacobi: iterations %s, reasons %s" % ([r[1]["iterations"] for r in runs], [r[1]["reason"] for r in runs]))
    assert all(r[1]["reason"] == K.CONVERGED_RTOL for r in runs)
    assert np.array_equal(runs[3][0], runs[0][0]) and np.array_equal(runs[3][1]["history"], runs[0][1]["history"])


@pytest.mark.parametrize("name,method", [("elasticity-1029", "cg"), ("bratu-1331", "bicgstab")])
def test_atol_with_a_nonzero_right_hand_side(name, method):
    _, _, _, _, b = _problem(name)
    op, prec = _callables(name, "jacobi")
    atol = 1e-6 * np.linalg.norm(b)
    _, ref = LOOPS[method][0](op, prec, np.array(b), rtol=0.0, atol=atol, maxit=MAXIT)
    assert ref["reason"] == K.CONVERGED_ATOL and 0 < ref["rnorm"] <= atol
    x, info = _solve(name, b, method=method, pc="jacobi", rtol=0.0, atol=atol, maxit=MAXIT)
    print("%s, %s, rtol 0, atol %.3e: reason %d, %d iterations (host loop %d), rnorm %.3e" % (name, method, atol, info["reason"], info["iterations"], ref["iterations"], info["rnorm"]))
    assert info["reason"] == K.CONVERGED_ATOL and 0 < info["rnorm"] <= atol
    assert info["history"].size == info["iterations"] + 1 and info["rnorm"] == info["history"][-1]
