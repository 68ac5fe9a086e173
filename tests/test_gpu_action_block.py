"""The matrix-free actions on a block of vectors (IGXComputeMatrixActionBlock / JacobianActionBlock / IJacobianActionBlock:
vec_sumfact with BATCH, petiga_amd/csrc/vec_sumfact.hpp) on the GPU.  The cases and references are those of
tests/test_gpu_action_entrywise.py, tests/test_gpu_matrix_action.py and tests/test_gpu_matrix_free_high_degree.py, by import; one case per
code path of the kernel:
  poisson-p2-graded-odd        two elements per wavefront, spans (5, 4, 3): the last wavefront holds one element
  poisson-p3-graded            one wavefront per element, the scalar form without a geometry (its single action loads F early: PIPE)
  poisson-p3-rational          a map with weights (GEO; the single action's early F: EF)
  poisson-p2-periodic          a periodic axis wrapped inside the rank
  elasticity-p3-affine         three fields on a map
  bratu-(i)jacobian-p3-graded  the Jacobian operators at a varying state
  ch-p2-graded-dirichlet       second-order features (the direction goes forward to order 2)
  nsvms-p2-nurbs               four fields on a NURBS map, IJacobian (the kernel at its register ceiling)
  poisson-p5, poisson-p7       one workgroup per element, 6 x 6 x 6 and 8 x 8 x 8 lanes
Checks
  each column against the reference   |Y_c - R_c| <= c u S_c row by row against the long double references with the project's constants
                                      (C_ID, C_MAP), for a block of two standard-normal columns around one with magnitudes spread over
                                      10^-6 .. 10^6; the cases without such a reference against the oracle's matrix at their files' own
                                      tolerances, for the block (X, -2 X, X / 2) of the file's X (scaling by a power of two is exact, so
                                      the file's R and S scale with it; a column gathered from a neighbour is off by a factor)
  block against single                np.array_equal.  Nothing promises it -- the compiler is free to contract differently in the two
                                      instantiations -- so the first version of this test held |Y_block - Y_single| <= 2 c u S (both lie
                                      within c u S of one reference) and counted the differing entries: 0 of 16 494 on the eleven cases on
                                      an MI355X, and the bound was replaced by bit equality.  The count is still printed
  a fixed row                         holds count x X_row for every column, within count u |count x X_row| (X_row is added once per element
                                      that holds the node, at most (p + 1)^3 <= 64, and each add rounds once); count itself, exactly,
                                      from the action on a vector of ones
  block sizes                         nx = 1, 2, 16, 17, 33: IGXGetLastTiming's launches = colours x ceil(nx / 16), colours from IGXGetColoring
  bit facts (np.array_equal)          two calls agree; a column's result is the same bits alone, at another place, in another chunk and
                                      beside other columns (a block, its reverse, its leading parts); a repeated X entry gives equal results;
                                      a NaN-filled Y is overwritten (every call here starts from one); rows outside a column's coupling are
                                      exactly 0.0
  a run-time struct                   the block call equals the single calls bit for bit (the same kernel) and says "column by column"
  refusals                            those that need vectors, in the header's order, and the action's IGX_ERR_SUP under the block's name
Two ranks: tests/test_gpu_action_block_ranks.py.  Every test prints what it sees before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import pointwise_ref as PW
import tensor_ref as T
import test_gpu_action_entrywise as AE
import test_gpu_matrix_action as MA
import test_gpu_matrix_free_high_degree as HD
from test_pointwise_reference import wide

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
ARG_WRONG, OUTOFRANGE, SUP, WRONGSTATE = 62, 63, 56, 73
MAXCOLS = 16

LD_CASES = {name: (AE.PROBE.get(name) or AE.ROWWISE[name]) for name in
            ("poisson-p2-graded-odd", "poisson-p3-graded", "poisson-p3-rational", "poisson-p2-periodic", "elasticity-p3-affine",
             "bratu-jacobian-p3-graded", "bratu-ijacobian-p3-graded", "ch-p2-graded-dirichlet")}
ORACLE_CASES = {"nsvms-p2-nurbs": MA, "poisson-p5": HD, "poisson-p7": HD}


class _Runner:
    """An engine with its form set and the state on the device; block(Xs) and single(X) return the results on the host"""

    def __init__(self, eng, driver, shift=0.0, Ustate=None, Vstate=None):
        self.eng, self.driver, self.shift = eng, driver, shift
        self.Uv = eng.create_vec().set(Ustate) if Ustate is not None else None
        self.Vv = eng.create_vec().set(Vstate) if Vstate is not None else None
        self.n = eng.create_vec().n
        c = eng.coloring()
        self.colours = c[0] * c[1] * c[2]

    def block(self, Xs, Xv=None, Yv=None):
        eng = self.eng
        Xv = Xv if Xv is not None else [eng.create_vec().set(x) for x in Xs]
        Yv = Yv if Yv is not None else [eng.create_vec().set(np.full(self.n, np.nan)) for _ in Xv]      # the call zeroes its results itself
        if self.driver == "matrix":
            eng.compute_matrix_action_block(Xv, Yv)
        elif self.driver == "jacobian":
            eng.compute_jacobian_action_block(self.Uv, Xv, Yv)
        else:
            eng.compute_ijacobian_action_block(self.shift, self.Vv, 0.0, self.Uv, Xv, Yv)
        eng.synchronize()
        self.kernel, self.launches = eng.kernel_name(), eng.last_timing()[2]
        return [y.get().copy() for y in Yv]

    def single(self, X):
        eng = self.eng
        Xv, Y = eng.create_vec().set(X), eng.create_vec()
        if self.driver == "matrix":
            eng.compute_matrix_action(Xv, Y)
        elif self.driver == "jacobian":
            eng.compute_jacobian_action(self.Uv, Xv, Y)
        else:
            eng.compute_ijacobian_action(self.shift, self.Vv, 0.0, self.Uv, Xv, Y)
        eng.synchronize()
        return Y.get().copy()


def _ld_runner(name):
    kw, form, driver = LD_CASES[name]
    act = AE._Action(kw, form, driver)
    return act, _Runner(act.eng, driver, act.shift, act.U, act.V)


def _oracle_runner(name):
    mod = ORACLE_CASES[name]
    form = mod.CASES[name][0]
    _, eng = mod._pair(name)
    X, Us, Vs = mod._reference(name)[:3]
    if mod is MA:
        eng.set_form(form, {"poisson": (), "nsvms": MA.NS}[form])
        shift = 2.0 / MA.DT
    else:
        HD._set_form(name, eng)
        shift = HD.I_SHIFT.get(form, 0.0)
    driver = "matrix" if form in ("poisson", "elasticity") else ("jacobian" if form == "bratu" else "ijacobian")
    return _Runner(eng, driver, shift, Us if driver != "matrix" else None, Vs if driver == "ijacobian" else None)


def _runner(name):
    return _ld_runner(name)[1] if name in LD_CASES else _oracle_runner(name)


def _layout_words(name):
    if name in ORACLE_CASES and ORACLE_CASES[name] is HD:
        k = HD.CASES[name][8]
        return "one workgroup per element, %d x %d x %d lanes" % (k, k, k)
    return "two elements per wavefront" if "-p2" in name else "one wavefront per element"


def _check_name(run, name):
    assert run.kernel.startswith("vec_sumfact(matrix action on a block: sum factorisation forward and backward, ") and _layout_words(name) in run.kernel, run.kernel


@pytest.mark.parametrize("name", list(LD_CASES))
def test_every_column_against_the_long_double_reference(name):
    kw = LD_CASES[name][0]
    act, run = _ld_runner(name)
    ref, _, action = AE._references(act, kw)
    n = act.n
    Xs = [np.random.default_rng(31).standard_normal(n), wide(n), np.random.default_rng(32).standard_normal(n)]
    Ys = run.block(Xs)
    _check_name(run, name)
    assert run.launches == run.colours, (run.launches, run.colours)
    fixed = ref.fixed(np.arange(n))[0] if kw.get("bcs") else np.zeros(n, dtype=bool)
    count = run.single(np.ones(n))[fixed]
    assert np.array_equal(count, np.round(count)) and (not fixed.any() or (count.min() >= 1 and count.max() <= 64))
    worst, differing = [], 0
    for c, (X, Y) in enumerate(zip(Xs, Ys)):
        R, S = action(X)
        worst.append(PW.compare_rows(Y, R, S, act.c, ref, "%s column %d" % (name, c)))
        want = count * X[fixed]
        assert np.all(np.abs(Y[fixed] - want) <= count * U * np.abs(want)), "%s column %d: a fixed row does not hold count x X_row" % (name, c)
        Y1 = run.single(X)
        differing += int(np.count_nonzero(Y != Y1))
        assert np.array_equal(Y, Y1), "%s column %d: the block's column and the single action differ" % (name, c)
    print("%-28s %s: worst %s u S (c = %g); %d fixed rows; block against single: %d of %d entries differ"
          % (name, run.kernel[28:], " ".join("%.2f" % w for w in worst), act.c, int(fixed.sum()), differing, 3 * n))


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_every_column_against_the_oracle_matrix(name):
    mod = ORACLE_CASES[name]
    X, _, _, R, S, fixed, diag = mod._reference(name)
    tol = mod.CASES[name][7]
    run = _oracle_runner(name)
    scales = (1.0, -2.0, 0.5)
    Ys = run.block([s * X for s in scales])
    _check_name(run, name)
    assert run.launches == run.colours, (run.launches, run.colours)
    differing = 0
    for s, Y in zip(scales, Ys):
        MA._check(Y, s * X, s * R, abs(s) * S, fixed, diag, tol)
        Y1 = run.single(s * X)
        differing += int(np.count_nonzero(Y != Y1))
        assert np.array_equal(Y, Y1), "%s x %g: the block's column and the single action differ" % (name, s)
    print("%-16s %s: block against single: %d of %d entries differ" % (name, run.kernel[28:], differing, 3 * X.size))


SIZES = ["poisson-p2-graded-odd", "poisson-p3-graded", "poisson-p3-rational", "elasticity-p3-affine", "bratu-ijacobian-p3-graded", "nsvms-p2-nurbs", "poisson-p5", "poisson-p7"]


@pytest.mark.parametrize("name", SIZES)
def test_block_sizes_and_bit_facts(name):
    run = _runner(name)
    n = run.n
    pool = [x.copy() for x in np.random.default_rng(41).standard_normal((33, n))]
    full = run.block(pool)
    _check_name(run, name)
    assert run.launches == 3 * run.colours
    assert all(np.all(np.isfinite(y)) for y in full)                                     # the NaN the results started from is gone
    again = run.block(pool)
    assert all(np.array_equal(a, b) for a, b in zip(full, again)), "two calls differ"
    for nx in (1, 2, 16, 17):                                                            # the leading parts: alone, one chunk, one column into the second
        part = run.block(pool[:nx])
        assert run.launches == run.colours * -(-nx // MAXCOLS), (nx, run.launches, run.colours)
        assert all(np.array_equal(a, b) for a, b in zip(part, full)), "nx = %d: a column depends on its neighbours" % nx
    back = run.block(pool[::-1])                                                         # every column at another place, most in another chunk
    assert all(np.array_equal(a, b) for a, b in zip(back[::-1], full)), "a column depends on its place in the block"
    Xv = [run.eng.create_vec().set(x) for x in pool[:2]]
    twice = run.block(None, Xv=[Xv[0], Xv[1], Xv[0]])                                    # the same vector at two places
    assert np.array_equal(twice[0], twice[2]) and np.array_equal(twice[0], full[0]) and np.array_equal(twice[1], full[1])
    # rows outside a column's coupling: the direction lives on one node, the rows the single action leaves at exactly 0.0 stay exactly 0.0
    dof = run.eng.dof
    node = (n // dof) // 2
    E = np.zeros(n)
    E[node * dof:(node + 1) * dof] = 1.5
    alone = run.single(E)
    sparse = run.block([pool[0], E, pool[1]])
    outside = alone == 0.0
    assert np.array_equal(sparse[0], full[0]) and np.array_equal(sparse[2], full[1])
    assert outside.any() and not outside.all() and not sparse[1][outside].any(), "a row outside the column's coupling is not exactly 0.0"
    print("%-28s %s: %d colours; 33, 1, 2, 16, 17 columns, reversed, repeated, beside a one-node direction (%d of %d rows outside its coupling)"
          % (name, run.kernel[28:], run.colours, int(outside.sum()), n))


@pytest.mark.parametrize("geo", [None, "poly"])
def test_run_time_struct_goes_column_by_column(geo):
    from common import make_pair, warped_geometry
    orc, eng = make_pair(3, 1, 2, [4, 4, 3])
    if geo:
        Xg, Wg = warped_geometry(orc, 3, seed=9, rational=False, amp=0.08)
        eng.set_geometry(Xg, Wg)
    eng.set_boundary_value(0, 0, 0, 2.0)
    eng.set_boundary_value(2, 1, 0, -1.0)
    eng.set_form_source(MA.USER_DIFFUSION, "UserDiffusion", (0.7,))
    run = _Runner(eng, "matrix")
    Xs = [x.copy() for x in np.random.default_rng(31).standard_normal((3, run.n))]
    Ys = run.block(Xs)
    print(run.kernel, run.launches)
    assert "hiprtc" in run.kernel and "matrix action on a block, column by column" in run.kernel, run.kernel
    assert run.launches == 3 * run.colours
    for X, Y in zip(Xs, Ys):
        assert np.array_equal(Y, run.single(X))


def test_refusals_that_need_vectors():
    import petiga_amd as P
    kw, form, driver = LD_CASES["poisson-p2-graded-odd"]
    _, eng, _ = T.setup_case(dim=3, engine=True, **kw)
    _, other, _ = T.setup_case(dim=3, engine=True, **kw)
    X, Y = [eng.create_vec() for _ in range(3)], [eng.create_vec() for _ in range(3)]
    Us = eng.create_vec()

    def refused(call, code, word):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))

    # no form is set yet: rules 3 and 4 answer before it
    refused(lambda: eng.compute_matrix_action_block(X[:2] + [other.create_vec()], Y), ARG_WRONG, "another IGX")
    refused(lambda: eng.compute_matrix_action_block(X, Y[:2] + [other.create_vec()]), ARG_WRONG, "another IGX")
    refused(lambda: eng.compute_jacobian_action_block(other.create_vec(), X, Y), ARG_WRONG, "another IGX")
    refused(lambda: eng.compute_matrix_action_block(X, [Y[0], Y[1], Y[0]]), ARG_WRONG, "two results")
    refused(lambda: eng.compute_matrix_action_block(X, [Y[0], Y[1], X[0]]), ARG_WRONG, "different vectors")
    refused(lambda: eng.compute_jacobian_action_block(Us, X, [Y[0], Us, Y[2]]), ARG_WRONG, "state vector")
    refused(lambda: eng.compute_ijacobian_action_block(1.0, Us, 0.0, eng.create_vec(), X, [Y[0], Us, Y[2]]), ARG_WRONG, "state vector")
    refused(lambda: eng.compute_matrix_action_block(X, Y), WRONGSTATE, "IGASetForm")      # 5
    eng.set_form("poisson")
    eng.set_boundary_form(0, 1, True)                                                    # 6: the action's own reason under the block's name
    refused(lambda: eng.compute_matrix_action_block(X, Y), SUP, "boundary-form")
    refused(lambda: eng.compute_matrix_action_block(X, Y), SUP, "matrix action on a block")
    eng.set_boundary_form(0, 1, False)
    eng.set_kernel(1)
    refused(lambda: eng.compute_matrix_action_block(X, Y), SUP, "IGXSetKernel")
    eng.set_kernel(0)
    eng.compute_matrix_action_block([X[0], X[0], X[1]], Y)                               # a refused call leaves nothing behind; entries of X may repeat
    eng.synchronize()
    assert "matrix action on a block" in eng.kernel_name()
