"""The matrix-free actions (IGXComputeMatrixAction / JacobianAction / IJacobianAction: vec_sumfact<..., ACTION = true>) against the long
double references, ENTRY BY ENTRY and ROW BY ROW: |Y - R| <= c u S with the project's constants (C_ID on the identity geometry, C_MAP on
an affine map; calibrated on the CPU oracle by test_tensor_reference.py and test_pointwise_reference.py).

test_gpu_matrix_action.py compares with the oracle's matrix times one standard-normal X at 1e-12 / 1e-11 of max_i S_i: a wrong
contribution to a row whose own S_i is small (a corner row, a short span of a graded mesh, a far-band coupling) or one gathered from the
wrong column with a similar magnitude passes it.  Here

  * the operator is recovered from the action one column at a time.  The columns are coloured so that no row couples with two columns
    of one colour (pointwise_ref.colouring); per colour X holds a distinct amplitude in +-[0.5, 2] on each probed column, so a value
    gathered from the wrong column changes the result.  Every row coupled with a probed column j must satisfy
    |Y_i - a_j R_ij| <= c u |a_j| S_ij (S_ij = 0: exactly), every other row must be exactly 0.0.  The entries R_ij come from
    tensor_ref.TensorRef (Poisson, elasticity) and pointwise_ref (Bratu at a VARYING state);
  * every case of test_gpu_matrix_action.py that the references cover -- Poisson and elasticity, Bratu, Cahn-Hilliard on the identity
    geometry -- and graded-mesh variants are checked row by row, |Y_i - R_i| <= c u S_i, with a standard-normal X and with an X whose
    magnitudes spread over 10^-6 ... 10^6.

The warped poly / nurbs cases and NS-VMS have no such reference and keep the oracle check of test_gpu_matrix_action.py only.

Worst ratios on an MI355X (u S): the recovered entries 15.4 on the identity geometry (Bratu Jacobian, p = 3 graded) and 19.7 on a map
(Poisson p = 3, constant NURBS weights); row by row 8.5 (Bratu IJacobian p = 3 graded, the wide X), 4.4 on a map, Cahn-Hilliard 0.45 on
the free rows and 2.6 on a Dirichlet row; on two ranks 3.4 (Poisson) and 0.06 (Cahn-Hilliard)."""
import numpy as np
import pytest

import pointwise_ref as PW
import tensor_ref as T
import test_gpu_matrix_action as MA
from test_pointwise_reference import wide

pytestmark = pytest.mark.gpu

LD = T.LD
LAM, SHIFT, CH_SHIFT = 3.5, 4.0, 250.0
CH, EL = MA.CH, MA.EL
_k = T.graded_knots
G3 = [_k(3, 6, 100.0), _k(3, 5, 0.01), _k(3, 6, 100.0)]
G2 = [_k(2, 5, 100.0), _k(2, 4, 0.01), _k(2, 3, 1000.0)]          # an odd element count: (5, 4, 3) spans


def _bcs(dof=1, kind="all"):
    return {(d, s, f): 0.2 + 0.1 * d - 0.15 * s + 0.05 * f for d in range(3) for s in range(2) for f in range(dof)
            if kind == "all" or (d + s + f) % 2 == 0}


BC3 = {(0, 0, 0): 0.2, (1, 1, 0): -0.1, (2, 0, 0): 0.3}
EL_BCS = {(0, 0, 0): 0.0, (0, 0, 1): 0.5, (0, 0, 2): -0.25, (2, 1, 0): 1.0, (1, 0, 2): 0.75}

# name: (setup_case keywords, form, driver)
PROBE = {
    "poisson-p3-graded": (dict(dof=1, p=3, N=0, knots=G3, bcs=_bcs()), "poisson", "matrix"),
    "poisson-p2-graded-odd": (dict(dof=1, p=2, N=0, knots=G2, bcs=_bcs(kind="some")), "poisson", "matrix"),
    "poisson-p2-periodic": (dict(dof=1, p=2, N=[6, 4, 5], periodic=[True, False, True], bcs={(1, 0, 0): 2.0}), "poisson", "matrix"),
    "poisson-mixed-degrees": (dict(dof=1, p=[2, 3, 2], N=[4, 3, 5], nqp=[3, 4, 4], bcs={(1, 0, 0): 1.0}), "poisson", "matrix"),
    "poisson-p3-C1": (dict(dof=1, p=3, N=[4, 4, 3], C=[1, 2, 2], bcs=_bcs(kind="some")), "poisson", "matrix"),
    "poisson-p3-affine": (dict(dof=1, p=3, N=[5, 4, 4], geometry="affine", seed=1, bcs=_bcs()), "poisson", "matrix"),
    "poisson-p3-rational": (dict(dof=1, p=3, N=[4, 4, 3], geometry="rational", seed=3, bcs=BC3), "poisson", "matrix"),
    "elasticity-p2": (dict(dof=3, p=2, N=[4, 3, 3], bcs=EL_BCS), "elasticity", "matrix"),
    "bratu-jacobian-p3-graded": (dict(dof=1, p=3, N=0, knots=G3, bcs=_bcs()), "bratu", "jacobian"),
    "bratu-ijacobian-p3-graded": (dict(dof=1, p=3, N=0, knots=G3, bcs=_bcs(kind="some")), "bratu", "ijacobian"),
    "bratu-jacobian-p2-odd": (dict(dof=1, p=2, N=0, knots=G2, bcs=_bcs(kind="some")), "bratu", "jacobian"),
    "bratu-ijacobian-p2-odd": (dict(dof=1, p=2, N=[5, 4, 3], bcs=_bcs()), "bratu", "ijacobian"),
}


def _from_matrix_action(name):
    form, dof, p, N, kw, geo, bcs, _ = MA.CASES[name]
    assert geo is None
    d = dict(dof=dof, p=list(p) if isinstance(p, tuple) else p, N=list(N), bcs={(a, s, f): v for a, s, f, v in bcs}, **kw)
    return d, form, {"poisson": "matrix", "elasticity": "matrix", "bratu": "jacobian", "cahnhilliard": "ijacobian"}[form]


# the covered cases of test_gpu_matrix_action.py, and graded / Bratu IJacobian / affine variants
ROWWISE = {name: _from_matrix_action(name) for name in
           ("poisson-p3-dirichlet", "poisson-p2-odd", "poisson-mixed-degrees", "poisson-p2-c0-knots", "poisson-p2-periodic", "ch-p2",
            "ch-p2-dirichlet", "bratu-p3", "elasticity-p3")}
ROWWISE.update({
    "poisson-p3-graded": PROBE["poisson-p3-graded"],
    "poisson-p3-affine": PROBE["poisson-p3-affine"],
    "elasticity-p3-affine": (dict(dof=3, p=3, N=[4, 3, 3], geometry="affine", seed=4, bcs=EL_BCS), "elasticity", "matrix"),
    "bratu-p3-graded": PROBE["bratu-jacobian-p3-graded"],
    "bratu-ijacobian-p3-graded": PROBE["bratu-ijacobian-p3-graded"],
    "bratu-p2-affine": (dict(dof=1, p=2, N=[5, 4, 3], geometry="affine", seed=5, bcs=BC3), "bratu", "jacobian"),
    "ch-p2-graded": (dict(dof=1, p=2, N=0, knots=G2), "cahnhilliard", "ijacobian"),
    "ch-p2-graded-dirichlet": (dict(dof=1, p=2, N=0, knots=G2, bcs={(0, 0, 0): 0.6, (1, 1, 0): 0.61, (2, 0, 0): 0.65}), "cahnhilliard", "ijacobian"),
})


def _state(form, n):
    rng = np.random.default_rng(29)
    V = rng.standard_normal(n)
    U = 0.63 + 0.05 * (2 * rng.random(n) - 1) if form == "cahnhilliard" else 0.3 * rng.standard_normal(n)
    return U, V


class _Action:
    """One engine with its form set and the state on the device; __call__(X) -> Y on the host."""

    def __init__(self, kw, form, driver):
        self.orc, self.eng, self.A = T.setup_case(dim=3, engine=True, **kw)
        eng = self.eng
        eng.set_form(form, {"poisson": (), "elasticity": EL, "bratu": (LAM,), "cahnhilliard": CH}[form])
        self.n = self.orc.global_size()
        self.form, self.driver, self.p = form, driver, kw["p"]
        self.U, self.V = _state(form, self.n)
        self.Uv, self.Vv, self.Xv, self.Y = (eng.create_vec() for _ in range(4))
        self.Uv.set(self.U)
        self.Vv.set(self.V)
        self.Y.set(np.full(self.n, np.nan))                 # the driver zeroes Y itself
        self.shift = CH_SHIFT if form == "cahnhilliard" else SHIFT
        self.c = T.C_MAP if self.A is not None else T.C_ID

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

    def check_kernel(self):
        kn = self.eng.kernel_name()
        assert "vec_sumfact" in kn and "action" in kn, kn
        degrees = self.p if isinstance(self.p, list) else [self.p] * 3
        assert ("two elements per wavefront" in kn) == all(d <= 2 for d in degrees), kn
        return kn


def _references(act, kw):
    """(the TensorRef that names and fixes the entries, entries(rows, cols) -> (R, S), action(X) -> (R, S))"""
    bcs = kw.get("bcs")
    if act.form in ("poisson", "elasticity"):
        ref = T.reference(act.orc, 3, T.poisson(3) if act.form == "poisson" else T.elasticity(*EL), A=act.A, bcs=bcs, driver="system")
        return ref, ref.entries, ref.action
    pw = PW.PointwiseRef(act.orc, A=act.A, bcs=bcs)
    if act.form == "bratu":
        shift = SHIFT if act.driver == "ijacobian" else 0.0
        return (pw.tref, lambda r, c: pw.bratu_entries(LAM, act.U, r, c, shift), lambda X: pw.bratu_action(LAM, act.U, X, shift))
    return pw.tref, None, lambda X: pw.ch_action(CH, CH_SHIFT, act.U, X)


@pytest.mark.parametrize("name", list(PROBE))
def test_operator_recovered_from_the_action(name):
    kw, form, driver = PROBE[name]
    act = _Action(kw, form, driver)
    ref, entries, _ = _references(act, kw)
    n, dof = act.n, kw["dof"]
    rows = np.arange(n)
    cols, valid = ref.stencil(rows)
    rr, cc = np.nonzero(valid)
    er, ec = rows[rr], cols[rr, cc]
    R, S = entries(er, ec)
    fx = ref.fixed(er)[0] if kw.get("bcs") else np.zeros(er.size, dtype=bool)
    diag = fx & (er == ec)
    S[diag] = R[diag]                                    # a fixed row: m a_i, added once per element -- rounded, bound m |a_i|
    colour, ncol, per_axis = PW.colouring(ref.tabs, dof)
    rng = np.random.default_rng(17)
    amp = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    order = np.argsort(colour[ec], kind="stable")
    start = np.searchsorted(colour[ec][order], np.arange(ncol + 1))
    worst, probed = 0.0, 0
    for k in range(ncol):
        Y = act(np.where(colour == k, amp, 0.0))
        if k == 0:
            kn = act.check_kernel()
        e = order[start[k]:start[k + 1]]
        assert np.unique(er[e]).size == e.size         # no row couples with two columns of this colour
        a = amp[ec[e]]
        worst = max(worst, T.compare_entrywise((er[e], ec[e], Y[er[e]]), LD(1) * a * R[e], np.abs(a) * S[e], act.c, ref,
                                               "%s colour %d" % (name, k), pattern=False))
        rest = np.ones(n, dtype=bool)
        rest[er[e]] = False
        bad = np.flatnonzero(rest & ~(Y == 0.0))
        assert bad.size == 0, "%s colour %d: row %d couples with no probed column and is %r" % (name, k, bad[0], Y[bad[0]])
        probed += e.size
    assert probed == er.size and ncol == int(np.prod(per_axis)) * dof
    print("%-28s %-70s %d colours %s, %d entries, worst %.2f u S (c = %g)" % (name, kn[:70], ncol, per_axis, probed, worst, act.c))


@pytest.mark.parametrize("name", list(ROWWISE))
def test_action_row_by_row(name):
    kw, form, driver = ROWWISE[name]
    act = _Action(kw, form, driver)
    ref, _, action = _references(act, kw)
    worst = {}
    for tag, X in (("X", np.random.default_rng(31).standard_normal(act.n)), ("Xwide", wide(act.n))):
        Y = act(X)
        kn = act.check_kernel()
        worst[tag] = PW.compare_rows(Y, *action(X), act.c, ref, "%s %s" % (name, tag))
    print("%-28s %-70s worst %s u S (c = %g)" % (name, kn[:70], "  ".join("%s %.2f" % kv for kv in worst.items()), act.c))
