"""The exact reference of IGXFastDiagApply (tests/fast_diag_ref.py: ExactApplyRef) without a GPU: the chain in long double from the
engine's own tables, with the entry-wise rounding bound c u S / (1 - c u), c = 2 (n0 + n1 + n2) + 8, that tests/test_gpu_fast_diag_entrywise.py
holds the device half to.  Here: it agrees with the numpy restatement (scipy's eigenpairs) on a small mixed case, a plain double
evaluation of the same chain stays inside the bound, and the bound notices each structural fault it is meant to notice."""
import copy

import numpy as np
import pytest

from fast_diag_ref import ExactApplyRef, FastDiagRef, axis_matrices, exact_case, fixed_faces, uniform_knots

# two fields with different faces, anisotropic beta, three different axis lengths (9, 7, 6 functions)
P_, N_, DOF, FACES, ALPHA, BETA = (2, 3, 2), (7, 4, 4), 2, [(0, 0, 0), (1, 1, 1), (2, 0, 1), (2, 1, 1)], 0.5, (1.0, 0.3, 4.0)


@pytest.fixture(scope="module")
def case():
    eng, ref, nz = exact_case(P_, N_, DOF, FACES, ALPHA, BETA)
    R = np.random.default_rng(11).standard_normal(int(np.prod(ref.n)) * DOF)
    Z_ref, S = ref.apply(R)
    return ref, nz, R, Z_ref, S


def _double_chain(ref, R):
    """the engine's arithmetic restated in plain double: what the bound must admit"""
    R = np.asarray(R).reshape(ref.n[::-1] + [ref.dof])
    Z = R / (ref.counts[2][:, None, None] * ref.counts[1][None, :, None] * ref.counts[0][None, None, :])[..., None]
    for f in range(ref.dof):
        (a0, m0, _, U0), (a1, m1, _, U1), (a2, m2, _, U2) = ref.tables[f]
        box = (slice(a2, a2 + m2), slice(a1, a1 + m1), slice(a0, a0 + m0), f)
        T = np.einsum("kji,kc,jb,ia->cba", R[box], U2, U1, U0) * ref.recip[f].astype(np.float64)
        Z[box] = np.einsum("cba,kc,jb,ia->kji", T, U2, U1, U0)
    return Z.reshape(-1)


def test_agrees_with_the_numpy_restatement(case):
    ref, nz, R, Z_ref, S = case
    axes = [axis_matrices(uniform_knots(P_[d], N_[d]), P_[d]) for d in range(3)]
    old = FastDiagRef(axes, DOF, fixed_faces(DOF, FACES), ALPHA, list(BETA))
    assert nz == ref.nzeroed == old.nzeroed == 0
    assert np.array_equal(ref.free_mask(), old.free_mask())
    Zn = old.apply(R)
    assert np.abs(Zn - Z_ref.astype(np.float64)).max() <= 1e-12 * np.abs(Zn).max()
    fixed = ~ref.free_mask()
    assert fixed.any() and np.array_equal(Z_ref.astype(np.float64)[fixed], Zn[fixed])


def test_a_double_evaluation_is_inside_the_bound(case):
    ref, _, R, Z_ref, S = case
    Z = _double_chain(ref, R)
    r, zeros = ref.ratio(Z, Z_ref, S)
    print("double chain: worst |Z - Z_ref| = %.3f u S; bound %d u S" % (r, ref.rounding_constant()))
    assert zeros and ref.holds(Z, Z_ref, S) and r < 2.0


def _perturbed(ref, change):
    t = copy.deepcopy(ref.tables)
    change(t)
    return ExactApplyRef(t, ref.n, ref.dof, ref.counts, ref.alpha, ref.beta)


def _scale_last_entry(t):
    U = t[0][0][3]
    U[-1, -1] *= 1 + 1e-9


def _drop_last_j(t):
    t[1][1][3][-1, :] = 0.0


def _field_one_gets_field_zero(t):
    t[1] = copy.deepcopy(t[0])


@pytest.mark.parametrize("change", [_scale_last_entry, _drop_last_j, _field_one_gets_field_zero], ids=lambda c: c.__name__.strip("_"))
def test_the_bound_notices(case, change):
    """each fault is put into a copy of the reference; the faulty result must fall outside the bound of the true one"""
    ref, _, R, Z_ref, S = case
    bad = _perturbed(ref, change)
    if change is _field_one_gets_field_zero:      # (the free ranges differ: evaluate the wrong tables the way a wrong kernel would)
        Zb = _double_chain(bad, R)
    else:
        Zb = bad.apply(R)[0].astype(np.float64)
    r, _ = ref.ratio(Zb, Z_ref, S)
    print("%s: %.3e u S against a bound of %d u S" % (change.__name__, r, ref.rounding_constant()))
    assert not ref.holds(Zb, Z_ref, S)


def test_zeroed_modes_and_an_empty_field():
    """alpha = 0 without faces zeroes the constant of each field; a field fixed at both ends of a two-function axis has m = 0 and is
    R / count everywhere"""
    eng, ref, nz = exact_case((1, 1, 1), (1, 1, 5), dof=2, faces=[(0, 0, 1), (0, 1, 1)])
    assert ref.tables[1][0][:2] == (1, 0)
    assert nz == ref.nzeroed == 1
    R = np.random.default_rng(2).standard_normal(2 * 2 * 6 * 2)
    Z_ref, S = ref.apply(R)
    cnt = (ref.counts[2][:, None, None] * ref.counts[1][None, :, None] * ref.counts[0][None, None, :])
    assert np.array_equal(Z_ref.reshape(6, 2, 2, 2)[..., 1].astype(np.float64), R.reshape(6, 2, 2, 2)[..., 1] / cnt)
    assert ref.holds(_double_chain(ref, R), Z_ref, S)
