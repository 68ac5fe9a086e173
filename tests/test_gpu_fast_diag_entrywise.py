"""IGXFastDiagApply held entry by entry to the exact chain from the engine's own tables (tests/fast_diag_ref.py: ExactApplyRef), at the
shapes where fast_diag_contract<NT> (fast_diag.hpp) takes another path: every row-tile count NT of fd_row_tiles, a second row block
(gridDim.y = 2, i0 = 144) on each of the three axes, axis lengths on a tile limit and one past it, several chunks of 16 with a remainder
on the strided axes 1 and 2, per-field tables with more than one column tile per field, dof 5, 7 and 8 (dof 8 leaves the j-fast staging
of axis 0), a field without a free function, fewer than 16 columns, a zeroed mode at a multi-tile size, the tables of a user-set rule.

The bound is derived, not measured: with S the sum of the absolute values of all terms of an entry (the same chain on |R|, |U|, |1/den|),
u = 2^-53 and c = 2 (n0 + n1 + n2) + 8 (one rounding per term of each of the six contractions on FMA hardware, at most 8 for the double
denominator, its reciprocal and the scaling), |Z - Z_ref| <= c u S / (1 - c u) for any summation order; where S = 0 the engine's value is
exactly 0; the fixed rows equal R / count bit for bit.  Pure rounding sits far below the bound; a dropped term, a wrong table or a
misplaced tile moves an entry by about S / n.  Every case asserts the `row tiles a/b/c` of the kernel name and prints its worst ratio
in units of u S.

Worst |Z - Z_ref| / (u S) seen on an MI355X on the random R (the bound c in brackets): ladder a 0.89 (216), b 0.67 (358), c 0.67 (714);
two row blocks on axis 0, 1, 2: 0.67 each (546), over their seven unit vectors 15.9, 10.6 and 11.9; tile edges 16/17/32 0.04 (138),
256 0.48 (530), 257 0.36 (532); per-field tables 0.86 (84), 2.99 over 16 unit vectors; dof 5, 7, 8 with shared tables 0.66, 0.79, 0.82 and
with per-field tables 0.84, 0.75, 0.76 (66); four columns per field 0.74 (96); zeroed periodic mode 0.009 (136); graded axis 0.64 (122).
No case failed: the device half needed no change.  End to end at these lengths (tests/test_gpu_fast_diag.py, engine error over the numpy
restatement's, bound 8): 0.70, 1.13 and 0.87 with 258 elements on axis 0, 1 and 2, 0.56 at p = 3 (97,45,2); with the host eigen-solver
before its refinement step (host.cpp: refine_eigen) the same four gave 5.26, 10.08, 5.51 and 1.28."""
import numpy as np
import pytest

from fast_diag_ref import exact_case

pytestmark = pytest.mark.gpu

MIXED = [(0, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0)]


def _graded_knots():
    """p = 3, 34 distinct interior breakpoints graded towards 0, the twelfth a triple knot (C0): 40 functions"""
    t = (np.arange(1, 35) / 35.0) ** 1.7
    inner = np.concatenate([t[:11], [t[11]] * 3, t[12:]])
    return np.concatenate([[0.0] * 4, inner, [1.0] * 4])


def _wide(dof, per_field):
    return dict(p=(2, 2, 2), N=(16, 4, 3), dof=dof, faces=[(1, 0, dof - 1)] if per_field else [(0, 1, f) for f in range(dof)], alpha=0.25,
                beta=(1.0, 2.0, 0.5), tiles="2/1/1", tables="tables per field" if per_field else "fields share their tables")


def _two_blocks(axis):
    short = [3, 4]
    p, N = tuple(2 if d == axis else 1 for d in range(3)), tuple(258 if d == axis else short.pop(0) for d in range(3))
    return dict(p=p, N=N, faces=[(axis, 0, 0), ((axis + 1) % 3, 1, 0)], alpha=0.0, tiles="/".join("9" if d == axis else "1" for d in range(3)),
                units=axis)


# name -> the arguments of exact_case, the row tiles and table mode the kernel name must report, `units`: the axis unit vectors run along,
# `repeat`: two runs and the in-place run are compared bit for bit
CASES = {
    "ladder a, NT 3/4/2": dict(p=(2, 2, 2), N=(33, 48, 17), faces=MIXED, alpha=0.25, beta=(1.0, 2.0, 0.5), tiles="3/4/2"),
    "ladder b, NT 6/9/1": dict(p=(2, 3, 1), N=(68, 97, 4), faces=[(0, 0, 0), (1, 1, 0)], alpha=0.0, tiles="6/9/1"),
    "ladder c, NT 12/16/1": dict(p=(3, 2, 1), N=(147, 198, 2), faces=[(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)], alpha=0.0, tiles="12/16/1", repeat=True),
    "two row blocks on axis 0": _two_blocks(0),
    "two row blocks on axis 1": _two_blocks(1),
    "two row blocks on axis 2": _two_blocks(2),
    "tile edges 16, 17, 32": dict(p=(1, 1, 1), N=(15, 16, 31), faces=[(1, 0, 0)], alpha=0.0, tiles="1/2/2"),
    "tile edge 256": dict(p=(1, 1, 1), N=(255, 2, 1), faces=[(0, 1, 0)], alpha=0.0, tiles="16/1/1"),
    "tile edge 257": dict(p=(1, 1, 1), N=(256, 1, 2), faces=[(0, 1, 0)], alpha=0.0, tiles="9/1/1"),
    "per-field tables, many column tiles": dict(p=(2, 2, 2), N=(18, 7, 7), dof=3, faces=[(0, 0, 0), (1, 1, 0), (0, 1, 1), (2, 0, 1), (2, 1, 1)], alpha=0.5,
                                                beta=(1.0, 0.3, 4.0), tiles="2/1/1", tables="tables per field", units=0, repeat=True),
    "dof 5, shared tables": _wide(5, False),
    "dof 5, per-field tables": _wide(5, True),
    "dof 7, shared tables": _wide(7, False),
    "dof 7, per-field tables": _wide(7, True),
    "dof 8, shared tables": _wide(8, False),
    "dof 8, per-field tables": _wide(8, True),
    "four columns per field, a field without a free function": dict(p=(1, 1, 1), N=(1, 1, 39), dof=2, faces=[(0, 0, 1), (0, 1, 1)], alpha=0.5, tiles="1/1/3",
                                                                    tables="tables per field", empty_field=1),
    "one zeroed mode, periodic axes 0 and 2": dict(p=(2, 2, 2), N=(20, 6, 36), periodic=(True, False, True), alpha=0.0, tiles="2/1/3", nzeroed=1),
    "graded axis 1 with a triple knot, nqp = 5": dict(p=(3, 3, 3), N=(6, 0, 5), knots=(None, _graded_knots(), None), nqp=(None, 5, None), faces=[(1, 0, 0), (0, 1, 0)],
                                                    alpha=0.0, tiles="1/3/1"),
}
SEAMS = (0, 1, 15, 16, 143, 144, -2, -1)      # the chunk seam of 16 and the row-block seam of 144, and both ends


def _apply(eng, R, inplace=False):
    Rv = eng.create_vec().set(R)
    Zv = Rv if inplace else eng.create_vec()
    eng.fast_diag_apply(Rv, Zv)
    eng.synchronize()
    return Zv.get().copy()


def _hold(label, eng, ref, R):
    Z_ref, S = ref.apply(R)
    Z = _apply(eng, R)
    r, zeros = ref.ratio(Z, Z_ref, S)
    c = ref.rounding_constant()
    fixed = ~ref.free_mask()
    cnt = ref.counts[2][:, None, None] * ref.counts[1][None, :, None] * ref.counts[0][None, None, :]
    want = (R.reshape(ref.n[::-1] + [ref.dof]) / cnt[..., None]).reshape(-1)
    assert zeros, "%s: an entry whose terms are all zero is not exactly 0" % label
    assert ref.holds(Z, Z_ref, S), "%s: worst |Z - Z_ref| = %.3e u S, bound %d u S" % (label, r, c)
    assert np.array_equal(Z[fixed], want[fixed]), "%s: a fixed row is not R / count bit for bit" % label
    return Z, r


@pytest.mark.parametrize("name", list(CASES))
def test_apply_entry_by_entry(name):
    spec = dict(CASES[name])
    tiles, tables, units = spec.pop("tiles"), spec.pop("tables", None), spec.pop("units", None)
    repeat, nzeroed, empty = spec.pop("repeat", False), spec.pop("nzeroed", 0), spec.pop("empty_field", None)
    eng, ref, nz = exact_case(**spec)
    assert nz == ref.nzeroed == nzeroed, "the zeroed set of the reference is not the engine's"
    n, dof = ref.n, ref.dof
    R = np.random.default_rng(17).standard_normal(n[0] * n[1] * n[2] * dof)
    Z, worst = _hold(name, eng, ref, R)
    kernel = eng.kernel_name()
    assert "row tiles %s," % tiles in kernel, kernel
    if tables:
        assert tables in kernel, kernel
    if empty is not None:
        assert ref.tables[empty][0][1] == 0 and not ref.free_mask()[empty::dof].any()
    worst_unit, nunit = 0.0, 0
    if units is not None:
        free = ref.free_mask().reshape(n[::-1] + [dof])
        for f in range(dof):
            for node in sorted(set(s % n[units] for s in SEAMS if -n[units] <= s < n[units])):
                at = [n[0] // 2, n[1] // 2, n[2] // 2]
                at[units] = node
                if not free[at[2], at[1], at[0], f]:
                    continue
                E = np.zeros(n[::-1] + [dof])
                E[at[2], at[1], at[0], f] = 1.0
                _, r = _hold("%s, unit vector at node %d of axis %d, field %d" % (name, node, units, f), eng, ref, E.reshape(-1))
                worst_unit, nunit = max(worst_unit, r), nunit + 1
        assert nunit >= 4
    if repeat:
        assert np.array_equal(Z, _apply(eng, R)), "two runs differ"
        assert np.array_equal(Z, _apply(eng, R, inplace=True)), "Apply(R, R) differs from Apply(R, Z)"
    print("%s: n = %s, dof %d, %d dofs: worst |Z - Z_ref| = %.3f u S on a random R%s; bound %d u S; %s"
          % (name, n, dof, R.size, worst, ", %.3f u S over %d unit vectors" % (worst_unit, nunit) if nunit else "", ref.rounding_constant(), kernel))
