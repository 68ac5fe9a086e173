"""Calibrates tests/transfer_ref.py, the long double reference of IGXTransfer, without the library and without a GPU: its two constructions
agree, the refined functions reproduce the coarse ones at 400 points per case (scipy's BSpline is the witness), every row has the
properties the kernels rely on, a periodic axis folds onto the dense evaluation of the wrapped functions, and five deliberately wrong
constructions are caught by the function-equality check.

Bounds.  Function equality compares sums of at most p + 1 products of numbers in [0, 1] evaluated in double by scipy on both sides: the
gap of a right table is a few u; GAP = 16 u is 4 x the worst seen over the cases here (4.0 u).  A wrong table moves
a function by a coefficient's size: the teeth test asks for a gap above 1e-3.  Boehm's chain rounds once per insertion and level: the two
constructions are held to (4 + number of inserted knots) (p + 1) u per entry."""
import numpy as np
import pytest

import transfer_ref as TR

U_RND = TR.U_RND
GAP = 16 * U_RND


def _cluster(U, p, k=10):
    """ten knots inside the second span"""
    b = np.unique(U)
    return TR.insert(U, p, b[1] + (b[2] - b[1]) * (np.arange(1, k + 1) / (k + 1.5)) ** 2)


def _raise_mult(U, p, upto):
    """the interior knots raised to multiplicity `upto`"""
    inner = np.unique(U)[1:-1]
    have = {v: int(np.sum(U == v)) for v in inner}
    return TR.insert(U, p, np.concatenate([[v] * max(upto - have[v], 0) for v in inner]))


def cases():
    """(name, p, Uc, Uf, periodic)"""
    out = []
    for p in range(1, 8):
        Uc = TR.uniform_knots(p, 4)
        out.append(("p%d-2x" % p, p, Uc, TR.uniform_knots(p, 8), False))
        out.append(("p%d-3x" % p, p, Uc, TR.uniform_knots(p, 12), False))
        out.append(("p%d-cluster" % p, p, Uc, _cluster(Uc, p), False))
        out.append(("p%d-c0" % p, p, Uc, _raise_mult(TR.uniform_knots(p, 8), p, p), False))
        out.append(("p%d-same" % p, p, Uc, Uc.copy(), False))
        if p > 1:
            out.append(("p%d-mult2-coarse" % p, p, _raise_mult(Uc, p, 2), _raise_mult(TR.uniform_knots(p, 8), p, min(p, 3)), False))
        out.append(("p%d-periodic" % p, p, TR.uniform_knots(p, p + 3, periodic=True), TR.uniform_knots(p, 2 * (p + 3), periodic=True), True))
        out.append(("p%d-periodic-small" % p, p, TR.uniform_knots(p, p + 1, periodic=True), TR.uniform_knots(p, 4 * (p + 1), periodic=True), True))
    out.append(("p2-periodic-c0", 2, TR.uniform_knots(2, 4, C=0, periodic=True), TR.uniform_knots(2, 8, C=0, periodic=True), True))
    return out


CASES = cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,p,Uc,Uf,periodic", CASES, ids=IDS)
def test_function_equality_and_row_properties(name, p, Uc, Uf, periodic):
    T = TR.matrix_rowwise(p, Uc, Uf, periodic)
    nf, nc = T.shape
    assert (nf, nc) == (TR.nnp_of(p, Uf, periodic), TR.nnp_of(p, Uc, periodic))
    gap = TR.function_gap(p, Uc, Uf, T, periodic, npts=400)
    print("%s: %d x %d, function gap %.1f u" % (name, nf, nc, gap / U_RND))
    assert gap <= GAP
    # rows: non-negative, of sum 1, at most p + 1 consecutive non-zeros, the first column non-decreasing by steps of at most 1
    assert np.all(T >= 0) and np.max(np.abs(T.sum(axis=1) - 1)) <= 2 * (p + 1) * U_RND
    first, count, band = TR.bands(T, periodic)
    assert count.max() <= p + 1 and band.shape[1] <= p + 1
    if nc > p + 1 or not periodic:
        step = np.diff(first) % nc if periodic else np.diff(first)
        assert np.all((step == 0) | (step == 1)), (first, step)
    if not periodic:
        assert first[0] == 0 and count[0] == 1 and T[0, 0] == 1 and first[-1] == nc - 1 and count[-1] == 1 and T[-1, -1] == 1      # clamped ends: unit rows
    if name.endswith("-same"):
        assert np.array_equal(T, np.eye(nc))                                                                                  # exactly 1.0, exactly 0.0
    if name.endswith("cluster"):
        print("  longest column: %d non-zeros" % int((T != 0).sum(axis=0).max()))
        assert (T != 0).sum(axis=0).max() >= 8      # a column can hold any number of non-zeros: the restriction's rows are unbounded


@pytest.mark.parametrize("name,p,Uc,Uf,periodic", [c for c in CASES if not c[4]], ids=[c[0] for c in CASES if not c[4]])
def test_the_two_constructions_agree(name, p, Uc, Uf, periodic):
    T, B = TR.matrix_rowwise(p, Uc, Uf), TR.matrix_by_insertion(p, Uc, Uf)
    assert T.shape == B.shape
    ninserted = len(Uf) - len(Uc)
    worst = float(np.max(np.abs(T - B)))
    print("%s: %d inserted knots, the constructions differ by %.2f u at the most" % (name, ninserted, worst / U_RND))
    assert worst <= (4 + ninserted) * (p + 1) * U_RND
    assert np.array_equal(T != 0, B != 0)


def test_periodic_folding_against_wrapped_functions():
    """the folded table against a dense evaluation: sum over the period's images of the unwrapped functions, on both sides"""
    for p, N in ((2, 3), (2, 5), (3, 4), (3, 6), (5, 6)):
        Uc, Uf = TR.uniform_knots(p, N, periodic=True), TR.uniform_knots(p, 3 * N, periodic=True)
        T = TR.matrix_rowwise(p, Uc, Uf, True)
        assert T.shape == (3 * N, N)
        x = np.linspace(0, 1, 97)[:-1]
        Bc, Bf = TR.basis(p, Uc, x, True), TR.basis(p, Uf, x, True)
        assert np.max(np.abs(Bc.sum(axis=1) - 1)) <= GAP and np.max(np.abs(Bf.sum(axis=1) - 1)) <= GAP      # the wrapped functions are a partition of unity
        assert np.max(np.abs(Bc - Bf @ T.astype(np.float64))) <= GAP
        assert np.max(np.abs(T.sum(axis=0) - 3)) <= 16 * U_RND                                          # uniform 3x: every column sums to 3


TEETH = [("first", 3, False), ("left", 2, False), ("multiplicity", 3, False), ("unfolded", 2, True), ("transpose", 3, False)]


@pytest.mark.parametrize("wrong,p,periodic", TEETH, ids=[t[0] for t in TEETH])
def test_wrong_constructions_are_caught(wrong, p, periodic):
    if wrong == "left":               # fine knots ON coarse knots, where the span rule matters: the coarse knots raised to C0 in the fine vector
        Uc = TR.uniform_knots(p, 4)
        Uf = _raise_mult(TR.uniform_knots(p, 8), p, p)
    elif wrong == "multiplicity":
        Uc = _raise_mult(TR.uniform_knots(p, 4), p, 2)
        Uf = _raise_mult(TR.uniform_knots(p, 8), p, 2)
    elif wrong == "transpose":        # (a square nested pair is the identity, its own transpose: the rectangular table's transpose is cut
        Uc = TR.uniform_knots(p, 4)   # and padded to the table's shape below)
        Uf = TR.uniform_knots(p, 8)
    else:
        Uc, Uf = TR.uniform_knots(p, 5, periodic=periodic), TR.uniform_knots(p, 10, periodic=periodic)
    right = TR.matrix_rowwise(p, Uc, Uf, periodic)
    assert TR.function_gap(p, Uc, Uf, right, periodic) <= GAP
    bad = TR.matrix_rowwise(p, Uc, Uf, periodic, wrong=wrong)
    if wrong == "transpose":
        pad = np.zeros(right.shape, dtype=TR.LD)
        r, c = min(bad.shape[0], pad.shape[0]), min(bad.shape[1], pad.shape[1])
        pad[:r, :c] = bad[:r, :c]
        bad = pad
    assert bad.shape == right.shape
    gap = TR.function_gap(p, Uc, Uf, bad, periodic)
    print("%s: the wrong table's function gap %.3g" % (wrong, gap))
    assert gap > 1e-3
