"""The vector algebra on IGXVec on the GPU (include/petiga_amd.h: IGXVecSet ... IGXVecNorm2; petiga_amd/csrc/krylov.hpp), every operation at
  8         one p = 1 element
  45        3 x 3 x 5 nodes, dof 1: an odd length, the scalar tail
  135       the same nodes at dof 3: odd again, several fields
  592704    40^3 elements at p = 2, dof 8: 296352 pairs over the capped grid of 256 workgroups x 512 threads = 131072 threads, so every
            thread takes two pairs and a part of them a third
Bounds, u = 2^-53: set, copy, scale exact; pointwise_divide correctly rounded (numpy's quotient, bit for bit); axpby
|y' - (a x + b y)| <= 2u (|a x| + |b y|) entry by entry against the expression in extended precision; dot |s - exact| <= gamma_n sum|x_i y_i|
with gamma_n = n u / (1 - n u), which holds for any summation order, against the exactly rounded sum (math.fsum) of the exact products
(each split into its rounded value and its rounding error); norm |s - sqrt(exact)| <= (gamma_n / 2 + gamma_n^2 + 2u) sqrt(exact): the same
bound through the square root, one rounding for the library's sqrt and one for the reference's.  Two calls give the same bits; on a rank
that holds ghost rows the sums run over its owned rows."""
import functools
import math

import numpy as np
import pytest

from krylov_ref import U_ROUND
from krylov_ref import exact_dot as _exact_dot
from krylov_ref import gamma as _gamma

pytestmark = pytest.mark.gpu

# name -> (dof, p, N)
LENGTHS = {"8": (1, 1, (1, 1, 1)), "45": (1, 1, (2, 2, 4)), "135": (3, 2, (1, 1, 3)), "592704": (8, 2, (40, 40, 40))}


@functools.lru_cache(maxsize=None)
def _engine(name):
    import petiga_amd as P
    dof, p, N = LENGTHS[name]
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_uniform(i, p, N[i])
    g.setup()
    return g


@functools.lru_cache(maxsize=None)
def _data(name):
    """(x, y, d) of the length: standard normal, and a divisor away from 0; made once, never written to"""
    n = int(name)
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    d = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    for a in (x, y, d):
        a.setflags(write=False)
    return x, y, d


@pytest.mark.parametrize("name", sorted(LENGTHS, key=int))
def test_set_copy_scale(name):
    g = _engine(name)
    x = _data(name)[0]
    v, w = g.create_vec(), g.create_vec()
    assert v.n == int(name)
    assert np.array_equal(v.fill(-2.75).get(), np.full(v.n, -2.75))
    assert np.array_equal(w.copy_from(v.set(x)).get(), x)
    assert np.array_equal(w.copy_from(w).get(), x)
    assert np.array_equal(w.scale(1.0 / 3.0).get(), (1.0 / 3.0) * x)
    assert np.array_equal(v.get(), x), "the source of a copy changed"


@pytest.mark.parametrize("name", sorted(LENGTHS, key=int))
def test_axpby(name):
    g = _engine(name)
    x, y, _ = _data(name)
    a, b = 0.7310585786300049, -1.6180339887498949
    xv, yv = g.create_vec().set(x), g.create_vec().set(y)
    got = yv.axpby(a, xv, b).get()
    L = np.longdouble
    ax, by = L(a) * x.astype(L), L(b) * y.astype(L)
    err, bound = np.abs(got.astype(L) - (ax + by)), 2 * U_ROUND * (np.abs(ax) + np.abs(by))
    print("axpby, n = %s: worst error / bound %.3f" % (name, float((err / bound).max())))
    assert np.all(err <= bound)
    assert np.array_equal(xv.get(), x)
    # b = 0: y = a x whatever y held
    yv.set(np.full(y.size, np.nan))
    assert np.array_equal(yv.axpby(a, xv, 0.0).get(), a * x)
    # y = y + y through the same vector
    assert np.array_equal(yv.set(y).axpby(1.0, yv, 1.0).get(), 2.0 * y)


@pytest.mark.parametrize("name", sorted(LENGTHS, key=int))
def test_pointwise_divide(name):
    g = _engine(name)
    x, _, d = _data(name)
    xv, dv, zv = g.create_vec().set(x), g.create_vec().set(d), g.create_vec()
    assert np.array_equal(zv.pointwise_divide(xv, dv).get(), x / d), "not the correctly rounded quotient"
    assert np.array_equal(xv.pointwise_divide(xv, dv).get(), x / d), "z = x differs"
    assert np.array_equal(dv.get(), d)


@pytest.mark.parametrize("name", sorted(LENGTHS, key=int))
def test_dot_and_norm(name):
    g = _engine(name)
    x, y, _ = _data(name)
    n = x.size
    xv, yv = g.create_vec().set(x), g.create_vec().set(y)
    s = xv.dot(yv)
    exact, mag = _exact_dot(x, y)
    print("dot, n = %d: |s - exact| = %.3e, bound %.3e" % (n, abs(s - exact), _gamma(n) * mag))
    assert abs(s - exact) <= _gamma(n) * mag
    assert xv.dot(yv) == s and yv.dot(xv) == s, "two calls differ"
    nrm = xv.norm()
    exact2, _ = _exact_dot(x, x)
    root = math.sqrt(exact2)
    bound = (_gamma(n) / 2 + _gamma(n) ** 2 + 2 * U_ROUND) * root
    print("norm, n = %d: |s - sqrt(exact)| = %.3e, bound %.3e" % (n, abs(nrm - root), bound))
    assert abs(nrm - root) <= bound
    assert xv.norm() == nrm and nrm == math.sqrt(xv.dot(xv))
    assert np.array_equal(xv.get(), x) and np.array_equal(yv.get(), y)


def test_vectors_of_two_engines_are_refused():
    import petiga_amd as P
    a, b = _engine("45").create_vec(), _engine("135").create_vec()
    for call in (lambda: a.copy_from(b), lambda: a.axpby(1.0, b, 1.0), lambda: a.dot(b), lambda: a.pointwise_divide(a, b)):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == 62


@pytest.mark.parametrize("dof,axis", [(1, 0), (3, 1), (2, 2)])
def test_sums_run_over_the_owned_rows(dof, axis):
    """two stand-alone engines of a 2-rank partition along `axis` (no communicator: nothing is exchanged): a vector of ones gives each rank's
    number of owned dofs, the two add up to the single-rank length, and a random pair gives the sum over the owned entries within the bound"""
    import petiga_amd as P
    N, p = (5, 4, 6), 2
    total = 0
    for r in range(2):
        g = P.IGX(3, dof)
        for i in range(3):
            g.axis_uniform(i, p, N[i])
        g.set_comm(2, r)
        g.set_processors(axis, 2)
        g.setup()
        v, w = g.create_vec(), g.create_vec()
        owned = v.indices(0, owned_only=True) >= 0
        assert 0 < owned.sum() and (r == 1 or owned.sum() < v.n), "the lower rank holds no ghost rows: the case tests nothing"
        ones = v.fill(1.0).dot(v)
        assert ones == owned.sum() and v.norm() == math.sqrt(owned.sum())
        total += ones
        rng = np.random.default_rng(7 + r)
        x, y = rng.standard_normal(v.n), rng.standard_normal(v.n)
        s = v.set(x).dot(w.set(y))
        exact, mag = _exact_dot(x[owned], y[owned])
        assert abs(s - exact) <= _gamma(int(owned.sum())) * mag and v.dot(w) == s
    assert total == (N[0] + p) * (N[1] + p) * (N[2] + p) * dof
