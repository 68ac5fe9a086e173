"""IGXMatMultBlock on the GPU (include/petiga_amd.h; petiga_amd/csrc/mat_ops.hpp, mat_mult_block): the assembled block-CSR
matrix times a block of vectors, on the small cases of tests/test_gpu_mat_mult.py (its CASES and its _assembled), under both index variants.
  bit contract    for nx in {1, 2, NC - 1, NC, NC + 1, 16, 17, 48} (NC the case's full chunk: a full chunk, a chunk edge and a remainder all
                  occur, asserted from the chunk plan) every column of Mat.mult_block equals Mat.mult of that column bit for bit
                  (torch.equal); a case with an odd block size must hold rows of each start parity
  entry by entry  every row of one column satisfies |y - y_ref| <= gamma_n sum |a| |x| against the np.longdouble product of the engine's own
                  matrix: the bound of tests/test_gpu_mat_mult.py, derived, which the bit test carries to every other column
  place and company   a column's bits are the same at three places in the block and under a permutation of the block; Y poisoned with NaN on
                  entry comes back finite; a NaN column of X makes exactly its own Y column NaN and the others keep their bits; a vector
                  twice in X gives two equal results; two block calls agree bit for bit
  figures         last_launches equals the chunk count of the plan; the kernel name carries bs, lanes per row, index variant and NC
  refusals        those that need vectors, in the header's order
Every test prints what it sees before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import krylov_ref as K
import mat_block_cases as MB
import mat_ops_ref as R
import test_gpu_mat_mult as MM

pytestmark = pytest.mark.gpu

ARG_WRONG, SUP, OUTOFRANGE = 62, 56, 63
NMAX = MB.ACTION_BLOCK_MAX


def _sizes(bs):
    nc = MB.full_width(bs)
    return sorted({1, 2, nc - 1, nc, nc + 1, 16, 17, NMAX} - {0})


def _columns(eng, n, count, seed=71):
    rng = np.random.default_rng(seed)
    return [eng.create_vec().set(rng.standard_normal(n)) for _ in range(count)]


def _t(v):
    return torch.from_numpy(v.get().copy())


@pytest.mark.parametrize("index", ["tables", "bcolidx"])
@pytest.mark.parametrize("name", sorted(MM.CASES))
def test_every_column_is_mat_mult_of_that_column_bit_for_bit(name, index, monkeypatch):
    import petiga_amd as P
    monkeypatch.setenv("IGX_MATMULT_INDEX", "0" if index == "tables" else "1")      # (read when the IGX is created)
    eng, A = MM._assembled(name)
    bs, n = A.bs, A.nbrows * A.bs
    nc = MB.full_width(bs)
    rp = A.host()[0]
    start_odd = (rp[:-1] * bs * bs) % 2 == 1
    assert (~start_odd).any() and (start_odd.any() if bs % 2 else not start_odd.any()), "the case lacks a row of each start parity"
    X = _columns(eng, n, NMAX)
    single = []
    y = eng.create_vec()
    for x in X:
        A.mult(x, y)
        single.append(_t(y))
    kinds = set()
    Y = [eng.create_vec() for _ in range(NMAX)]
    for nx in _sizes(bs):
        plan = P.mat_mult_block_plan(bs, nx)
        assert plan == MB.plan(bs, nx)
        kinds |= {"full" if k == nc else "single" if k == 1 else "narrower" for k in plan}
        for v in Y[:nx]:
            v.set(np.full(n, np.nan))                      # NaN in Y on entry does not survive
        eng.set_timing(True)
        A.mult_block(X[:nx], Y[:nx])
        eng.synchronize()
        kname, launches = eng.kernel_name(), eng.last_timing()[2]
        eng.set_timing(False)
        got = [_t(v) for v in Y[:nx]]
        same = [torch.equal(got[j], single[j]) for j in range(nx)]
        print("%s, %s, nx = %d: plan %s, %d launches, %d of %d columns equal Mat.mult's bits; %s" % (name, index, nx, plan, launches, sum(same), nx, kname))
        assert all(torch.isfinite(g).all() for g in got)
        assert all(same), [j for j in range(nx) if not same[j]]
        assert launches == len(plan)
        lanes = kname.split(", ")[1]
        assert kname == "mat_mult_block(bs=%d, %s, columns from %s, NC=%d)" % (bs, lanes, "the axis tables" if index == "tables" else "bcolidx", nc), kname
        assert lanes == "one wavefront per row" or lanes in ("8 lanes per row", "16 lanes per row", "32 lanes per row")
    assert kinds == {"full", "single", "narrower"} if nc > 2 else kinds == {"full", "single"}, kinds
    # the lanes per row are the single product's
    A.mult(X[0], y)
    assert eng.kernel_name() == "mat_mult(bs=%d, %s, columns from %s)" % (bs, lanes, "the axis tables" if index == "tables" else "bcolidx")


@pytest.mark.parametrize("name", sorted(MM.CASES))
def test_every_row_of_one_column_within_the_bound_of_its_sum(name):
    eng, A = MM._assembled(name)
    rp, ci, val, x, y_ref, S, n = MM._reference(A)
    nx = MB.full_width(A.bs) + 1
    X = _columns(eng, x.size, nx)
    X[nx - 2].set(x)                                        # the last column of the full chunk
    Y = [eng.create_vec() for _ in range(nx)]
    A.mult_block(X, Y)
    eng.synchronize()
    got = Y[nx - 2].get()
    bound = np.array([K.gamma(int(k)) for k in n], dtype=np.longdouble) * S
    err = np.abs(got.astype(np.longdouble) - y_ref)
    print("%s: column %d of %d, %d rows, max |y - y_ref| / bound = %.3f" % (name, nx - 2, nx, A.nbrows, float((err / np.maximum(bound, np.longdouble(1e-300))).max())))
    assert np.isfinite(got).all() and np.all(err <= bound)


@pytest.mark.parametrize("name", ["poisson-p2", "elasticity", "nsvms-nurbs", "poisson-p3", "dim1"])
def test_place_company_and_repeats(name):
    eng, A = MM._assembled(name)
    bs, n = A.bs, A.nbrows * A.bs
    nc = MB.full_width(bs)
    nx = 2 * nc + 3                                         # two full chunks and a remainder of a narrower chunk and a single column
    X = _columns(eng, n, nx, seed=5)
    Y = [eng.create_vec() for _ in range(nx)]
    A.mult_block(X, Y)
    base = [_t(v) for v in Y]
    # two block calls agree bit for bit
    Y2 = [eng.create_vec() for _ in range(nx)]
    A.mult_block(X, Y2)
    assert all(torch.equal(_t(Y2[j]), base[j]) for j in range(nx))
    # a column at three places: first of a full chunk, inside the second chunk, the last single column
    for place in (0, nc + 1, nx - 1):
        order = list(range(nx))
        order[0], order[place] = order[place], order[0]
        A.mult_block([X[k] for k in order], Y2)
        assert torch.equal(_t(Y2[place]), base[0]), place
    # a permutation of the block
    perm = np.random.default_rng(3).permutation(nx)
    A.mult_block([X[k] for k in perm], Y2)
    moved = [torch.equal(_t(Y2[j]), base[perm[j]]) for j in range(nx)]
    print("%s: nx = %d, plan %s; permutation %s: %d columns keep their bits" % (name, nx, MB.plan(bs, nx), perm.tolist(), sum(moved)))
    assert all(moved)
    # a NaN column of X makes exactly its own column NaN
    for bad in (1, nc, nx - 1):
        Xn = list(X)
        Xn[bad] = eng.create_vec().set(np.full(n, np.nan))
        A.mult_block(Xn, Y2)
        for j in range(nx):
            got = _t(Y2[j])
            assert torch.isnan(got).all() if j == bad else torch.equal(got, base[j]), (bad, j)
    # a vector twice in X
    Xr = list(X)
    Xr[nc] = X[0]
    Xr[nx - 1] = X[0]
    A.mult_block(Xr, Y2)
    assert torch.equal(_t(Y2[nc]), base[0]) and torch.equal(_t(Y2[nx - 1]), base[0]) and torch.equal(_t(Y2[0]), base[0])


def test_refusals_that_need_vectors():
    import petiga_amd as P
    eng, A = MM._assembled("elasticity")
    X, Y = [eng.create_vec() for _ in range(3)], [eng.create_vec() for _ in range(3)]

    def refused(call, code, *words):
        with pytest.raises(P.IGXError) as e:
            call()
        print(e.value)
        assert e.value.code == code and "IGXMatMultBlock" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    other, _ = MM._assembled("elasticity")
    foreign = other.create_vec()
    many = [eng.create_vec() for _ in range(NMAX + 1)]
    refused(lambda: A.mult_block([], []), OUTOFRANGE, "1 to 48")
    refused(lambda: A.mult_block(many, many), OUTOFRANGE, "1 to 48")                       # the range before the aliasing
    refused(lambda: A.mult_block([X[0], None], [Y[0], Y[0]]), ARG_WRONG, "null")            # a null entry before the aliasing
    refused(lambda: A.mult_block([foreign, X[1]], [Y[0], Y[0]]), ARG_WRONG, "another IGX")  # a foreign vector before the aliasing
    refused(lambda: A.mult_block(X, [Y[0], Y[1], foreign]), ARG_WRONG, "another IGX")
    refused(lambda: A.mult_block(X, [Y[0], Y[1], Y[0]]), ARG_WRONG, "two results")
    refused(lambda: A.mult_block(X, [Y[0], Y[1], X[0]]), ARG_WRONG, "different vectors")
    refused(lambda: A.mult_block([X[0], X[1], X[0]], [Y[0], Y[0], X[0]]), ARG_WRONG, "two results")      # Y twice before X in Y
    A.mult_block([X[0], X[1], X[0]], Y)                                                  # twice in X is allowed; a refused call leaves nothing behind
    assert eng.kernel_name().startswith("mat_mult_block")
    # stale: the space changes under the matrix and the vectors
    eng.axis_uniform(0, 2, 5)
    eng.setup()
    fresh = [eng.create_vec() for _ in range(3)]
    refused(lambda: A.mult_block(X, Y), ARG_WRONG, "IGXSetUp")
    A2 = eng.create_mat()
    refused(lambda: A2.mult_block(fresh[:2], [fresh[2], Y[0]]), ARG_WRONG, "vector of another size")
    refused(lambda: A2.mult_block(fresh[:1], fresh[:1]), ARG_WRONG, "different vectors")
    # two ranks on an axis (no communicator needed); the aliasing still answers first
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.set_comm(2, 0)
    g.setup()
    Ag, xg, yg = g.create_mat(), g.create_vec(), g.create_vec()
    refused(lambda: Ag.mult_block([xg], [xg]), ARG_WRONG, "different vectors")
    refused(lambda: Ag.mult_block([xg], [yg]), SUP, "one rank")
