"""IGXMatMult, IGXMatGetDiagonal and IGXMatGetBlockDiagonal on the GPU (include/petiga_amd.h; petiga_amd/csrc/mat_ops.hpp): the assembled
block-CSR matrix as an operator.
  entry by entry   for EVERY row |y - y_ref| <= gamma_n sum_j |a_rj| |x_j| with y_ref the np.longdouble product of the engine's own matrix
                   (Mat.host()) with x, n the number of products of the row and gamma_n = n u / (1 - n u) (krylov_ref.gamma): the bound of a
                   sum of n products in ANY order, so it is derived, not measured.  Under both index variants (IGX_MATMULT_INDEX).
  other operators  the oracle's matrix times x and IGXComputeMatrixAction / IJacobianAction on the same x, by the bounds of
                   tests/test_gpu_matrix_action.py (its cases, its references, its _check), Dirichlet values set.
  bit facts        two products agree bit for bit; NaN in y does not survive; a row's product does not change when every OTHER row's values
                   become NaN.
  diagonals        np.array_equal to the entries picked out of Mat.host(); the block columns through IGXBlockDiagonalInvert / Apply;
                   Cahn-Hilliard's IJacobian diagonal (which no matrix-free driver forms) against the oracle's.
  refusals         foreign and stale vectors, x == y, nb != bs, two ranks on an axis.
The meshes are the smallest that hold every row kind (at most 8 elements per axis).  Every case asserts from browptr that it holds rows whose
start is 16-byte aligned and, where bs is odd, rows whose start is not (bs^2 even: every row starts on an even double).  Every test prints
what it sees before it asserts (run with -s)."""
import ctypes as C

import numpy as np
import pytest

import krylov_ref as K
import mat_ops_ref as R
import oracle_api as O
import test_gpu_matrix_action as MA
from common import make_pair, warped_geometry

pytestmark = pytest.mark.gpu

ARG_WRONG, SUP = 62, 56
# name -> (dim, dof, p, N, make_pair keywords, what is assembled)
CASES = {
    "poisson-p1": (3, 1, 1, (5, 4, 6), {}, "system"),
    "poisson-p2": (3, 1, 2, (5, 4, 6), {}, "system"),
    "poisson-p3": (3, 1, 3, (5, 4, 6), {}, "system"),
    "poisson-p4": (3, 1, 4, (5, 4, 6), {}, "system"),
    "graded-c0-line": (3, 1, 2, (0, 0, 0), {"knots": MA.KNOTS_C0}, "system"),
    "periodic-axis": (3, 1, 2, (4, 6, 5), {"periodic": [False, True, False]}, "system"),
    "periodic-folded": (3, 1, 2, (3, 5, 3), {"periodic": [True, False, False]}, "system"),      # 3 < 2p + 1 functions on axis 0: a row's stencil wraps onto itself
    "dim1": (1, 1, 2, (7,), {}, "system"),
    "dim2": (2, 1, 3, (5, 4), {}, "system"),
    "elasticity": (3, 3, 2, (4, 3, 3), {}, "system"),
    "nsvms-nurbs": (3, 4, 2, (4, 4, 4), {}, "nsvms"),
    "run-time-struct": (3, 1, 2, (4, 4, 3), {}, "struct"),
}


def _assembled(name):
    """(engine, its assembled matrix) of a case; Dirichlet values on the lower face of every non-periodic axis"""
    import petiga_amd as P
    dim, dof, p, N, kw, what = CASES[name]
    periodic = kw.get("periodic", [False] * dim)
    if what == "nsvms":
        orc, eng = make_pair(dim, dof, p, list(N))
        Xg, Wg = warped_geometry(orc, 3, seed=11, rational=True, amp=0.08)
        eng.set_geometry(Xg, Wg)
    else:
        eng = P.IGX(dim, dof)
        for i in range(dim):
            if "knots" in kw:
                eng.axis_knots(i, p, kw["knots"][i])
            else:
                eng.axis_uniform(i, p, N[i], periodic=periodic[i])
        eng.setup()
    for d in range(dim):
        if not periodic[d]:
            for f in range(min(dof, 3)):
                eng.set_boundary_value(d, 0, f, 0.25 + 0.5 * f)
    A = eng.create_mat()
    if what == "nsvms":
        rng = np.random.default_rng(17)
        n = eng.create_vec().n
        eng.set_form("nsvms", MA.NS)
        eng.compute_ijacobian(2.0 / MA.DT, eng.create_vec().set(0.1 * rng.standard_normal(n)), 0.0, eng.create_vec().set(0.3 * rng.standard_normal(n)), A)
    elif what == "struct":
        eng.set_form_source(MA.USER_DIFFUSION, "UserDiffusion", (0.7,))
        eng.compute_system(A, eng.create_vec())
    else:
        eng.set_form("poisson" if dof == 1 else "elasticity", () if dof == 1 else MA.EL)
        eng.compute_system(A, eng.create_vec())
    eng.synchronize()
    return eng, A


def _reference(A):
    """(rp, ci, val, x, y_ref, S, n) from the engine's own matrix on the host"""
    rp, ci, val = A.host()
    x = np.random.default_rng(53).standard_normal(A.nbrows * A.bs)
    return (rp, ci, val, x) + R.entrywise_product(rp, ci, val, A.bs, x)


@pytest.mark.parametrize("index", ["tables", "bcolidx"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_row_within_the_bound_of_its_sum(name, index, monkeypatch):
    monkeypatch.setenv("IGX_MATMULT_INDEX", "0" if index == "tables" else "1")      # (read when the IGX is created)
    eng, A = _assembled(name)
    rp, ci, val, x, y_ref, S, n = _reference(A)
    bs = A.bs
    # the pattern the product walks is the one the restatement rebuilds from the axis tables
    nrow, ncol, _ = A.layout()
    assert nrow == ncol
    rcnt, rcol = R.tables_of_pattern(rp, ci, nrow, ncol)
    assert np.array_equal(R.browptr(rcnt), rp) and np.array_equal(R.bcolidx(rcnt, rcol, ncol), ci)
    start_odd = (rp[:-1] * bs * bs) % 2 == 1
    lengths = np.unique(np.diff(rp)) * bs * bs
    assert (~start_odd).any() and (start_odd.any() if bs % 2 else not start_odd.any())
    y = eng.create_vec().set(np.full(x.size, np.nan))
    eng.set_timing(True)
    A.mult(eng.create_vec().set(x), y)
    eng.synchronize()
    kname, launches = eng.kernel_name(), eng.last_timing()[2]
    eng.set_timing(False)
    got = y.get()
    bound = np.array([K.gamma(int(k)) for k in n], dtype=np.longdouble) * S
    err = np.abs(got.astype(np.longdouble) - y_ref)
    worst = float((err / np.maximum(bound, np.longdouble(1e-300))).max())
    print("%s, %s: %d rows (%d start on an odd double), row lengths %d .. %d doubles (%d kinds); max |y - y_ref| / bound = %.3f; %s"
          % (name, index, A.nbrows, start_odd.sum(), lengths.min(), lengths.max(), lengths.size, worst, kname))
    assert kname.startswith("mat_mult") and ("axis tables" if index == "tables" else "bcolidx") in kname and launches == 1
    assert np.isfinite(got).all()
    assert np.all(err <= bound)
    # two products agree bit for bit
    y2 = eng.create_vec()
    A.mult(eng.create_vec().set(x), y2)
    assert np.array_equal(y2.get(), got)


def test_sub_groups_and_wavefronts_by_the_longest_row(monkeypatch):
    """the lane rule of DESIGN.md 3.26: 8, 16 or 32 lanes per row while a lane takes two pairs at the most, else one wavefront; and the default
    index variant: the axis tables where a sub-group takes a row, bcolidx where a wavefront does"""
    monkeypatch.delenv("IGX_MATMULT_INDEX", raising=False)
    want = {"poisson-p1": "8 lanes per row", "dim1": "8 lanes per row", "dim2": "16 lanes per row", "poisson-p2": "32 lanes per row", "poisson-p3": "one wavefront per row",
            "elasticity": "one wavefront per row"}
    for name, words in want.items():
        eng, A = _assembled(name)
        A.mult(eng.create_vec(), eng.create_vec())
        print(name, "->", eng.kernel_name())
        assert words in eng.kernel_name()
        assert ("columns from bcolidx" if "wavefront" in words else "columns from the axis tables") in eng.kernel_name()


# ---- against the project's other operators
@pytest.mark.parametrize("name", ["poisson-p3-dirichlet", "poisson-p2-periodic", "elasticity-p3", "ch-p2-dirichlet", "poisson-p3-nurbs"])
def test_product_equals_the_oracle_matrix_times_x_and_the_matrix_free_action(name):
    X, U, V, Rx, S, fixed, diag = MA._reference(name)
    form, tol = MA.CASES[name][0], MA.CASES[name][7]
    _, eng = MA._pair(name)
    Ya = MA._action(name, eng, X, U, V).get().copy()      # (sets the form)
    A = eng.create_mat()
    if form == "cahnhilliard":
        eng.compute_ijacobian(250.0, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), A)
    else:
        eng.compute_system(A, eng.create_vec())
    y = eng.create_vec()
    A.mult(eng.create_vec().set(X), y)
    eng.synchronize()
    Y = y.get()
    assert fixed.any() and eng.kernel_name().startswith("mat_mult")
    MA._check(Y, X, Rx, S, fixed, diag, tol)              # the oracle's matrix times x
    free = ~fixed
    dev = np.abs(Y - Ya)[free].max() / S[free].max()
    print("%s: the product against the matrix-free action: max|Y - Ya| / max S = %.3e on the free rows" % (name, dev))
    assert dev <= tol                                      # that file's tolerance for the quantity: the same numbers reached two ways
    want = diag[fixed] * X[fixed]                          # the element count on the diagonal of a fixed row, in both operators
    assert np.all(np.abs(Y[fixed] - want) <= 1e-12 * np.abs(want)) and np.all(np.abs(Ya[fixed] - want) <= 1e-12 * np.abs(want))


# ---- bit facts
def _write_values(A, val):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    val = np.ascontiguousarray(val, dtype=np.float64)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(A.device_ptrs()[2], val.ctypes.data, val.nbytes, 1) == 0


@pytest.mark.parametrize("name", ["poisson-p2", "elasticity", "poisson-p3"])
def test_a_row_reads_its_own_values_alone(name):
    eng, A = _assembled(name)
    rp, ci, val, x = _reference(A)[:4]
    bs = A.bs
    xv, y = eng.create_vec().set(x), eng.create_vec()
    A.mult(xv, y)
    eng.synchronize()
    clean = y.get().copy()
    rows = np.unique(np.r_[0, 1, A.nbrows // 2, A.nbrows - 1, np.random.default_rng(7).integers(0, A.nbrows, 12)])
    poisoned = np.full(val.size, np.nan)
    for r in rows:
        poisoned[rp[r] * bs * bs:rp[r + 1] * bs * bs] = val[rp[r] * bs * bs:rp[r + 1] * bs * bs]
    _write_values(A, poisoned)
    A.mult(xv, y.set(np.full(x.size, np.nan)))
    eng.synchronize()
    got = y.get().reshape(-1, bs)
    keep = np.zeros(A.nbrows, dtype=bool)
    keep[rows] = True
    print("%s: %d rows keep their values, %d rows are NaN" % (name, keep.sum(), (~keep).sum()))
    assert np.array_equal(got[keep], clean.reshape(-1, bs)[keep]) and np.isnan(got[~keep]).all()


# ---- diagonals
def _picked_blocks(rp, ci, val, bs):
    """[nbrows][bs][bs]: the diagonal block of every row, picked out of the host copy"""
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    at = np.flatnonzero(ci == row)
    assert at.size == len(rp) - 1
    return val.reshape(-1, bs, bs)[at]


@pytest.mark.parametrize("name", sorted(CASES))
def test_diagonals_are_copies_of_the_stored_entries(name):
    eng, A = _assembled(name)
    rp, ci, val = A.host()
    bs = A.bs
    blocks = _picked_blocks(rp, ci, val, bs)
    pos = R.diagonal_position(*R.tables_of_pattern(rp, ci, *A.layout()[:2]))
    assert np.array_equal(ci[rp[:-1] + pos], np.arange(A.nbrows))      # the restatement finds the same block
    d = eng.create_vec().set(np.full(A.nbrows * bs, np.nan))
    eng.set_timing(True)
    A.diagonal(d)
    assert eng.kernel_name().startswith("mat_get_diagonal") and eng.last_timing()[2] == 1
    B = [eng.create_vec().set(np.full(A.nbrows * bs, np.nan)) for _ in range(bs)]
    A.block_diagonal(B)
    assert eng.kernel_name().startswith("mat_get_block_diagonal") and eng.last_timing()[2] == 1
    eng.set_timing(False)
    eng.synchronize()
    assert np.array_equal(d.get(), np.einsum("rii->ri", blocks).reshape(-1))
    for j in range(bs):
        assert np.array_equal(B[j].get(), blocks[:, :, j].reshape(-1))
    if bs == 1:
        return
    # the columns are the layout IGXBlockDiagonalInvert / Apply take, by the bounds of tests/test_gpu_matrix_block_diagonal.py: per node
    # max|B Binv - I| <= 16 bs u cond(B), and Y = Binv X within 4 bs u (|Binv| |X|) of the product of the read-back inverse
    u = 2.0 ** -53
    cond = np.linalg.cond(blocks)
    assert np.all(np.isfinite(cond)) and cond.max() <= 1e6
    assert eng.block_diagonal_invert(B) == 0
    inv = np.stack([B[j].get().reshape(-1, bs) for j in range(bs)], axis=2)
    res = np.abs(np.einsum("rik,rkj->rij", blocks, inv) - np.eye(bs)).max(axis=(1, 2))
    X = np.random.default_rng(3).standard_normal(A.nbrows * bs)
    Y = eng.create_vec()
    eng.block_diagonal_apply(B, eng.create_vec().set(X), Y)
    eng.synchronize()
    Xb = X.reshape(-1, bs)
    want, mag = np.einsum("rij,rj->ri", inv, Xb), np.einsum("rij,rj->ri", np.abs(inv), np.abs(Xb))
    print("%s: cond up to %.2e, worst max|B Binv - I| / (bs u cond) = %.3f (bound 16), worst |Y - Binv X| / (bs u |Binv||X|) = %.3f (bound 4)"
          % (name, cond.max(), (res / (bs * u * cond)).max(), (np.abs(Y.get().reshape(-1, bs) - want) / (bs * u * mag)).max()))
    assert np.all(res <= 16 * bs * u * cond)
    assert np.all(np.abs(Y.get().reshape(-1, bs) - want) <= 4 * bs * u * mag)


def test_cahn_hilliard_ijacobian_diagonal_against_the_oracle():
    """the form whose matrix-free diagonal is refused: the assembled IJacobian at the varying state of test_gpu_matrix_action's ch-p2 holds it"""
    name = "ch-p2"
    X, U, V, Rx, S, fixed, diag = MA._reference(name)
    _, eng = MA._pair(name)
    eng.set_form("cahnhilliard", MA.CH)
    A = eng.create_mat()
    eng.compute_ijacobian(250.0, eng.create_vec().set(V), 0.0, eng.create_vec().set(U), A)
    d = eng.create_vec()
    A.diagonal(d)
    eng.synchronize()
    # the scale of the file's tolerance: the largest entry of |A| over the free rows (S is |A| |X| row by row; the matrix-parity scale is max|A|)
    orc, _ = MA._pair(name)
    A_o = orc.compute_ijacobian("orc_form_ch_tangent", O.CahnHilliardCtx(*MA.CH), 250.0, V, 0.0, U).scipy()
    scale = abs(A_o).max()
    err = np.abs(d.get() - diag).max()
    print("Cahn-Hilliard IJacobian: max|d - diag A_o| = %.3e, max|A_o| = %.3e, ratio %.3e (tol %g)" % (err, scale, err / scale, MA.CASES[name][7]))
    assert err <= MA.CASES[name][7] * scale


# ---- refusals
def test_refusals_that_need_vectors():
    import petiga_amd as P
    eng, A = _assembled("elasticity")
    x, y = eng.create_vec(), eng.create_vec()

    def refused(call, code, *words):
        with pytest.raises(P.IGXError) as e:
            call()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    other, _ = _assembled("elasticity")
    foreign = other.create_vec()
    for call, fn in ((lambda: A.mult(foreign, foreign), "IGXMatMult"), (lambda: A.mult(x, foreign), "IGXMatMult"), (lambda: A.diagonal(foreign), "IGXMatGetDiagonal"),
                     (lambda: A.block_diagonal([x, y, foreign]), "IGXMatGetBlockDiagonal"), (lambda: A.solve(foreign, x), "IGXMatSolve")):
        refused(call, ARG_WRONG, fn, "another IGX")
    refused(lambda: A.mult(x, x), ARG_WRONG, "IGXMatMult", "different")
    refused(lambda: A.mult(None, y), ARG_WRONG, "IGXMatMult", "null")
    refused(lambda: A.block_diagonal([x, y]), ARG_WRONG, "nb must equal")
    refused(lambda: A.block_diagonal([x, y, None]), ARG_WRONG, "null block column")
    refused(lambda: A.block_diagonal([x, y, x]), ARG_WRONG, "two block columns")
    A.mult(x, y)                                   # a refused call leaves nothing behind
    assert eng.kernel_name().startswith("mat_mult")
    # stale: the space changes under the matrix and the vectors
    eng.axis_uniform(0, 2, 5)
    eng.setup()
    fresh = eng.create_vec()
    refused(lambda: A.mult(x, y), ARG_WRONG, "IGXMatMult", "IGXSetUp")
    refused(lambda: A.mult(fresh, y), ARG_WRONG, "IGXMatMult", "IGXSetUp")
    refused(lambda: A.diagonal(fresh), ARG_WRONG, "IGXMatGetDiagonal", "IGXSetUp")
    A2 = eng.create_mat()
    refused(lambda: A2.mult(fresh, y), ARG_WRONG, "IGXMatMult", "vector of another size")
    refused(lambda: A2.mult(fresh, fresh), ARG_WRONG, "different")      # sizes in order, then x == y
    A2.mult(fresh, eng.create_vec())
    eng.setup()                                    # a set-up that keeps every size: the matrix still carries the earlier set-up's pattern
    refused(lambda: A2.mult(fresh, eng.create_vec()), ARG_WRONG, "IGXMatMult", "IGXSetUp")
    # two ranks on an axis (no communicator needed): every call by name, and x == y still answers first
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.set_comm(2, 0)
    g.setup()
    Ag, xg, yg = g.create_mat(), g.create_vec(), g.create_vec()
    refused(lambda: Ag.mult(xg, xg), ARG_WRONG, "different")
    for call, fn in ((lambda: Ag.mult(xg, yg), "IGXMatMult"), (lambda: Ag.diagonal(xg), "IGXMatGetDiagonal"), (lambda: Ag.block_diagonal([xg]), "IGXMatGetBlockDiagonal"),
                     (lambda: Ag.solve(xg, yg, maxit=-1), "IGXMatSolve")):
        refused(call, SUP, fn, "one rank")
