"""The vector algebra on IGXVec and IGXSolve in the C ABI (include/petiga_amd.h) and its Python view: the eight calls are declared, exported and
bound with the header's argument counts; the two structs have the header's layout; the refusals that are decided before any HIP call, each
by code and word; and the two reference loops of tests/krylov_ref.py against scipy's sparse direct solve on a small SPD and a small
nonsymmetric matrix built here (and cg() against pcg(), bit for bit); and, on the oracle's matrices, what tests/test_gpu_krylov_lengths.py
leans on: the count rule between the summation orders and the two corner-supported outcomes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import krylov_ref as K
from fast_diag_ref import pcg

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
CALLS = {"IGXVecSet": 2, "IGXVecCopy": 2, "IGXVecScale": 2, "IGXVecAXPBY": 4, "IGXVecPointwiseDivide": 3, "IGXVecDot": 3, "IGXVecNorm2": 2, "IGXSolve": 6}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declarations():
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(IGX\w+)\s*\(([^)]*)\)\s*;", _header())}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    import petiga_amd as P
    decl = _declarations()
    assert name in decl, "not declared in include/petiga_amd.h"
    args = [a.strip() for a in decl[name].split(",") if a.strip()]
    assert len(args) == CALLS[name]
    f = getattr(P.lib(), name)                      # AttributeError: the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == len(args)
    doubles = [i for i, a in enumerate(args) if a.startswith("double") and "[" not in a and "*" not in a]
    assert [i for i, t in enumerate(f.argtypes) if t is C.c_double] == doubles


def test_python_view():
    import petiga_amd as P
    for m in ("fill", "copy_from", "scale", "axpby", "pointwise_divide", "dot", "norm"):
        assert callable(getattr(P.Vec, m)), m
    assert callable(P.IGX.solve)


CTYPES = {"int": C.c_int, "double": C.c_double, "IGXVec": C.c_void_p}


def _struct_from_header(name):
    """a ctypes.Structure with the members of `typedef struct { ... } name;` in the header's order"""
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header())
    assert m, name + " is not declared"
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ty]) for n in names.split(",")]
    return type(name, (C.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("name,size", [("IGXSolveSpec", 72), ("IGXSolveInfo", 32)])
def test_struct_layout(name, size):
    import petiga_amd as P
    want, have = _struct_from_header(name), getattr(P, name)
    assert C.sizeof(want) == size == C.sizeof(have)
    assert [(f[0], getattr(want, f[0]).offset) for f in want._fields_] == [(f[0], getattr(have, f[0]).offset) for f in have._fields_]


def test_enums_of_the_header():
    text = _header()
    for word, value in (("IGX_SOLVE_CG", 0), ("IGX_SOLVE_BICGSTAB", 1), ("IGX_OP_MATRIX", 0), ("IGX_OP_JACOBIAN", 1), ("IGX_OP_IJACOBIAN", 2), ("IGX_PC_NONE", 0),
                        ("IGX_PC_JACOBI", 1), ("IGX_PC_PBJACOBI", 2), ("IGX_PC_FASTDIAG", 3), ("IGX_CONVERGED_RTOL", K.CONVERGED_RTOL), ("IGX_CONVERGED_ATOL", K.CONVERGED_ATOL),
                        ("IGX_DIVERGED_ITS", K.DIVERGED_ITS), ("IGX_DIVERGED_BREAKDOWN", K.DIVERGED_BREAKDOWN), ("IGX_DIVERGED_NAN", K.DIVERGED_NAN)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (word, value), text), word
    import petiga_amd as P
    assert P.SOLVE_METHODS == dict(cg=0, bicgstab=1) and P.SOLVE_PCS == dict(none=0, jacobi=1, pbjacobi=2, fastdiag=3) and P.SOLVE_OPERATORS == dict(matrix=0, jacobian=1, ijacobian=2)


def _box(setup=True):
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i, N in enumerate((4, 3, 3)):
        g.axis_uniform(i, 2, N)
    if setup:
        g.setup()
    return g


def _solve_rc(g, **kw):
    """IGXSolve with null vectors: every refusal tested here is decided before the vectors are looked at"""
    import petiga_amd as P
    spec = P.IGXSolveSpec(kw.get("method", 0), kw.get("op", 0), kw.get("pc", 0), 0.0, 0.0, None, None, kw.get("rtol", 1e-8), kw.get("atol", 0.0), kw.get("maxit", 10))
    info = P.IGXSolveInfo()
    rc = P.lib().IGXSolve(g.h, C.byref(spec), None, None, C.byref(info), None)
    return rc, P.lib().IGXGetLastError().decode()


def test_refusals_decided_before_any_hip_call():
    import petiga_amd as P
    g = _box()
    g.set_form("poisson")
    for kw in (dict(rtol=-1e-8), dict(atol=-1.0), dict(rtol=float("nan")), dict(maxit=-1), dict(method=2), dict(method=-1), dict(op=3), dict(pc=4), dict(pc=-1)):
        rc, why = _solve_rc(g, **kw)
        assert rc == 63 and "IGXSolve" in why, (kw, rc, why)
    rc, why = _solve_rc(g)
    assert rc == 62, (rc, why)                                  # in range: now the null vectors are looked at
    assert P.lib().IGXSolve(g.h, None, None, None, None, None) == 62

    rc, why = _solve_rc(_box(setup=False))                      # before IGXSetUp
    assert rc == 58 and "IGXSetUp" in why, (rc, why)

    rc, why = _solve_rc(_box())                                 # no form set
    assert rc == 73, (rc, why)

    g = _box(setup=False)
    g.set_comm(2, 0)
    g.set_processors(1, 2)
    g.setup()
    g.set_form("poisson")
    rc, why = _solve_rc(g)
    assert rc == 56 and "Krylov solve" in why and "rank" in why, (rc, why)
    with pytest.raises(P.IGXError) as e:
        g.solve(None, None)
    assert e.value.code == 56 and "rank" in str(e.value)


def test_vector_calls_refuse_null_vectors():
    import petiga_amd as P
    L = P.lib()
    s = C.c_double(0)
    assert L.IGXVecSet(None, 1.0) == 62 and L.IGXVecCopy(None, None) == 62 and L.IGXVecScale(None, 2.0) == 62
    assert L.IGXVecAXPBY(None, 1.0, None, 1.0) == 62 and L.IGXVecPointwiseDivide(None, None, None) == 62
    assert L.IGXVecDot(None, None, C.byref(s)) == 62 and L.IGXVecNorm2(None, C.byref(s)) == 62


# ---- the reference loops against a sparse direct solve
def _spd(n=60, seed=0):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    L = sp.diags([-1.0, 2.8, -1.0], [-1, 0, 1], shape=(n, n)) + sp.diags([-0.3, -0.3], [-7, 7], shape=(n, n))
    d = 1.0 + rng.random(n)
    return (sp.diags(d) @ L @ sp.diags(d)).tocsc(), rng.standard_normal(n)


def _nonsymmetric(n=60, seed=1):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A = sp.diags([-1.0, 2.5, -0.4], [-1, 0, 1], shape=(n, n)) + sp.diags([0.35], [5], shape=(n, n)) + sp.diags([-0.2], [-9], shape=(n, n))
    return (A @ sp.diags(1.0 + rng.random(n))).tocsc(), rng.standard_normal(n)


@pytest.mark.parametrize("jacobi", [False, True])
def test_reference_cg_against_spsolve(jacobi):
    import scipy.sparse.linalg as spla
    A, b = _spd()
    want = spla.spsolve(A, b)
    D = A.diagonal()
    prec = (lambda v: v / D) if jacobi else (lambda v: v.copy())
    x, info = K.cg(lambda v: A @ v, prec, b, rtol=1e-12)
    assert info["reason"] == K.CONVERGED_RTOL and info["iterations"] <= b.size + 5
    assert info["history"].size == info["iterations"] + 1 and info["rnorm"] <= 1e-12 * info["bnorm"]
    assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max()
    x2, k2 = pcg(lambda v: A @ v, prec, b, rtol=1e-12)
    assert k2 == info["iterations"] and np.array_equal(x, x2), "cg() is not pcg()'s loop"
    # another summation order moves the count by one at the most here
    _, other = K.cg(lambda v: A @ v, prec, b, rtol=1e-12, dot=K.dot_pairwise_chunks)
    assert abs(other["iterations"] - info["iterations"]) <= 1


@pytest.mark.parametrize("jacobi", [False, True])
def test_reference_bicgstab_against_spsolve(jacobi):
    import scipy.sparse.linalg as spla
    A, b = _nonsymmetric()
    assert abs(A - A.T).max() > 0.1
    want = spla.spsolve(A, b)
    D = A.diagonal()
    prec = (lambda v: v / D) if jacobi else (lambda v: v.copy())
    x, info = K.bicgstab(lambda v: A @ v, prec, b, rtol=1e-12)
    assert info["reason"] == K.CONVERGED_RTOL and info["iterations"] <= b.size
    assert np.linalg.norm(b - A @ x) <= 1e-10 * np.linalg.norm(b)
    assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max()


def test_reference_outcomes():
    A, b = _spd()
    op, ident = (lambda v: A @ v), (lambda v: v.copy())
    for loop in (K.cg, K.bicgstab):
        x, info = loop(op, ident, np.zeros_like(b), x0=np.ones_like(b))
        assert info["reason"] == K.CONVERGED_ATOL and info["iterations"] == 0 and not x.any()
        x, info = loop(op, ident, b, maxit=1)
        assert info["reason"] == K.DIVERGED_ITS and info["iterations"] == 1 and info["history"].size == 2
        x, info = loop(op, ident, b, rtol=0.0, atol=1e-6)
        assert info["reason"] == K.CONVERGED_ATOL and info["rnorm"] <= 1e-6
    x, info = K.cg(lambda v: -(A @ v), ident, b)                # p.Ap < 0
    assert info["reason"] == K.DIVERGED_BREAKDOWN and info["iterations"] == 0 and not x.any()
    x, info = K.bicgstab(lambda v: 0.0 * v, ident, b)           # rhat.v = 0
    assert info["reason"] == K.DIVERGED_BREAKDOWN and info["iterations"] == 0 and not x.any()


@pytest.mark.parametrize("p,N", [(3, (5, 4, 3)), (2, (8, 8, 8))])
def test_summation_order_moves_the_cg_count_by_one_at_the_most(p, N):
    """The cases tests/test_gpu_krylov_solve.py pins the device loop's count on, here on the CPU oracle's matrix with numpy's preconditioners:
    the same loop with its inner products added in three orders (np.dot, from the far end, chunk by chunk like a slab reduction) crosses
    rtol = 1e-10 within one step of each other, for no preconditioner, Jacobi and fast diagonalisation.  A case that fails here sits on the
    threshold: move rtol, not the margin."""
    from common import make_pair, warped_geometry
    from fast_diag_ref import FastDiagRef, axis_matrices, fixed_faces
    orc, _ = make_pair(3, 1, p, list(N), engine=False)
    X, W = warped_geometry(orc, 3, seed=2, rational=True, amp=0.05)
    orc.set_geometry(X, W)
    faces = [(d, s) for d in range(3) for s in range(2)]
    for d, s in faces:
        orc.set_boundary_value(d, s, 0, 0.0)
    A_o, b = orc.compute_system("orc_form_poisson")
    A, b = A_o.scipy().tocsr(), np.asarray(b)
    D = A.diagonal()
    fd = FastDiagRef([axis_matrices(orc.axis(d)["U"], orc.axis(d)["p"]) for d in range(3)], 1, fixed_faces(1, [(d, s, 0) for d, s in faces]), 0.0, [1.0, 1.0, 1.0])
    for label, prec in (("none", lambda v: v.copy()), ("jacobi", lambda v: v / D), ("fastdiag", fd.apply)):
        counts = [K.cg(lambda v: A @ v, prec, b, rtol=1e-10, dot=dot)[1]["iterations"] for dot in (np.dot, K.dot_reversed, K.dot_pairwise_chunks)]
        print("p = %d %s, pc %s: iterations %s" % (p, N, label, counts))
        assert max(counts) - min(counts) <= 1


# ---- the references of tests/test_gpu_krylov_lengths.py, on the oracle's matrices
def _length_problem(n):
    """(A, {pc: M^-1}) of a problem of krylov_ref.SMALL_LENGTHS from the oracle's matrix, with numpy's preconditioners"""
    import oracle_api as O
    from common import make_pair
    from fast_diag_ref import FastDiagRef, axis_matrices, fixed_faces
    form, dof, p, N, bcs = K.SMALL_LENGTHS[n]
    orc, _ = make_pair(3, dof, p, list(N), engine=False)
    for bc in bcs:
        orc.set_boundary_value(*bc)
    if form == "poisson":
        A = orc.compute_system("orc_form_poisson")[0].scipy().tocsr()
    else:
        from test_gpu_matrix_action import EL
        A = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))[0].scipy().tocsr()
    assert A.shape[0] == n
    D = A.diagonal()
    precs = {"none": lambda v: v.copy(), "jacobi": lambda v: v / D}
    if n == 1025:
        fd = FastDiagRef([axis_matrices(orc.axis(d)["U"], orc.axis(d)["p"]) for d in range(3)], 1, fixed_faces(1, [bc[:3] for bc in bcs]), 0.0, [1.0, 1.0, 1.0])
        precs["fastdiag"] = fd.apply
    if dof > 1:
        dense = A.toarray().reshape(n // dof, dof, n // dof, dof)
        inv = np.linalg.inv(np.stack([dense[i, :, i, :] for i in range(n // dof)]))
        precs["pbjacobi"] = lambda v: np.einsum("nij,nj->ni", inv, v.reshape(-1, dof)).reshape(-1)
    return A, precs


@pytest.mark.parametrize("n", sorted(K.SMALL_LENGTHS))
def test_count_rule_holds_between_the_host_orders(n):
    """The device count is held to [lo - m, hi + m], m = max(1, hi - lo), over the host loop in three summation orders: here each order is
    held to the window of the other two, on b = A x_true as the GPU cases form it."""
    A, precs = _length_problem(n)
    b = A @ K.x_true(n)
    for pc in sorted(precs):
        counts = []
        for _, dot in K.ORDERS:
            x, info = K.cg(lambda v: A @ v, precs[pc], b, rtol=1e-10, maxit=600, dot=dot)
            assert info["reason"] == K.CONVERGED_RTOL
            assert np.abs(x - K.x_true(n)).max() <= 1e-7 * np.abs(K.x_true(n)).max()
            counts.append(info["iterations"])
        print("n = %d, pc %s: iterations %s" % (n, pc, counts))
        for i, k in enumerate(counts):
            lo, hi, m = K.count_window(counts[:i] + counts[i + 1:])
            assert lo - m <= k <= hi + m, (pc, counts)


def test_corner_supported_outcomes_of_the_host_loops():
    """b on the eight corner dofs of the all-Dirichlet box (a corner node lies in one element: its row and column are the identity's, so
    A b = b exactly): CG without a preconditioner is exact after one step; BiCGStab from x0 = c b has s = 0, t = 0, t.t = 0 and breaks down
    at iteration 0 with x untouched."""
    n = 175
    A, precs = _length_problem(n)
    form, dof, p, N, _ = K.SMALL_LENGTHS[n]
    b = np.zeros(n)
    b[K.corner_dofs([N[d] + p for d in range(3)])] = np.random.default_rng(8).standard_normal(8)
    assert np.count_nonzero(b) == 8 and np.array_equal(A @ b, b)
    op = lambda v: A @ v
    for _, dot in K.ORDERS:
        x, info = K.cg(op, precs["none"], b, rtol=1e-10, dot=dot)
        assert info["reason"] == K.CONVERGED_RTOL and info["iterations"] == 1 and info["rnorm"] == 0.0 and np.array_equal(x, b)
        x0 = 0.375 * b
        x, info = K.bicgstab(op, precs["none"], b, x0=x0, rtol=1e-9, dot=dot)
        assert info["reason"] == K.DIVERGED_BREAKDOWN and info["iterations"] == 0 and info["history"].size == 1 and np.array_equal(x, x0)
