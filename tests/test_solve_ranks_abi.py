"""IGXCommAllSum in the C ABI (include/petiga_amd.h) and its Python view, and the count rule of IGXSolve on a partition, on the CPU.
  export      IGXCommAllSum is declared, exported and bound with the header's arguments; IGX.comm_all_sum is there.
  refusals    null iga or values, n outside [1, 64], before IGXSetUp, more than one rank without a communicator -- in that order, each decided
              before any HIP call; on one rank the call returns 0 and leaves the values as they are.
  count rule  tests/krylov_ref.py's loops on the oracle's matrices of the cases tests/test_gpu_solve_ranks.py runs, every inner product
              formed once as a plain sum and once as the rank-ordered sum of the ranks' sums over the entries they own (IGX.sizes() of engines
              set up on the partition): CG crosses its threshold within 1 step of itself, BiCGStab within BICG_MARGIN of
              tests/test_gpu_krylov_solve.py.  A case that fails here sits on a threshold: the case moves, not the margin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import krylov_ref as K
import solve_ranks_cases as SR

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "petiga_amd.h")
BICG_MARGIN = 8      # tests/test_gpu_krylov_solve.py's (that module needs the GPU suite's imports: the figure is restated and compared below)


def test_margin_is_the_gpu_suites():
    text = open(os.path.join(HERE, "test_gpu_krylov_solve.py")).read()
    assert re.search(r"^BICG_MARGIN = %d\b" % BICG_MARGIN, text, flags=re.M)


def test_declared_exported_and_bound():
    import petiga_amd as P
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+IGXCommAllSum\s*\(([^)]*)\)\s*;", text)
    assert m, "not declared in include/petiga_amd.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["IGX iga", "int n", "double vals[]"]
    f = P.lib().IGXCommAllSum                       # AttributeError: the library does not export it
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    assert callable(P.IGX.comm_all_sum)


def _box(setup=True, ranks=1):
    import petiga_amd as P
    g = P.IGX(3, 1)
    if ranks > 1:
        g.set_comm(ranks, 0)
    for i, N in enumerate((4, 3, 3)):
        g.axis_uniform(i, 2, N)
    if setup:
        g.setup()
    return g


def test_refusals_in_their_order_and_the_one_rank_no_op():
    import petiga_amd as P
    L = P.lib()
    vals = (C.c_double * 64)(*range(64))
    why = lambda: L.IGXGetLastError().decode()
    # 1. null iga or values, whatever else is wrong
    raw, raw2 = _box(setup=False), _box(setup=False, ranks=2)
    assert L.IGXCommAllSum(None, 0, vals) == 62
    assert L.IGXCommAllSum(raw.h, 0, None) == 62 and "IGXCommAllSum" in why()
    # 2. the range, before the set-up is looked at
    for n in (0, -1, 65):
        assert L.IGXCommAllSum(raw.h, n, vals) == 63 and "IGXCommAllSum" in why(), n
    # 3. before IGXSetUp, on one rank and on two
    assert L.IGXCommAllSum(raw.h, 1, vals) == 58 and "IGXSetUp" in why()
    assert L.IGXCommAllSum(raw2.h, 64, vals) == 58 and "IGXSetUp" in why()
    # 4. two ranks and no communicator: comm_exchange's words
    g = _box(ranks=2)
    assert L.IGXCommAllSum(g.h, 3, vals) == 73 and "IGXCommInitRCCL() / IGXCommInitTransport()" in why()
    with pytest.raises(P.IGXError) as e:
        g.comm_all_sum([1.0, 2.0])
    assert e.value.code == 73
    assert list(vals) == list(range(64))
    # one rank: 0, the values untouched
    g = _box()
    for n in (1, 64):
        assert L.IGXCommAllSum(g.h, n, vals) == 0
    assert list(vals) == list(range(64))
    out = g.comm_all_sum([1e16, 1.0, -1e16])
    assert isinstance(out, np.ndarray) and out.tolist() == [1e16, 1.0, -1e16]


def test_sweep_timing_hook_is_declared_bound_and_refuses_before_any_hip_call():
    import petiga_amd as P
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+IGXKrylovSweepTime\s*\(([^)]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 5 == len(P.lib().IGXKrylovSweepTime.argtypes)
    names = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*IGXKrylovSweep\s*;", text).group(1)
    names = [w.split("=")[0].strip() for w in names.split(",")]
    assert names[-1] == "IGX_SWEEP_COUNT" and [w[len("IGX_SWEEP_"):].lower() for w in names[:-1]] == list(P.KRYLOV_SWEEPS)
    L, ms = P.lib(), C.c_double(-1.0)
    raw, g = _box(setup=False), _box(ranks=2)
    assert L.IGXKrylovSweepTime(g.h, 0, 1, 1, None) == 62
    for sweep, runs, reps in ((-1, 1, 1), (len(P.KRYLOV_SWEEPS), 1, 1), (0, 2, 1), (0, 1, 0)):
        assert L.IGXKrylovSweepTime(g.h, sweep, runs, reps, C.byref(ms)) == 63, (sweep, runs, reps)
    assert L.IGXKrylovSweepTime(raw.h, 0, 1, 1, C.byref(ms)) == 58
    assert ms.value == -1.0


def test_two_ranks_without_a_communicator_keep_the_solves_refusal():
    """IGXSolve on a partition needs the communicator: without one the refusal and its words are what they were"""
    import petiga_amd as P
    g = _box(ranks=2)
    g.set_form("poisson")
    with pytest.raises(P.IGXError) as e:
        g.solve(None, None)
    assert e.value.code == 56 and "the library has no sum across ranks" in str(e.value)


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_owned_sets_cover_every_entry_once(name):
    A, b = SR.oracle_system(name)
    sets = SR.owned_sets(name)
    seen = np.zeros(b.size, dtype=int)
    for idx in sets:
        np.add.at(seen, idx, 1)
    assert len(sets) == SR.world(name) and np.all(seen == 1)
    assert min(idx.size for idx in sets) > 0


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_rank_ordered_sums_keep_the_count(name):
    c = SR.CASES[name]
    A, b = SR.oracle_system(name)
    ranked = SR.rank_ordered_dot(SR.owned_sets(name))
    for method, pc in c["solves"]:
        loop, margin = (K.cg, 1) if method == "cg" else (K.bicgstab, BICG_MARGIN)
        prec = SR.preconditioner(A, pc, c["dof"])
        runs = [loop(lambda v: A @ v, prec, b, rtol=c["rtol"], maxit=c["maxit"], dot=dot) for dot in (np.dot, ranked)]
        counts = [info["iterations"] for _, info in runs]
        res = [np.linalg.norm(b - A @ x) / np.linalg.norm(b) for x, _ in runs]
        print("%s, %s with %s: iterations %s, true residuals / |b| %s" % (name, method, pc, counts, ["%.2e" % r for r in res]))
        assert all(info["reason"] == K.CONVERGED_RTOL for _, info in runs)
        assert abs(counts[0] - counts[1]) <= margin
