"""The matrix-free action and diagonal at degree 4 on two ranks (IGXComputeMatrixAction / IGXComputeMatrixDiagonal + IGXRefreshGhosts
+ IGXReduceGhostRows; vec_sumfact, one workgroup per element, 6 x 6 x 6 lanes): Poisson on (3, 3, 6) elements with Dirichlet values on all
six faces.  Only the owner's values of X are set, the ghosts arrive through IGXRefreshGhosts; each rank forms its part of Y and of D and
IGXReduceGhostRows(NULL, .) completes the rows it owns.  The owned rows of both ranks together equal the single-rank oracle's matrix
times X, |Y - R| <= 1e-12 max(S) on the free rows and |Y_i - m_i X_i| <= 1e-12 |m_i X_i| on the Dirichlet rows, and its diagonal,
|D - R| <= 1e-12 max|R| on the free rows and exactly on the fixed ones (the element count over BOTH ranks); and row by row the long
double TensorRef: |Y_i - R_i| <= C_ID u S_i, |D_r - R_rr| <= C_ID u S_rr.  Two processes share the GPU over tests/fake_rccl's double of
librccl.so, in the pattern of tests/test_gpu_matrix_action_ranks.py; each is started once."""
import os
import sys

import numpy as np
import pytest

from test_gpu_matrix_action_ranks import FAKE_RCCL, HERE, _free_port

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]

P_DEG, N_EL = 4, (3, 3, 6)
BCS = {(d, s, 0): 1.0 + d for d in range(3) for s in range(2)}


def _x(n):
    return np.random.default_rng(5).standard_normal(n)


def _rank_main(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      IGX_RCCL_LIB=FAKE_RCCL, FAKE_RCCL_TIMEOUT_S="90", IGX_LINK_PROBE_MB="8")
    for p_ in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import petiga_amd as P
    from petiga_amd import exchange
    g = P.IGX(3, 1)
    g.set_comm(world, rank)
    for i in range(3):
        g.axis_uniform(i, P_DEG, N_EL[i])
    g.setup()
    for (d, s, f), v in BCS.items():
        g.set_boundary_value(d, s, f, v)
    g.set_form("poisson")
    assert exchange.init_comm(g, transport="rccl") == "rccl"
    A = g.create_mat()                       # (for the row numbering only: nothing is assembled into it)
    nrow, _, maps = A.layout()
    ns = g.sizes()["node_sizes"]
    r = np.arange(A.nbrows)
    node = maps[0][0][r % nrow[0]].astype(np.int64) + ns[0] * (maps[1][0][(r // nrow[0]) % nrow[1]].astype(np.int64) + ns[1] * maps[2][0][r // (nrow[0] * nrow[1])].astype(np.int64))
    own = np.array([g.row_owned(int(a), int(b), int(c)) for a, b, c in zip(r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1]))])
    Xg = _x(int(np.prod(ns)))
    X = g.create_vec().set(np.where(own, Xg[node], 3.0))      # only the owner's values are set
    g.refresh_ghosts(X)
    assert np.array_equal(X.get(), Xg[node])
    Y, D = g.create_vec(), g.create_vec()
    g.compute_matrix_action(X, Y)
    kn = g.kernel_name()
    assert "vec_sumfact" in kn and "matrix action" in kn and "one workgroup per element" in kn and "6 x 6 x 6 lanes" in kn, kn
    g.reduce_ghost_rows(None, Y)
    sent = g.comm_last_bytes()
    g.compute_matrix_diagonal(D)
    kn = g.kernel_name()
    assert "vec_sumfact" in kn and "matrix diagonal" in kn and "one workgroup per element" in kn and "6 x 6 x 6 lanes" in kn, kn
    g.reduce_ghost_rows(None, D)
    g.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), row=node[own], Y=Y.get()[own], D=D.get()[own], bytes=sent + g.comm_last_bytes())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_the_single_rank_oracle_and_the_tensor_reference(tmp_path):
    import torch.multiprocessing as mp
    import pointwise_ref as PW
    import tensor_ref as T
    from common import make_pair
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    orc, _ = make_pair(3, 1, P_DEG, list(N_EL), engine=False)
    for (d, s, f), v in BCS.items():
        orc.set_boundary_value(d, s, f, v)
    n = orc.global_size()
    X = _x(n)
    M = orc.compute_system("orc_form_poisson")[0].scipy()
    R, S, diag = M @ X, abs(M) @ np.abs(X), M.diagonal()
    off = abs(M)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    Y, D, seen, sent = np.zeros(n), np.zeros(n), np.zeros(n, dtype=int), 0
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        Y[d["row"]] = d["Y"]
        D[d["row"]] = d["D"]
        np.add.at(seen, d["row"], 1)
        sent += int(d["bytes"])
    assert sent > 0 and np.all(seen == 1)                # every row is owned by exactly one rank
    free = ~fixed
    assert fixed.any() and free.any()
    err, scale = np.abs(Y - R)[free].max(), S[free].max()
    print("action, free rows: max|Y - R| = %.3e, max S = %.3e, ratio %.3e (tol 1e-12); Dirichlet rows: %d" % (err, scale, err / scale, fixed.sum()))
    assert err <= 1e-12 * scale
    want = diag[fixed] * X[fixed]
    assert np.all(np.abs(Y[fixed] - want) <= 1e-12 * np.abs(want))
    err, scale = np.abs(D - diag)[free].max(), np.abs(diag)[free].max()
    print("diagonal, free rows: max|D - R| = %.3e, max|R| = %.3e, ratio %.3e (tol 1e-12)" % (err, scale, err / scale))
    assert err <= 1e-12 * scale
    assert np.array_equal(D[fixed], diag[fixed])
    # row by row against the long double reference of the single-rank operator
    ref = T.reference(orc, 3, T.poisson(3), bcs=BCS)
    print("action row by row: worst %.2f u S (c = %g)" % (PW.compare_rows(Y, *ref.action(X), T.C_ID, ref, "poisson-p4 two ranks"), T.C_ID))
    rows = np.arange(n)
    Rd, Sd = ref.entries(rows, rows)
    print("diagonal row by row: worst %.2f u S (c = %g)" % (T.compare_entrywise((rows, rows, D), Rd, Sd, T.C_ID, ref, "poisson-p4 two ranks", pattern=False), T.C_ID))
