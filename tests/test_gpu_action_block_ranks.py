"""The matrix-free action on a block of vectors on two ranks (IGXComputeMatrixActionBlock + IGXRefreshGhosts per direction +
IGXReduceGhostRows per result), with the helper and the case of tests/test_gpu_matrix_action_ranks.py: only the owner's values of
every X_c are set, the ghosts arrive through IGXRefreshGhosts; each rank forms its part of every Y_c in ONE block call and
IGXReduceGhostRows(NULL, Y_c) completes the rows it owns.  The owned rows of both ranks together equal the single-rank oracle's matrix
times X_c, column by column: |Y - R| <= 1e-12 max(S) on the free rows, |Y_i - m_i X_i| <= 1e-12 |m_i X_i| on the Dirichlet rows, and row by
row |Y_i - R_i| <= C_ID u S_i against the long double reference of the single-rank operator.  The launch count of a rank's block call
is the rank's colours (three columns: one chunk).  The results start from NaN: the call zeroes them."""
import os
import sys

import numpy as np
import pytest

from test_gpu_matrix_action_ranks import CASES, FAKE_RCCL, HERE, _free_port

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]
NAME = "poisson-p3"
NCOL = 3


def _columns(n):
    return np.random.default_rng(5).standard_normal((NCOL, n))


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
    p, N, periodic, form = CASES[NAME]
    g = P.IGX(3, 1)
    g.set_comm(world, rank)
    for i in range(3):
        g.axis_uniform(i, p, N[i], periodic=bool(periodic[i]))
    g.setup()
    for d in range(3):
        for s in range(2):
            g.set_boundary_value(d, s, 0, 1.0 + d)
    g.set_form(form)
    assert exchange.init_comm(g, transport="rccl") == "rccl"
    A = g.create_mat()                       # (for the row numbering only: nothing is assembled into it)
    nrow, _, maps = A.layout()
    ns = g.sizes()["node_sizes"]
    r = np.arange(A.nbrows)
    node = maps[0][0][r % nrow[0]].astype(np.int64) + ns[0] * (maps[1][0][(r // nrow[0]) % nrow[1]].astype(np.int64) + ns[1] * maps[2][0][r // (nrow[0] * nrow[1])].astype(np.int64))
    own = np.array([g.row_owned(int(a), int(b), int(c)) for a, b, c in zip(r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1]))])
    X = []
    for glob in _columns(int(np.prod(ns))):      # only the owner's values are set
        v = g.create_vec().set(np.where(own, glob[node], 3.0))
        g.refresh_ghosts(v)
        assert np.array_equal(v.get(), glob[node])
        X.append(v)
    Y = [g.create_vec().set(np.full(A.nbrows, np.nan)) for _ in X]
    g.compute_matrix_action_block(X, Y)
    assert "vec_sumfact" in g.kernel_name() and "action on a block" in g.kernel_name(), g.kernel_name()
    c = g.coloring()
    assert g.last_timing()[2] == c[0] * c[1] * c[2]
    sent = 0
    for y in Y:
        g.reduce_ghost_rows(None, y)
        sent += g.comm_last_bytes()
    g.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), row=node[own], val=np.array([y.get()[own] for y in Y]), bytes=sent)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_the_single_rank_oracle_product_column_by_column(tmp_path):
    import torch.multiprocessing as mp
    import pointwise_ref as PW
    import tensor_ref as T
    from common import make_pair
    p, N, periodic, form = CASES[NAME]
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    orc, _ = make_pair(3, 1, p, list(N), periodic=[bool(x) for x in periodic], engine=False)
    n = orc.global_size()
    for d in range(3):
        for s in range(2):
            orc.set_boundary_value(d, s, 0, 1.0 + d)
    M = orc.compute_system("orc_form_poisson")[0].scipy()
    diag = M.diagonal()
    off = abs(M)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    Y, seen, sent = np.zeros((NCOL, n)), np.zeros(n, dtype=int), 0
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        Y[:, d["row"]] = d["val"]
        np.add.at(seen, d["row"], 1)
        sent += int(d["bytes"])
    assert sent > 0 and np.all(seen == 1) and fixed.any()      # every row is owned by exactly one rank
    ref = T.reference(orc, 3, T.poisson(3), bcs={(d, s, 0): 1.0 + d for d in range(3) for s in range(2)})
    for c, X in enumerate(_columns(n)):
        R, S = M @ X, abs(M) @ np.abs(X)
        free = ~fixed
        err, scale = np.abs(Y[c] - R)[free].max(), S[free].max()
        Rl, Sl = ref.action(X)
        worst = PW.compare_rows(Y[c], Rl, Sl, T.C_ID, ref, "%s column %d" % (NAME, c))
        print("column %d: free rows max|Y - R| = %.3e, max S = %.3e, ratio %.3e; row by row worst %.2f u S (c = %g)" % (c, err, scale, err / scale, worst, T.C_ID))
        assert err <= 1e-12 * scale
        want = diag[fixed] * X[fixed]
        assert np.all(np.abs(Y[c][fixed] - want) <= 1e-12 * np.abs(want))
