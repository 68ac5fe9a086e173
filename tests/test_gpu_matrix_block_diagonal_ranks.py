"""The matrix-free point-block diagonal on two ranks (IGXComputeMatrixBlockDiagonal + one IGXReduceGhostRows per column), with the
mechanism of tests/test_gpu_matrix_diagonal_ranks.py: elasticity-p3 of tests/test_gpu_matrix_action.py split along one axis; each rank
forms its part of the dof columns and IGXReduceGhostRows(NULL, B[j]) completes the rows it owns.  The owned rows of both ranks together
equal the blocks of the single-rank oracle's matrix within the bound of tests/test_gpu_matrix_block_diagonal.py (fixed dofs exactly:
the element count over BOTH ranks)."""
import os
import sys

import numpy as np
import pytest

from test_gpu_matrix_action_ranks import FAKE_RCCL, HERE, _free_port

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]

EL = (1.5, 0.8)
P_, N_, DOF = 3, (4, 3, 3), 3
BCS = [(0, 0, 0, 0.0), (0, 0, 1, 0.0), (0, 0, 2, 0.0), (2, 1, 0, 1.0)]


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
    g = P.IGX(3, DOF)
    g.set_comm(world, rank)
    for i in range(3):
        g.axis_uniform(i, P_, N_[i])
    g.setup()
    for bc in BCS:
        g.set_boundary_value(*bc)
    g.set_form("elasticity", EL)
    assert exchange.init_comm(g, transport="rccl") == "rccl"
    A = g.create_mat()                       # (for the row numbering only: nothing is assembled into it)
    nrow, _, maps = A.layout()
    ns = g.sizes()["node_sizes"]
    r = np.arange(A.nbrows)
    node = maps[0][0][r % nrow[0]].astype(np.int64) + ns[0] * (maps[1][0][(r // nrow[0]) % nrow[1]].astype(np.int64) + ns[1] * maps[2][0][r // (nrow[0] * nrow[1])].astype(np.int64))
    own = np.array([g.row_owned(int(a), int(b), int(c)) for a, b, c in zip(r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1]))])
    assert 0 < own.sum() < int(np.prod(ns))                  # the mesh is split
    B = [g.create_vec() for _ in range(DOF)]
    g.compute_matrix_block_diagonal(B)
    assert "vec_sumfact" in g.kernel_name() and "matrix block diagonal" in g.kernel_name(), g.kernel_name()
    sent = 0
    for b in B:
        g.reduce_ghost_rows(None, b)
        sent += g.comm_last_bytes()
    g.synchronize()
    val = np.stack([b.get().reshape(-1, DOF) for b in B], axis=2)      # [local node, i, j]
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), node=node[own], val=val[own], bytes=sent)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_the_single_rank_oracle_blocks(tmp_path):
    import torch.multiprocessing as mp
    import oracle_api as O
    from common import make_pair
    from test_gpu_matrix_block_diagonal import blocks_of, check_blocks, fixed_rows
    mp.spawn(_rank_main, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    orc, _ = make_pair(3, DOF, P_, list(N_), engine=False)
    for bc in BCS:
        orc.set_boundary_value(*bc)
    M = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))[0].scipy()
    R, fx = blocks_of(M, DOF), fixed_rows(M).reshape(-1, DOF)
    Bh, seen, sent = np.zeros_like(R), np.zeros(R.shape[0], dtype=int), 0
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        Bh[d["node"]] = d["val"]
        np.add.at(seen, d["node"], 1)
        sent += int(d["bytes"])
    assert sent > 0 and np.all(seen == 1)                # every node is owned by exactly one rank
    assert fx.any()
    check_blocks(Bh, R, fx, 1e-12, "elasticity-p3 on two ranks")
