"""The matrix-free diagonals on two ranks (IGXComputeMatrixDiagonal / IGXComputeIJacobianDiagonal + IGXRefreshGhosts +
IGXReduceGhostRows): only the owner's values of U and V are set, the ghosts arrive through IGXRefreshGhosts; each rank forms its part
of D and IGXReduceGhostRows(NULL, D) completes the rows it owns.  The owned rows of both ranks together equal the diagonal R of the
single-rank oracle's matrix: free dofs |D - R| <= tol max|R| over the free dofs of the same field (tol 1e-12 for Poisson, 1e-11 for
the NS-VMS Tangent), fixed dofs exactly (the element count over BOTH ranks).  Two processes share the GPU over tests/fake_rccl's
double of librccl.so, as in tests/test_gpu_matrix_action_ranks.py; each is started once."""
import os
import sys

import numpy as np
import pytest

from test_gpu_matrix_action_ranks import FAKE_RCCL, HERE, _free_port

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]

NU, FX, DT = 1.472e-4, 3.37204e-3, 1e-2
NS = (NU, FX, -0.4 * FX, 0.25 * FX, DT)
# name -> (p, N, dof, form, Dirichlet values (axis, side, field, value))
CASES = {"poisson-p3": (3, (6, 5, 9), 1, "poisson", [(d, s, 0, 1.0 + d) for d in range(3) for s in range(2)]),
         "nsvms-p2": (2, (4, 4, 8), 4, "nsvms", [(a, s, f, 0.1 * f - 0.05 * s) for a in (1, 2) for s in range(2) for f in range(3)])}


def _vectors(n):
    rng = np.random.default_rng(5)
    return 0.3 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)      # U, V


def _rank_main(rank, world, port, name, outdir):
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
    p, N, dof, form, bcs = CASES[name]
    g = P.IGX(3, dof)
    g.set_comm(world, rank)
    for i in range(3):
        g.axis_uniform(i, p, N[i])
    g.setup()
    for bc in bcs:
        g.set_boundary_value(*bc)
    g.set_form(form, NS if form == "nsvms" else ())
    assert exchange.init_comm(g, transport="rccl") == "rccl"
    A = g.create_mat()                       # (for the row numbering only: nothing is assembled into it)
    nrow, _, maps = A.layout()
    ns = g.sizes()["node_sizes"]
    r = np.arange(A.nbrows)
    node = maps[0][0][r % nrow[0]].astype(np.int64) + ns[0] * (maps[1][0][(r // nrow[0]) % nrow[1]].astype(np.int64) + ns[1] * maps[2][0][r // (nrow[0] * nrow[1])].astype(np.int64))
    own = np.array([g.row_owned(int(a), int(b), int(c)) for a, b, c in zip(r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1]))])
    dofrow = (node[:, None] * dof + np.arange(dof)).ravel()      # global dof of every local vector entry
    owndof = np.repeat(own, dof)
    vecs = []
    for glob, junk in zip(_vectors(int(np.prod(ns)) * dof), (-7.0, 9.0)):      # only the owner's values are set
        v = g.create_vec().set(np.where(owndof, glob[dofrow], junk))
        g.refresh_ghosts(v)
        assert np.array_equal(v.get(), glob[dofrow])
        vecs.append(v)
    U, V = vecs
    D = g.create_vec()
    if form == "poisson":
        g.compute_matrix_diagonal(D)
    else:
        g.compute_ijacobian_diagonal(2.0 / DT, V, 0.0, U, D)
    assert "vec_sumfact" in g.kernel_name() and "matrix diagonal" in g.kernel_name(), g.kernel_name()
    g.reduce_ghost_rows(None, D)
    g.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), row=dofrow[owndof], val=D.get()[owndof], bytes=g.comm_last_bytes())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_ranks_match_the_single_rank_oracle_diagonal(name, tmp_path):
    import torch.multiprocessing as mp
    import oracle_api as O
    from common import make_pair
    p, N, dof, form, bcs = CASES[name]
    mp.spawn(_rank_main, args=(2, _free_port(), name, str(tmp_path)), nprocs=2, join=True)
    orc, _ = make_pair(3, dof, p, list(N), engine=False)
    for bc in bcs:
        orc.set_boundary_value(*bc)
    n = orc.global_size()
    U, V = _vectors(n)
    if form == "poisson":
        M, tol = orc.compute_system("orc_form_poisson")[0].scipy(), 1e-12
    else:
        M, tol = orc.compute_ijacobian("orc_form_ns_tangent", O.NSVMSCtx(*NS), 2.0 / DT, V, 0.0, U).scipy(), 1e-11
    R = M.diagonal()
    off = abs(M)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    D, seen, sent = np.zeros(n), np.zeros(n, dtype=int), 0
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        D[d["row"]] = d["val"]
        np.add.at(seen, d["row"], 1)
        sent += int(d["bytes"])
    assert sent > 0 and np.all(seen == 1)                # every row is owned by exactly one rank
    assert fixed.any()
    for f in range(dof):
        free = ~fixed[f::dof]
        err, scale = np.abs(D[f::dof] - R[f::dof])[free].max(), np.abs(R[f::dof])[free].max()
        print("%s field %d: max|D - R| = %.3e, max|R| = %.3e, ratio %.3e (tol %g); fixed dofs: %d" % (name, f, err, scale, err / scale, tol, (~free).sum()))
        assert err <= tol * scale
    assert np.array_equal(D[fixed], R[fixed])
