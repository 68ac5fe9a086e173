"""The matrix-free actions on two ranks (IGXComputeMatrixAction / IGXComputeIJacobianAction + IGXRefreshGhosts + IGXReduceGhostRows):
only the owner's values of X (and U, V) are set, the ghosts arrive through IGXRefreshGhosts; each rank forms its part of Y and
IGXReduceGhostRows(NULL, Y) completes the rows it owns.  The owned rows of both ranks together equal the single-rank oracle's matrix
times X: |Y - R| <= tol max(S) with R = A_o X, S = |A_o| |X| (tol 1e-12 for Poisson, 1e-11 for the Tangent), Dirichlet rows
|Y_i - m_i X_i| <= 1e-12 |m_i X_i|; and row by row |Y_i - R_i| <= C_ID u S_i against the long double references (the TensorRef action for
Poisson, the point-wise one for Cahn-Hilliard: tests/test_gpu_action_entrywise.py).  Two processes share the GPU over tests/fake_rccl's double of librccl.so, as in
tests/test_gpu_comm.py; each is started once."""
import os
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE_RCCL = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 108.0, 1.0)
# name -> (p, N, periodic, form)
CASES = {"poisson-p3": (3, (6, 5, 9), (0, 0, 0), "poisson"), "cahnhilliard-p2-periodic": (2, (6, 6, 8), (1, 1, 1), "cahnhilliard")}


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _vectors(n):
    rng = np.random.default_rng(5)
    return rng.standard_normal(n), 0.63 + 0.05 * (2 * rng.random(n) - 1), rng.standard_normal(n)      # X, U, V


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
    p, N, periodic, form = CASES[name]
    g = P.IGX(3, 1)
    g.set_comm(world, rank)
    for i in range(3):
        g.axis_uniform(i, p, N[i], periodic=bool(periodic[i]))
    g.setup()
    if form == "poisson":
        for d in range(3):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 1.0 + d)
    g.set_form(form, CH if form == "cahnhilliard" else ())
    assert exchange.init_comm(g, transport="rccl") == "rccl"
    A = g.create_mat()                       # (for the row numbering only: nothing is assembled into it)
    nrow, _, maps = A.layout()
    ns = g.sizes()["node_sizes"]
    r = np.arange(A.nbrows)
    node = maps[0][0][r % nrow[0]].astype(np.int64) + ns[0] * (maps[1][0][(r // nrow[0]) % nrow[1]].astype(np.int64) + ns[1] * maps[2][0][r // (nrow[0] * nrow[1])].astype(np.int64))
    own = np.array([g.row_owned(int(a), int(b), int(c)) for a, b, c in zip(r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1]))])
    Xg, Ug, Vg = _vectors(int(np.prod(ns)))
    vecs = []
    for glob, junk in ((Xg, 3.0), (Ug, -7.0), (Vg, 9.0)):      # only the owner's values are set
        v = g.create_vec().set(np.where(own, glob[node], junk))
        g.refresh_ghosts(v)
        assert np.array_equal(v.get(), glob[node])
        vecs.append(v)
    X, U, V = vecs
    Y = g.create_vec()
    if form == "poisson":
        g.compute_matrix_action(X, Y)
    else:
        g.compute_ijacobian_action(1e3, V, 0.0, U, X, Y)
    assert "vec_sumfact" in g.kernel_name() and "action" in g.kernel_name(), g.kernel_name()
    g.reduce_ghost_rows(None, Y)
    g.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), row=node[own], val=Y.get()[own], bytes=g.comm_last_bytes())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_ranks_match_the_single_rank_oracle_product(name, tmp_path):
    import torch.multiprocessing as mp
    import oracle_api as O
    from common import make_pair
    p, N, periodic, form = CASES[name]
    mp.spawn(_rank_main, args=(2, _free_port(), name, str(tmp_path)), nprocs=2, join=True)
    orc, _ = make_pair(3, 1, p, list(N), periodic=[bool(x) for x in periodic], engine=False)
    n = orc.global_size()
    X, U, V = _vectors(n)
    if form == "poisson":
        for d in range(3):
            for s in range(2):
                orc.set_boundary_value(d, s, 0, 1.0 + d)
        M, tol = orc.compute_system("orc_form_poisson")[0].scipy(), 1e-12
    else:
        M, tol = orc.compute_ijacobian("orc_form_ch_tangent", O.CahnHilliardCtx(*CH), 1e3, V, 0.0, U).scipy(), 1e-11
    R, S, diag = M @ X, abs(M) @ np.abs(X), M.diagonal()
    off = abs(M)
    off.setdiag(0.0)
    fixed = np.asarray(off.sum(axis=1)).ravel() == 0.0
    Y, seen, sent = np.zeros(n), np.zeros(n, dtype=int), 0
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        Y[d["row"]] = d["val"]
        np.add.at(seen, d["row"], 1)
        sent += int(d["bytes"])
    assert sent > 0 and np.all(seen == 1)                # every row is owned by exactly one rank
    free = ~fixed
    err, scale = np.abs(Y - R)[free].max(), S[free].max()
    print("free rows: max|Y - R| = %.3e, max S = %.3e, ratio %.3e (tol %g); Dirichlet rows: %d" % (err, scale, err / scale, tol, fixed.sum()))
    assert err <= tol * scale
    assert fixed.any() == (form == "poisson")
    want = diag[fixed] * X[fixed]
    assert np.all(np.abs(Y[fixed] - want) <= 1e-12 * np.abs(want))
    # row by row against the long double reference of the single-rank operator: |Y_i - R_i| <= c u S_i
    import pointwise_ref as PW
    import tensor_ref as T
    if form == "poisson":
        ref = T.reference(orc, 3, T.poisson(3), bcs={(d, s, 0): 1.0 + d for d in range(3) for s in range(2)})
        Rl, Sl = ref.action(X)
    else:
        pw = PW.PointwiseRef(orc)
        ref, (Rl, Sl) = pw.tref, pw.ch_action(CH, 1e3, U, X)
    print("row by row: worst %.2f u S (c = %g)" % (PW.compare_rows(Y, Rl, Sl, T.C_ID, ref, name), T.C_ID))
