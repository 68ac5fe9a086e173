"""The ghost-row exchange INSIDE the library (include/petiga_amd.h: IGXCommInitRCCL / IGXCommInitTransport,
IGXReduceGhostRows, IGXRefreshGhosts): replaces MatAssemblyBegin/End + VecAssemblyBegin/End (src/petigaksp.c:197-200) and the
DMGlobalToLocal of IGAGetLocalVecArray (src/petigavec.c:256-269).

A GPU test machine has one GPU, so the N-rank flow runs as N processes sharing it.  Every case goes through the PRODUCT transport
(comm.hpp kind == 1: grouped ncclSend / ncclRecv on the exchange stream, three stream-ordered phases, receives posted ahead of the
assembly) bound to tests/fake_rccl's double of librccl.so ($IGX_RCCL_LIB), which keeps RCCL's ordering semantics -- stream-enqueued
operations, concurrent progress inside a group, ordered groups, rendezvous -- between processes on one device; a few cases also
run on the host-callback transport over gloo (kind == 2: the hook an MPI caller uses).  The real librccl.so is exercised on one
rank through IGXCommLoopbackTest.  Results are compared with the single-rank ORACLE."""
import os
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]      # (pytest.ini: at most four rank processes per test)

HERE = os.path.dirname(os.path.abspath(__file__))


def test_rccl_binding_loopback():
    import petiga_amd as P
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, 4)
    g.setup()
    uid = P.IGX.comm_unique_id()
    assert len(uid) == 128 and any(uid)
    g.comm_init_rccl(uid)
    assert g.comm_ranks() == ("rccl", 1)          # ncclCommCount of the library's communicator (bench.py prints it as rccl_ranks)
    assert g.comm_loopback_test(1 << 18) == 0.0
    # a reduction on the one-rank communicator: no neighbours, the three phases are empty groups that are never opened
    A, b = g.create_mat(), g.create_vec()
    g.set_form("poisson")
    g.compute_system(A, b)
    g.reduce_ghost_rows(A, b)
    g.synchronize()
    assert g.comm_early_phases() == 0
    g.comm_destroy()
    assert g.comm_ranks() == (None, 0)


def _free_port():
    """a free rendezvous port on the loop-back interface (test processes may run side by side: no port arithmetic)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _poisson_loads(g):
    """a Dirichlet face, loads on three others (IGASetBoundaryLoad): lumped by the per-face kernel next to the pencil kernel"""
    g.set_boundary_value(0, 0, 0, 0.5)
    g.set_boundary_load(0, 1, 0, 2.0)
    g.set_boundary_load(1, 0, 0, -0.75)
    g.set_boundary_load(2, 1, 0, 1.25)
    g.set_boundary_load(2, 0, 0, 0.4)


FAKE_RCCL = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")


def _rank_main(rank, world, port, case, outdir, name="", transport="rccl"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if transport == "rccl":
        os.environ.update(IGX_RCCL_LIB=FAKE_RCCL, FAKE_RCCL_TIMEOUT_S="90", IGX_LINK_PROBE_MB="8")
    if "pencil" in name:
        os.environ["IGX_OVERLAP"] = "1"       # the face-first passes whatever their cost (unset, the walk weighs it against the size of the faces: tiny here)
    if "combine" in name:
        os.environ["IGX_COMBINE"] = "1"
    if "split" in name and "block" not in name:
        os.environ["IGX_BLOCK_PENCIL"] = "0"      # these cases pin the feature kernel's two modes (the automatic choice takes the block pencil at p = 3)
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import petiga_amd as P
    from petiga_amd import exchange
    dim, dof, p, N, periodic, form, params = case
    g = P.IGX(dim, dof)
    g.set_comm(world, rank)
    for i in range(dim):
        g.axis_uniform(i, p, N[i], periodic=bool(periodic[i]))
    g.setup()
    if "nurbs" in name:        # the same rational control net on every rank (and in the oracle below); a rank keeps its ghosted box
        from common import make_pair, warped_geometry
        orc_geo, _ = make_pair(dim, dof, p, list(N), periodic=[bool(x) for x in periodic], engine=False)
        X, W = warped_geometry(orc_geo, dim, seed=7, rational=True, amp=0.08)
        g.set_geometry(X, W)
    if form == "poisson" and "loads" in name:
        _poisson_loads(g)
    elif form == "poisson":
        for d in range(dim):
            for s in range(2):
                g.set_boundary_value(d, s, 0, 1.0 + d)
    elif form == "elasticity":
        for f in range(3):
            g.set_boundary_value(0, 0, f, 0.0)
        g.set_boundary_value(2, 1, 0, 1.0)
        if "loads" in name:
            g.set_boundary_load(1, 1, 2, 0.5)
            g.set_boundary_load(2, 0, 1, -0.25)
    g.set_form(form, params)
    assert exchange.init_comm(g, transport=transport) == transport
    # the link rate of the face-first decision: measured over the transport when the communicator was created (a grouped
    # ncclSend / ncclRecv with every face neighbour; 8 MB here), the constant for a host transport
    gbs, source, probe_ms, faces = g.comm_link_rate()
    if transport == "rccl":
        assert source == "measured" and gbs > 0 and probe_ms > 0 and faces >= 1, (gbs, source, probe_ms, faces)
    else:
        assert (gbs, source) == (60.0, "constant")
    assert g.comm_ranks() == (transport, world)      # kind 1: ncclCommCount of the communicator the library created
    A, b = g.create_mat(), g.create_vec()
    n_global = int(np.prod(g.sizes()["node_sizes"])) * dof
    rng = np.random.default_rng(5)
    Ug, Vg = 0.63 + 0.05 * (2 * rng.random(n_global) - 1), rng.standard_normal(n_global)
    nrow, _, maps = A.layout()
    ns = g.sizes()["node_sizes"]
    r = np.arange(A.nbrows)
    node = maps[0][0][r % nrow[0]].astype(np.int64) + ns[0] * (maps[1][0][(r // nrow[0]) % nrow[1]].astype(np.int64) + ns[1] * maps[2][0][r // (nrow[0] * nrow[1])].astype(np.int64))
    own = np.array([g.row_owned(int(a), int(b_), int(c)) for a, b_, c in zip(r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1]))])
    loc = (node[:, None] * dof + np.arange(dof)[None, :]).reshape(-1)
    ownd = np.repeat(own, dof)
    if form == "cahnhilliard":
        # only the owner's values are set: the ghosts arrive through IGXRefreshGhosts
        U, V = g.create_vec().set(np.where(ownd, Ug[loc], -7.0)), g.create_vec().set(np.where(ownd, Vg[loc], 9.0))
        g.refresh_ghosts(U)
        g.refresh_ghosts(V)
        assert np.array_equal(U.get(), Ug[loc]) and np.array_equal(V.get(), Vg[loc])
        g.compute_ifunction(1e3, V, 0.0, U, b)
        g.compute_ijacobian(1e3, V, 0.0, U, A)
    else:
        g.compute_system(A, b)
    if "split" in name:       # the feature kernel makes the same two passes: more launches than colours on a rank with an upper neighbour
        has_upper = g.sizes()["proc_ranks"][2] < g.sizes()["proc_sizes"][2] - 1 or bool(periodic[2])
        ncol = int(np.prod(g.coloring()))
        if "block" in name:       # block_pencil.hpp: the upper half of axis 2 first, all 16 colours in both passes
            assert "block_pencil" in g.kernel_name() and g.dominant_kernel()["launches"] == (32 if has_upper else 16), (g.kernel_name(), g.dominant_kernel())
        elif "combine" in name:     # 16 colours over axes 1, 2; the face pass adds 3 of the 4 colours of axis 2
            assert "pencil walk" in g.kernel_name() and g.dominant_kernel()["launches"] == (28 if has_upper else 16)
        else:
            assert "feature_assemble" in g.kernel_name() and (g.dominant_kernel()["launches"] > ncol) == has_upper
    faces = None
    if "pencil" in name:
        # a communicator and upper neighbours: the elements next to the upper face of axis 2 are assembled first (all colours), then
        # those next to the upper face of axis 1, then the last p elements of every remaining pencil (the upper face of axis 0),
        # then the rest: the ghost rows of a face are complete when its pass ends (gram_mfma.hpp: three marks for the exchange)
        assert ("state_pencil" if form == "cahnhilliard" else "gram_pencil") in g.kernel_name(), g.kernel_name()
        sz = g.sizes()
        up = [sz["proc_sizes"][d] > 1 and (sz["proc_ranks"][d] < sz["proc_sizes"][d] - 1 or bool(periodic[d])) for d in range(3)]
        n = sz["elem_width"]
        can2, can1, can0 = up[2] and n[2] >= 2 * (p + 1), up[1] and n[1] >= 2 * (p + 1), up[0] and n[0] >= 16
        cut = lambda m: max(p + 1, min((m // 2) // (p + 1) * (p + 1), m - (p + 1)))      # face_cut (pencil_common.hpp): the upper half goes first
        ncol = lambda cnt: min(cnt, p + 1)
        r1, r2, launches = n[1], n[2], 0
        if can2:
            launches += ncol(r1) * ncol(n[2] - cut(n[2])); r2 = cut(n[2])
        if can1:
            launches += ncol(n[1] - cut(n[1])) * ncol(r2); r1 = cut(n[1])
        if can0:
            launches += ncol(r1) * ncol(r2)
        launches += ncol(r1) * ncol(r2)
        assert g.dominant_kernel()["launches"] == launches, (g.dominant_kernel(), launches, up, n)
        faces = int(can2) + int(can1) + int(can0)
    if "rewrite" in name:     # the vector is written again after the assembly marked its face: the mark no longer stands for it,
        b.set(2.0 * b.get())  # the reduction must pack the NEW values (comm.hpp: every writer clears the mark)
    g.reduce_ghost_rows(A, b)          # enqueued; the copies below wait on the engine stream
    if faces is not None:              # every face pass of the assembly started its phase of the exchange behind its own mark
        assert g.comm_early_phases() == (0 if "rewrite" in name else faces), (g.comm_early_phases(), faces)
    if "pencil" in name or "split" in name:
        has_upper = g.sizes()["proc_ranks"][2] < g.sizes()["proc_sizes"][2] - 1 or bool(periodic[2])
        if has_upper and "rewrite" not in name:      # the reduction started behind the face mark (on these tiny meshes, with the ranks sharing one GPU, the
            # sign of the lead is noise; bench.py reports it at size: 29 ms of a 46 ms assembly at 2 x 128^3 / 2)
            assert abs(g.comm_overlap_ms()) < 1e3
        else:
            with pytest.raises(P.IGXError):
                g.comm_overlap_ms()
    rows, cols, vals = A.to_coo_global()
    rp, _, _ = A.host()
    keep = np.repeat(np.repeat(own, np.diff(rp)), dof * dof)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), rows=rows[keep], cols=cols[keep], vals=vals[keep], vrow=loc[ownd], vval=b.get()[ownd],
             bytes=g.comm_last_bytes())
    dist.barrier()
    dist.destroy_process_group()


CASES = {
    "poisson-p3-2ranks": (2, (3, 1, 3, (6, 5, 9), (0, 0, 0), "poisson", ())),
    "poisson-p2-4ranks-periodic": (4, (3, 1, 2, (8, 8, 8), (1, 0, 1), "poisson", ())),
    "poisson-p3-2ranks-pencil-loads": (2, (3, 1, 3, (8, 6, 16), (0, 0, 0), "poisson", ())),
    "poisson-p2-4ranks-pencil-loads": (4, (3, 1, 2, (9, 12, 12), (0, 0, 0), "poisson", ())),
    "poisson-p2-4ranks-pencil": (4, (3, 1, 2, (16, 12, 12), (0, 0, 0), "poisson", ())),      # [2,1,2]: faces and an edge (a [2,2,2] grid needs eight processes on the GPU; test_gpu_parity.py covers its corners in one)
    "poisson-p2-4ranks-pencil-faces": (4, (3, 1, 2, (24, 12, 12), (0, 0, 0), "poisson", ())),  # ... longer on axis 0
    "poisson-p3-4ranks-pencil-faces": (4, (3, 1, 3, (24, 16, 16), (0, 0, 0), "poisson", ())),
    "poisson-p3-4ranks-pencil-faces-periodic": (4, (3, 1, 3, (12, 16, 16), (0, 1, 1), "poisson", ())),
    "poisson-p3-4ranks-pencil-faces-nurbs": (4, (3, 1, 3, (8, 16, 16), (0, 0, 0), "poisson", ())),         # the mapped-geometry walk, [1,2,2]: the passes of axes 2 and 1
    "cahnhilliard-p2-4ranks-pencil-faces": (4, (3, 1, 2, (24, 12, 12), (0, 0, 0), "cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / 108.0, 1.0))),   # the Tangent's walk
    "poisson-p3-2ranks-pencil": (2, (3, 1, 3, (8, 9, 17), (0, 0, 0), "poisson", ())),
    "poisson-p3-2ranks-pencil-rewrite": (2, (3, 1, 3, (8, 9, 17), (0, 0, 0), "poisson", ())),
    "poisson-p3-2ranks-pencil-periodic": (2, (3, 1, 3, (8, 8, 16), (0, 0, 1), "poisson", ())),
    "elasticity-p3-2ranks-split-combine": (2, (3, 3, 3, (8, 5, 16), (0, 0, 0), "elasticity", (1.5, 0.8))),   # pencil mode of the feature kernel
    "elasticity-p3-2ranks-split": (2, (3, 3, 3, (8, 5, 16), (0, 0, 0), "elasticity", (1.5, 0.8))),
    "elasticity-p3-2ranks-split-block-loads": (2, (3, 3, 3, (8, 5, 16), (0, 0, 0), "elasticity", (1.5, 0.8))),   # block pencil, upper face of axis 2 first
    "elasticity-p3-4ranks-split-block": (4, (3, 3, 3, (9, 16, 16), (0, 0, 0), "elasticity", (1.5, 0.8))),
    "elasticity-p3-2ranks-split-block-periodic": (2, (3, 3, 3, (8, 8, 16), (0, 0, 1), "elasticity", (1.5, 0.8))),
    "elasticity-p2-2ranks-split": (2, (3, 3, 2, (5, 6, 13), (0, 0, 0), "elasticity", (1.5, 0.8))),
    "cahnhilliard-p2-2ranks-split": (2, (3, 1, 2, (6, 6, 12), (1, 1, 1), "cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / 108.0, 1.0))),
    "cahnhilliard-p2-2ranks": (2, (3, 1, 2, (6, 6, 8), (1, 1, 1), "cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / 108.0, 1.0))),
    # ranks of two elements at p = 3 ([1,1,3]): rank 0's ghost layer belongs to ranks 1 AND 2 -- two messages up, one of them skipping a rank
    "poisson-p3-3ranks-thin": (3, (3, 1, 3, (4, 4, 6), (0, 0, 0), "poisson", ())),
    # one element per rank on a periodic axis of 2p + 1 functions ([1,1,4], widths 2,1,1,1): the ghost layers of ranks 1, 2 and 3 reach two
    # ranks, those of ranks 2 and 3 across the seam
    "poisson-p2-4ranks-periodic-wrap": (4, (3, 1, 2, (2, 2, 5), (0, 0, 1), "poisson", ())),
}
# the host-callback transport (kind == 2) keeps a few cases: both list shapes, the refresh, the face passes
HOST_CASES = ["poisson-p3-2ranks", "poisson-p2-4ranks-pencil-faces", "cahnhilliard-p2-2ranks"]
MAX_RANKS = 4           # rank processes one test may start (pytest.ini)
assert all(w <= MAX_RANKS for w, _ in CASES.values())


@pytest.mark.parametrize("name,transport", [(n, "rccl") for n in sorted(CASES)] + [(n, "host") for n in HOST_CASES])
def test_library_exchange_matches_single_rank_oracle(name, transport, tmp_path):
    import torch.multiprocessing as mp
    import oracle_api as O
    from common import make_pair
    world, case = CASES[name]
    dim, dof, p, N, periodic, form, params = case
    port = _free_port()
    mp.spawn(_rank_main, args=(world, port, case, str(tmp_path), name, transport), nprocs=world, join=True)
    orc, _ = make_pair(dim, dof, p, list(N), periodic=[bool(x) for x in periodic], engine=False)
    if "nurbs" in name:
        from common import warped_geometry
        X, W = warped_geometry(orc, dim, seed=7, rational=True, amp=0.08)
        orc.set_geometry(X, W)
    if form == "poisson" and "loads" in name:
        _poisson_loads(orc)
        A_o, b_o = orc.compute_system("orc_form_poisson")
    elif form == "poisson":
        for d in range(dim):
            for s in range(2):
                orc.set_boundary_value(d, s, 0, 1.0 + d)
        A_o, b_o = orc.compute_system("orc_form_poisson")
    elif form == "elasticity":
        for f in range(3):
            orc.set_boundary_value(0, 0, f, 0.0)
        orc.set_boundary_value(2, 1, 0, 1.0)
        if "loads" in name:
            orc.set_boundary_load(1, 1, 2, 0.5)
            orc.set_boundary_load(2, 0, 1, -0.25)
        A_o, b_o = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*params))
    else:
        ctx = O.CahnHilliardCtx(*params)
        rng = np.random.default_rng(5)
        n = orc.global_size()
        Ug, Vg = 0.63 + 0.05 * (2 * rng.random(n) - 1), rng.standard_normal(n)
        b_o = orc.compute_ifunction("orc_form_ch_residual", ctx, 1e3, Vg, 0.0, Ug)
        A_o = orc.compute_ijacobian("orc_form_ch_tangent", ctx, 1e3, Vg, 0.0, Ug)
    M_o = A_o.scipy().tocoo()
    n = M_o.shape[0]
    ko = M_o.row.astype(np.int64) * n + M_o.col
    import scipy.sparse as sp
    # explicit zeros included on the engine side: compare as dense-free dictionaries of the oracle's pattern
    ref = sp.csr_matrix((A_o.val, A_o.colidx, A_o.rowptr), shape=(n, n))
    rows, cols, vals, vrow, vval, sent = [], [], [], [], [], 0
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        rows.append(d["rows"]); cols.append(d["cols"]); vals.append(d["vals"]); vrow.append(d["vrow"]); vval.append(d["vval"]); sent += int(d["bytes"])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    assert sent > 0
    # every owned row appears exactly once over the ranks, with the oracle's pattern
    key = rows * n + cols
    o = np.argsort(key, kind="stable")
    orow = np.repeat(np.arange(n, dtype=np.int64), np.diff(A_o.rowptr))
    ko = orow * n + A_o.colidx.astype(np.int64)
    oo = np.argsort(ko, kind="stable")
    assert np.array_equal(key[o], ko[oo])
    from common import free_row_scale
    scale = free_row_scale(orow[oo], A_o.colidx.astype(np.int64)[oo], A_o.val[oo])     # rows without a Dirichlet condition (tests/common.py)
    assert np.abs(vals[o] - A_o.val[oo]).max() <= 1e-11 * scale
    vrow, vval = np.concatenate(vrow), np.concatenate(vval)
    assert np.array_equal(np.sort(vrow), np.arange(n))
    if "rewrite" in name:
        b_o = 2.0 * b_o
    assert np.abs(vval[np.argsort(vrow)] - b_o).max() <= 1e-11 * np.abs(b_o).max()
    del ref, ko
