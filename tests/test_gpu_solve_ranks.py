"""IGXSolve on 2 and 4 ranks (include/petiga_amd.h; petiga_amd/csrc/solve_loops.hpp, krylov.hpp, comm.hpp): the device loop on a partition, its
inner products added across the ranks in rank order, its sweeps over the owned rows alone.  Ranks are processes that share the GPU over
tests/fake_rccl's double of librccl.so, as in tests/test_gpu_matrix_action_ranks.py; every rank process is started once per test, runs all
of that test's cases and writes one .npz.  The cases are tests/solve_ranks_cases.py's: one contiguous prefix (Poisson, cut on axis 2), runs of
3 nown0 doubles with an odd length and an odd start (elasticity, cut on axis 0), four ranks as 2 x 2 x 1 (Bratu), a periodic seam
(Cahn-Hilliard).  Every test asserts the shape it claims and fails with "the case tests nothing" otherwise.
The yardstick is the host loop of tests/krylov_ref.py on a ONE-rank engine's operators (krylov_ref.engine_callables), the oracle's matrix
the reference of every true residual:
  ownership        every row is owned exactly once
  counts           CG within 1 of the host loop, BiCGStab within BICG_MARGIN (tests/test_solve_ranks_abi.py holds the rule on the CPU)
  history          the first min(k, 5) entries agree with the host loop's to RANKS_HISTORY_RTOL
  true residual    |b - A_o x| <= max(2 rtol |b|, 8 x the host loop's own)
  across ranks     info and history are the same bits on every rank; a second solve gives the same bits
RANKS_HISTORY_RTOL is measured: 8 x the largest relative deviation of a head entry seen on these cases on an MI355X (the figure stands at
the constant below and in DESIGN.md 3.25); every test prints what it sees before it asserts (run with -s)."""
import os
import sys

import numpy as np
import pytest

import krylov_ref as K
import solve_ranks_cases as SR

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("gpu_procs")]

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE_RCCL = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
RANKS_HISTORY_RTOL = 8 * 5.4e-14      # measured: the largest relative deviation of a head entry is 5.37e-14 (Poisson p = 3, CG with Jacobi, 2 ranks); the other cases stay below 4e-15
INFO_KEYS = ("iterations", "reason", "rnorm0", "rnorm", "bnorm")


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


class _Rank:
    """one case on one rank: the engine on its part, the numbering of its rows, the state vectors with their ghosts"""

    def __init__(self, name, world, rank, outdir, transport="rccl"):
        import petiga_amd as P
        from petiga_amd import exchange
        c = SR.EVERY[name]
        self.name, self.c, self.rank = name, c, rank
        g = self.g = SR.configure(P.IGX(3, c["dof"]), name, comm=(world, rank))
        g.set_form(c["form"], SR.FORM_PARAMS[c["form"]])
        assert exchange.init_comm(g, transport=transport) == transport
        A = g.create_mat()                       # (for the row numbering only: nothing is assembled into it)
        nrow, _, maps = A.layout()
        ns = g.sizes()["node_sizes"]
        r = np.arange(A.nbrows)
        r0, r1, r2 = r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1])
        node = maps[0][0][r0].astype(np.int64) + ns[0] * (maps[1][0][r1].astype(np.int64) + ns[1] * maps[2][0][r2].astype(np.int64))
        own0, own1, own2 = (np.array([g.row_owned(*[k if e == d else 0 for e in range(3)]) for k in range(nrow[d])]) for d in range(3))
        own = own0[r0] & own1[r1] & own2[r2]                # (the owned rows are a box: row by row, tests/test_gpu_matrix_action_ranks.py asks the same of IGXRowOwned)
        dof = c["dof"]
        self.entry = (node[:, None] * dof + np.arange(dof)[None, :]).ravel()       # global entry of every local entry
        self.own = np.repeat(own, dof)
        self.nrow = [int(v) for v in nrow]
        self.nown = [int(own.reshape(nrow[2], nrow[1], nrow[0])[0, 0, :].sum()), int(own.reshape(nrow[2], nrow[1], nrow[0])[0, :, 0].sum()),
                     int(own.reshape(nrow[2], nrow[1], nrow[0])[:, 0, 0].sum())]
        self.rhs = np.load(os.path.join(outdir, "rhs_%s.npy" % name))
        U, V = SR.states(name, self.rhs.size)
        self.U, self.V = (None if s is None else self.vec(s, junk=-7.0, refresh=True) for s in (U, V))
        self.kw = SR.solve_keywords(name, self.U, self.V)

    def vec(self, glob, junk=np.nan, refresh=False):
        """a vector with the owner's values of `glob` and `junk` in its ghost rows"""
        v = self.g.create_vec().set(np.where(self.own, glob[self.entry], junk))
        if refresh:
            self.g.refresh_ghosts(v)
        return v

    def solve(self, method, pc, rhs=None, x0=None, junk=0.0, **kw):
        b = self.vec(self.rhs if rhs is None else rhs, junk=junk)
        x = self.vec(np.zeros(self.rhs.size) if x0 is None else x0, junk=junk)
        args = dict(method=method, pc=pc, rtol=self.c["rtol"], maxit=self.c["maxit"], history=True)
        args.update(self.kw)
        args.update(kw)
        info = self.g.solve(b, x, **args)
        self.g.synchronize()
        return x.get().copy(), info


def _store(out, key, x, info):
    out[key + ".x"], out[key + ".hist"] = x, info["history"]
    out[key + ".info"] = np.array([float(info[k]) for k in INFO_KEYS])


def _rank_main(rank, world, port, job, names, outdir):
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
    out = {}
    for name in names:
        rk = _Rank(name, world, rank, outdir)
        g = rk.g
        out[name + ".entry"], out[name + ".own"] = rk.entry, rk.own
        out[name + ".nrow"], out[name + ".nown"] = np.array(rk.nrow), np.array(rk.nown)
        if job == "cases":
            for method, pc in rk.c["solves"]:
                key = "%s.%s.%s" % (name, method, pc)
                x, info = rk.solve(method, pc)
                _store(out, key, x, info)
                out[key + ".kernel"] = np.array(g.kernel_name())
                x2, info2 = rk.solve(method, pc)
                _store(out, key + ".again", x2, info2)
        elif job == "long":      # NaN in every ghost row of b and x, two iterations from x = 0
            for method, pc in rk.c["solves"]:
                _store(out, "%s.%s.%s" % (name, method, pc), *rk.solve(method, pc, junk=np.nan))
        elif job == "ghosts":
            method, pc = rk.c["solves"][0]
            x0 = np.random.default_rng(8).standard_normal(rk.rhs.size)
            _store(out, name + ".clean", *rk.solve(method, pc, x0=x0, junk=0.0))
            _store(out, name + ".nan", *rk.solve(method, pc, x0=x0, junk=np.nan))
        elif job == "sums":
            part = [1e16, 1.0, -1e16, 1.0][rank] if world == 4 else float(rank)
            out["one"] = g.comm_all_sum([part])
            out["three"] = g.comm_all_sum([float(rank + 1), 2.0 ** 40 * (rank + 1), -3.0 * rank])
            ones = rk.vec(np.ones(rk.rhs.size), junk=5.0)
            out["dot"] = g.comm_all_sum([ones.dot(ones)])
        elif job == "transports":      # the same solve and the same sum over the host transport: a second engine of this rank
            method, pc = rk.c["solves"][-1]
            _store(out, "rccl", *rk.solve(method, pc))
            host = _Rank(name, world, rank, outdir, transport="host")
            _store(out, "host", *host.solve(method, pc))
            out["host.kernel"] = np.array(host.g.kernel_name())
            out["host.sum"] = host.g.comm_all_sum([1e16 * (1 - 2 * rank), 1.0 + rank, 0.5])
            host.g.synchronize()
        elif job == "outcomes":
            zero = np.zeros(rk.rhs.size)
            _store(out, "zero", *rk.solve("cg", "jacobi", rhs=zero, x0=np.ones(rk.rhs.size)))
            _store(out, "maxit3", *rk.solve("cg", "jacobi", maxit=3))
            _store(out, "maxit3.again", *rk.solve("cg", "jacobi", maxit=3))
            bad = rk.rhs.copy()
            bad[np.load(os.path.join(outdir, "nan_entry.npy"))] = np.nan      # an entry rank 1 owns
            _store(out, "nan", *rk.solve("cg", "jacobi", rhs=bad))
            try:
                rk.solve("cg", "fastdiag")
                out["fastdiag"] = np.array([0.0])
            except P.IGXError as e:
                out["fastdiag"] = np.array([float(e.code)])
                out["fastdiag.why"] = np.array(str(e))
            _store(out, "after", *rk.solve("cg", "jacobi"))
        g.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


def _run(job, names, world, tmp_path, rhs):
    import torch.multiprocessing as mp
    for name in names:
        np.save(os.path.join(str(tmp_path), "rhs_%s.npy" % name), rhs[name])
    mp.spawn(_rank_main, args=(world, _free_port(), job, names, str(tmp_path)), nprocs=world, join=True)
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]


_ONE_RANK = {}


def _one_rank(name):
    """(engine on one rank, right-hand side, solve keywords, the oracle's matrix): made once per case, never written to"""
    if name not in _ONE_RANK:
        import petiga_amd as P
        c = SR.CASES[name]
        eng = SR.configure(P.IGX(3, c["dof"]), name)
        eng.set_form(c["form"], SR.FORM_PARAMS[c["form"]])
        A_s, b_o = SR.oracle_system(name)
        if c["form"] in ("poisson", "elasticity"):      # the engine's own load vector
            A, bv = eng.create_mat(), eng.create_vec()
            eng.compute_system(A, bv)
            eng.synchronize()
            rhs = bv.get().copy()
        else:
            rhs = b_o
        rhs.setflags(write=False)
        U, V = SR.states(name, rhs.size)
        kw = SR.solve_keywords(name, *(None if s is None else eng.create_vec().set(s) for s in (U, V)))
        _ONE_RANK[name] = (eng, rhs, kw, A_s)
    return _ONE_RANK[name]


def _gather(ranks, name, key, n):
    """the ranks' owned rows of x put together, and how often every entry was owned"""
    x, seen = np.zeros(n), np.zeros(n, dtype=int)
    for d in ranks:
        own, entry = d[name + ".own"], d[name + ".entry"]
        x[entry[own]] = d[key + ".x"][own]
        np.add.at(seen, entry[own], 1)
    return x, seen


def _same_on_all_ranks(ranks, key):
    for d in ranks[1:]:
        assert np.array_equal(d[key + ".info"], ranks[0][key + ".info"], equal_nan=True), key + ": info differs between the ranks"
        assert np.array_equal(d[key + ".hist"], ranks[0][key + ".hist"], equal_nan=True), key + ": the history differs between the ranks"


def _shape(ranks, name):
    """what the owned rows of the ranks look like: a list of (run length, number of runs, parities of the run starts)"""
    dof = SR.EVERY[name]["dof"]
    shapes = []
    for d in ranks:
        nrow, nown = d[name + ".nrow"], d[name + ".nown"]
        if nown[0] == nrow[0] and nown[1] == nrow[1]:
            shapes.append((int(dof * nrow[0] * nrow[1] * nown[2]), 1, {0}))
        elif nown[0] == nrow[0]:
            shapes.append((int(dof * nrow[0] * nown[1]), int(nown[2]), {int(dof * nrow[0] * nrow[1] * j) & 1 for j in range(nown[2])}))
        else:
            shapes.append((int(dof * nown[0]), int(nown[1] * nown[2]), {int(dof * nrow[0] * (i + nrow[1] * j)) & 1 for i in range(nown[1]) for j in range(nown[2])}))
    return shapes


def _check_shape(ranks, name):
    shapes = _shape(ranks, name)
    print("%s: runs per rank (length, count, start parities) %s" % (name, shapes))
    nothing = "the case tests nothing"
    if name in ("poisson-axis2", "ch-seam-axis2"):
        assert all(count == 1 for _, count, _ in shapes), nothing
        assert any(d[name + ".nown"][2] < d[name + ".nrow"][2] for d in ranks), nothing          # a rank holds ghost rows behind its prefix
    elif name == "elasticity-axis0":
        assert any(count > 1 and length % 2 == 1 and 1 in par for length, count, par in shapes), nothing     # odd runs that start at odd entries
        assert all(length % 3 == 0 for length, _, _ in shapes), nothing
    else:
        cut0 = [d[name + ".nown"][0] < d[name + ".nrow"][0] for d in ranks]
        cut1 = [d[name + ".nown"][1] < d[name + ".nrow"][1] for d in ranks]
        assert len(shapes) == 4, nothing
        assert any(cut0) and any(c1 and not c0 for c0, c1 in zip(cut0, cut1)), nothing      # runs of nown0 nodes, and runs of nrow0 nown1 nodes
        assert any(count == 1 and not c0 and not c1 for (_, count, _), c0, c1 in zip(shapes, cut0, cut1)), nothing      # the top rank: its whole box, one run


def _against_the_host_loop(ranks, name, method, pc):
    from test_gpu_krylov_solve import BICG_MARGIN      # (imported here: a rank process that loads this module needs none of that one's)
    c = SR.CASES[name]
    eng, rhs, kw, A_s = _one_rank(name)
    key = "%s.%s.%s" % (name, method, pc)
    loop, margin = (K.cg, 1) if method == "cg" else (K.bicgstab, BICG_MARGIN)
    op, prec = K.engine_callables(eng, pc=pc, **kw)
    b = np.array(rhs)
    x_ref, ref = loop(op, prec, b, rtol=c["rtol"], maxit=c["maxit"])
    x, seen = _gather(ranks, name, key, b.size)
    assert np.all(seen == 1)                                   # every row is owned exactly once
    _same_on_all_ranks(ranks, key)
    _same_on_all_ranks(ranks, key + ".again")
    hist, info = ranks[0][key + ".hist"], dict(zip(INFO_KEYS, ranks[0][key + ".info"]))
    k, k_ref = int(info["iterations"]), ref["iterations"]
    m = min(k, k_ref, 5)
    dev = np.abs(hist[:m + 1] - ref["history"][:m + 1]) / ref["history"][:m + 1]
    bn = np.linalg.norm(b)
    res, res_ref = np.linalg.norm(b - A_s @ x), np.linalg.norm(b - A_s @ x_ref)
    kernel = str(ranks[0][key + ".kernel"])
    print("%s: %d iterations (host loop %d), reason %d; head of the history deviates by %.3e; true residual / |b| %.3e (host loop %.3e); %s"
          % (key, k, k_ref, info["reason"], dev.max(), res / bn, res_ref / bn, kernel))
    assert info["reason"] == K.CONVERGED_RTOL == ref["reason"]
    assert abs(k - k_ref) <= margin
    assert hist.size == k + 1 and info["rnorm"] == hist[-1] and info["rnorm0"] == hist[0] and info["rnorm"] <= c["rtol"] * info["bnorm"]
    assert dev.max() <= RANKS_HISTORY_RTOL
    assert res <= max(2 * c["rtol"] * bn, 8 * res_ref)
    assert kernel.startswith("krylov(%s, pc=%s, vec_sumfact" % (method, pc)) and kernel.endswith(", %d iterations, %d ranks)" % (k, len(ranks))), kernel
    for d in ranks:                                            # a second solve: the same bits in every row and in the history
        assert np.array_equal(d[key + ".x"], d[key + ".again.x"]) and np.array_equal(d[key + ".hist"], d[key + ".again.hist"]), "two solves differ"
        assert not np.isnan(d[key + ".x"]).any()
    return dev.max()


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_partitioned_solve_against_the_host_loop(name, tmp_path):
    rhs = _one_rank(name)[1]
    ranks = _run("cases", [name], SR.world(name), tmp_path, {name: rhs})
    _check_shape(ranks, name)
    worst = max(_against_the_host_loop(ranks, name, method, pc) for method, pc in SR.CASES[name]["solves"])
    print("%s: the largest relative deviation of a head entry is %.3e (RANKS_HISTORY_RTOL %.3e)" % (name, worst, RANKS_HISTORY_RTOL))


def test_ghost_rows_are_never_summed(tmp_path):
    """b and the guess in x with NaN in every row the rank does not own: the same bits in every owned row and in the history as with clean
    ghosts, and no NaN anywhere in x on return (the final refresh)"""
    name = "elasticity-axis0"
    ranks = _run("ghosts", [name], 2, tmp_path, {name: _one_rank(name)[1]})
    _check_shape(ranks, name)
    assert any((~d[name + ".own"]).any() for d in ranks), "the case tests nothing"      # a rank holds rows it does not own
    for d in ranks:
        own = d[name + ".own"]
        assert np.array_equal(d[name + ".nan.hist"], d[name + ".clean.hist"]) and np.array_equal(d[name + ".nan.info"], d[name + ".clean.info"])
        assert np.array_equal(d[name + ".nan.x"][own], d[name + ".clean.x"][own])
        assert not np.isnan(d[name + ".nan.x"]).any()
        assert d[name + ".clean.info"][1] == K.CONVERGED_RTOL and d[name + ".clean.info"][0] > 0
    _same_on_all_ranks(ranks, name + ".nan")


def test_comm_all_sum_adds_in_rank_order_on_four_ranks(tmp_path):
    name = "bratu-2x2"
    ranks = _run("sums", [name], 4, tmp_path, {name: _one_rank(name)[1]})
    for r, d in enumerate(ranks):
        print("rank %d: %r %r" % (r, d["one"], d["three"]))
        assert d["one"].tolist() == [1.0]                      # ((1e16 + 1) - 1e16) + 1: any other order gives 0 or 2
        assert d["three"].tolist() == [10.0, 2.0 ** 40 * 10, -18.0]


def test_vec_dot_and_comm_all_sum_give_the_global_length(tmp_path):
    name = "poisson-axis2"
    rhs = _one_rank(name)[1]
    ranks = _run("sums", [name], 2, tmp_path, {name: rhs})
    for d in ranks:
        assert d["dot"].tolist() == [float(rhs.size)]
        assert d["one"].tolist() == [1.0]


def test_outcomes_and_refusals_on_two_ranks(tmp_path):
    name = "poisson-axis2"
    eng, rhs, kw, A_s = _one_rank(name)
    owned = SR.owned_sets(name)
    np.save(os.path.join(str(tmp_path), "nan_entry.npy"), owned[1][owned[1].size // 2])
    ranks = _run("outcomes", [name], 2, tmp_path, {name: rhs})
    info = lambda d, key: dict(zip(INFO_KEYS, d[key + ".info"]))
    for key in ("zero", "maxit3", "maxit3.again", "nan", "after"):
        _same_on_all_ranks(ranks, key)
    op, prec = K.engine_callables(eng, pc="jacobi")
    x_ref, ref = K.cg(op, prec, np.array(rhs), rtol=SR.CASES[name]["rtol"], maxit=3)
    x3, seen = _gather(ranks, name, "maxit3", rhs.size)
    assert np.all(seen == 1)
    print("third iterate: max|x - x_ref| / max|x_ref| = %.3e" % (np.abs(x3 - x_ref).max() / np.abs(x_ref).max()))
    for d in ranks:
        z = info(d, "zero")
        assert z["reason"] == K.CONVERGED_ATOL and z["iterations"] == 0 and z["rnorm"] == 0.0 and z["bnorm"] == 0.0 and not d["zero.x"].any()
        m = info(d, "maxit3")
        assert m["reason"] == K.DIVERGED_ITS == ref["reason"] and m["iterations"] == 3 and d["maxit3.hist"].size == 4
        assert np.array_equal(d["maxit3.x"], d["maxit3.again.x"]) and np.array_equal(d["maxit3.hist"], d["maxit3.again.hist"])
        assert info(d, "nan")["reason"] == K.DIVERGED_NAN
        assert d["fastdiag"].tolist() == [56.0] and "fast diagonalisation" in str(d["fastdiag.why"]) and "Krylov solve" in str(d["fastdiag.why"])
        assert info(d, "after")["reason"] == K.CONVERGED_RTOL
    # x after three steps is the host loop's third iterate up to the summation order of nine inner products
    assert np.abs(x3 - x_ref).max() <= 1e-10 * np.abs(x_ref).max()
    assert np.abs(ranks[0]["maxit3.hist"] - ref["history"]).max() <= RANKS_HISTORY_RTOL * ref["history"].max()


def test_sweep_timing_hook_runs_every_sweep_in_both_forms():
    """IGXKrylovSweepTime on a stand-alone rank 0 of 2 cut on axis 1 (runs of 42 x 5 nodes: two chunks of 64 pairs each, several runs):
    every sweep launches in the run form and in the contiguous one and reports a positive time; a solve on the same engine's space is
    refused as before (no communicator), so the hook needs none"""
    import petiga_amd as P
    g = P.IGX(3, 1)
    g.set_comm(2, 0)
    for i, (N, procs) in enumerate(((40, 1), (8, 2), (4, 1))):
        g.set_processors(i, procs)
        g.axis_uniform(i, 2, N)
    g.setup()
    s = g.sizes()
    assert s["node_lwidth"][0] == s["node_gwidth"][0] and s["node_lwidth"][1] < s["node_gwidth"][1], "the case tests nothing"
    assert s["node_lwidth"][0] * s["node_lwidth"][1] > 128 and s["node_lwidth"][2] > 1, "the case tests nothing"
    for name in P.KRYLOV_SWEEPS:
        t = [g.krylov_sweep_time(name, runs, reps=2) for runs in (True, False)]
        print("%-10s runs %.4f ms, contiguous %.4f ms" % (name, t[0], t[1]))
        assert t[0] > 0 and t[1] > 0


def test_host_transport_gives_the_bits_of_rccl(tmp_path):
    """IGXCommInitTransport instead of RCCL: one call of the callback with every other rank as peer carries a rank sum, and the solve's
    info, history and x are the bits of the RCCL path; IGXCommAllSum adds in rank order there too"""
    name = "poisson-axis2"
    ranks = _run("transports", [name], 2, tmp_path, {name: _one_rank(name)[1]})
    _same_on_all_ranks(ranks, "host")
    for d in ranks:
        assert np.array_equal(d["host.hist"], d["rccl.hist"]) and np.array_equal(d["host.info"], d["rccl.info"]) and np.array_equal(d["host.x"], d["rccl.x"])
        assert d["host.info"][1] == K.CONVERGED_RTOL and str(d["host.kernel"]).endswith("2 ranks)")
        assert d["host.sum"].tolist() == [0.0, 3.0, 1.0]


def test_sweeps_past_one_item_per_wavefront(tmp_path):
    """The run sweeps where a wavefront takes more than one (run, chunk) item, so that the stepping of KR_RUN_SWEEP's position counters decides
    which entries are visited (tests/solve_ranks_cases.py: LONG_CASES): 2704 runs of one chunk; 1089 runs of three chunks with starts of either parity, where the chunk
    counter carries into the run counters; on the top rank one run of more than 2048 chunks.  Two iterations of CG with Jacobi and of
    BiCGStab from x = 0 on 2 ranks, NaN in every ghost row of b and x, against the host loop on a one-rank engine.
    Bound: the loops differ by the order of their sums of n terms -- gamma_n relative each (tests/krylov_ref.py) -- and by the action's
    rounding across the cut (1e-12 of its scale, tests/test_gpu_matrix_action_ranks.py), carried through two steps: 16 gamma_n + 1e-11 of
    max|x| for x and of |r_k| for the history.  A sweep that skips or repeats one entry in n moves a sum by about 1 / n, which is
    2^53 / 16 n^2 > 1000 times that at these lengths, and leaves x = 0 or 2 alpha p where it does."""
    import petiga_amd as P
    names = sorted(SR.LONG_CASES)
    engines, rhs = {}, {}
    for name in names:
        engines[name] = eng = SR.configure(P.IGX(3, 1), name)
        eng.set_form("poisson")
        rhs[name] = np.random.default_rng(41).standard_normal(eng.create_vec().n)
    ranks = _run("long", names, 2, tmp_path, rhs)
    nothing = "the case tests nothing"
    for name in names:
        c, (low, top) = SR.LONG_CASES[name], _shape(ranks, name)
        chunks = lambda length: max(1, ((length >> 1) + 63) >> 6)
        print("%s: runs per rank (length, count, start parities) %s, chunks per run %d and %d" % (name, [low, top], chunks(low[0]), chunks(top[0])))
        assert low[1] * chunks(low[0]) > 2048 and top[1] == 1, nothing
        if name == "poisson-long-runs":
            assert chunks(low[0]) > 1 and 2048 % chunks(low[0]) != 0 and chunks(top[0]) > 2048 and 1 in low[2], nothing
        assert any((~d[name + ".own"]).any() for d in ranks), nothing
        b, n = rhs[name], rhs[name].size
        tol = 16 * K.gamma(n) + 1e-11
        for method, pc in c["solves"]:
            key = "%s.%s.%s" % (name, method, pc)
            op, prec = K.engine_callables(engines[name], pc=pc)
            x_ref, ref = (K.cg if method == "cg" else K.bicgstab)(op, prec, b, rtol=0.0, maxit=2)
            x, seen = _gather(ranks, name, key, n)
            assert np.all(seen == 1)
            _same_on_all_ranks(ranks, key)
            hist, info = ranks[0][key + ".hist"], dict(zip(INFO_KEYS, ranks[0][key + ".info"]))
            dx, dh = np.abs(x - x_ref).max() / np.abs(x_ref).max(), (np.abs(hist - ref["history"]) / ref["history"]).max()
            print("%s: n = %d, max|x - x_ref| / max|x_ref| = %.3e, history deviates by %.3e (bound %.3e)" % (key, n, dx, dh, tol))
            assert info["iterations"] == 2 == ref["iterations"] and info["reason"] == K.DIVERGED_ITS == ref["reason"]
            assert all(not np.isnan(d[key + ".x"]).any() for d in ranks)
            assert dx <= tol and dh <= tol
