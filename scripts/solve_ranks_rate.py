"""Times what IGXSolve on a partition adds to the one-rank loop (profiles/solve_ranks.txt):
  1. every run-structured sweep of krylov.hpp against its contiguous sibling on the same number of entries (IGXKrylovSweepTime): a
     stand-alone engine as rank 0 of 2, cut on axis 0, on axis 1 and on axis 2, no communicator, Poisson p = 3 at --size^3 elements.  3
     untimed launches, then --rounds rounds of --reps launches; the median of the rounds' means and their spread (min .. max).  The run form
     pays the scalar head and tail of its runs; the ratio is reported, nothing is gated on it.
  2. the time per CG iteration (Jacobi, a fixed number of iterations: rtol = atol = 0) on one rank and on two ranks that share the GPU over
     the test double of librccl.so (tests/fake_rccl), by the host's clock with timing off, and next to it the same number of rank sums
     (IGXCommAllSum) and ghost exchanges (IGXRefreshGhosts + IGXReduceGhostRows) timed alone.  Two ranks on one GPU share its memory system and
     talk through host memory: the figures say what the loop adds in calls, nothing about links.

    python scripts/solve_ranks_rate.py [--size 128] [--reps 20] [--rounds 7] [--its 20] [--part sweeps,cg]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

FAKE_RCCL = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
P_DEG = 3


def engine(size, comm=None, axis=2):
    import petiga_amd as P
    g = P.IGX(3, 1)
    if comm is not None:
        g.set_comm(*comm)
        for i in range(3):
            g.set_processors(i, comm[0] if i == axis else 1)
    for i in range(3):
        g.axis_uniform(i, P_DEG, size)
    g.setup()
    for d in range(3):
        for s in range(2):
            g.set_boundary_value(d, s, 0, 0.0)
    g.set_form("poisson")
    return g


def sweeps(a):
    import petiga_amd as P
    print(P.device_info(), flush=True)
    for axis in range(3):
        g = engine(a.size, comm=(2, 0), axis=axis)
        s = g.sizes()
        own, box = s["node_lwidth"], s["node_gwidth"]
        print("rank 0 of 2 cut on axis %d: owns %s of the %s nodes it holds, %d entries (%.1f MB per vector)"
              % (axis, own, box, int(np.prod(own)), 8 * np.prod(own) / 1e6), flush=True)
        for name in P.KRYLOV_SWEEPS:
            t = {form: [g.krylov_sweep_time(name, form, a.reps) for _ in range(a.rounds)] for form in (True, False)}
            run, flat = statistics.median(t[True]), statistics.median(t[False])
            print("  %-10s runs %.4f ms (%.4f .. %.4f), contiguous %.4f ms (%.4f .. %.4f), runs / contiguous = %.3f"
                  % (name, run, min(t[True]), max(t[True]), flat, min(t[False]), max(t[False]), run / flat), flush=True)
        del g


def cg_rank(rank, world, port, a):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", IGX_RCCL_LIB=FAKE_RCCL, FAKE_RCCL_TIMEOUT_S="90", IGX_LINK_PROBE_MB="8")
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from petiga_amd import exchange
    g = engine(a.size, comm=(world, rank) if world > 1 else None)
    if world > 1:
        assert exchange.init_comm(g, transport="rccl") == "rccl"
    b, x = g.create_vec(), g.create_vec()
    g.compute_vector(b)
    if world > 1:
        g.reduce_ghost_rows(None, b)
    g.synchronize()

    def clock(fn, rounds):
        out = []
        for k in range(-2, rounds):
            g.synchronize()
            t0 = time.perf_counter()
            fn()
            g.synchronize()
            if k >= 0:
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), min(out), max(out)

    def solve():
        x.fill(0.0)
        info = g.solve(b, x, method="cg", pc="jacobi", rtol=0.0, atol=0.0, maxit=a.its)
        assert info["iterations"] == a.its, info

    t = clock(solve, a.rounds)
    line = "%d rank(s), rank %d, n = %d local entries: CG + Jacobi %.3f ms per iteration (%.3f .. %.3f), %s" % (world, rank, b.n, t[0] / a.its, t[1] / a.its, t[2] / a.its, g.kernel_name())
    if world > 1:
        def sums():
            for _ in range(2 * a.its):
                g.comm_all_sum([1.0, 2.0])

        def exchanges():
            for _ in range(a.its):
                g.refresh_ghosts(x)
                g.reduce_ghost_rows(None, x)

        ts, te = clock(sums, a.rounds), clock(exchanges, a.rounds)
        line += "\n    alone: 2 rank sums %.3f ms per iteration (%.3f .. %.3f), 1 refresh + 1 reduction %.3f ms per iteration (%.3f .. %.3f): %.0f %% of the iteration" % (
            ts[0] / a.its, ts[1] / a.its, ts[2] / a.its, te[0] / a.its, te[1] / a.its, te[2] / a.its, 100.0 * (ts[0] + te[0]) / t[0])
    print(line, flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--its", type=int, default=20)
    ap.add_argument("--part", default="sweeps,cg")
    a = ap.parse_args()
    if "sweeps" in a.part:
        sweeps(a)
    if "cg" in a.part:
        import torch.multiprocessing as mp
        print("Poisson p = %d, %d^3 elements, CG with Jacobi, %d iterations per solve" % (P_DEG, a.size, a.its), flush=True)
        for world in (1, 2):
            mp.spawn(cg_rank, args=(world, _free_port(), a), nprocs=world, join=True)


if __name__ == "__main__":
    main()
