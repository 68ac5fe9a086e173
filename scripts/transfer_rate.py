"""Measures IGXTransferProlong and IGXTransferRestrict (transfer.hpp) at 2x refinement per axis onto N^3 elements (default 256), p = 2 and
p = 3, dof 1 and dof 4: the prolongation on both paths (the fused kernel, the axis passes), the restriction on its gather passes.
Per configuration, by the host's clock over 20 calls between two synchronisations (timing off, nothing blocks inside) and by the call's
own events (IGXSetTiming: median of 10 after 3 warm-ups):
  the bytes the kernels ask for per fine dof, counted from shapes -- fused: every box's coarse footprint (taken from the tables, the
    re-reads of neighbouring boxes counted in full although the caches serve most of them) plus the fine box; passes: input plus output of
    every pass -- against the floor 8 (nc + nf) dof bytes of reading the coarse vector once and writing the fine one once;
  the time against IGXVecCopy of the FINE length measured in the same run by the same clock: the copy reads and writes the fine vector,
    16 bytes per fine dof, so a prolongation at the copy's byte rate would take (nc + nf) / (2 nf) of the copy's time (0.56 at 2x).
Appends to the output file (profiles/transfer.txt holds this script's and scripts/nested_newton.py's output).

    python scripts/transfer_rate.py [--size 256] [--out profiles/transfer.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from time_action import timed


def wall(g, call, calls=20, rounds=5):
    """ms per call by the host's clock: `calls` calls between two synchronisations, the median of `rounds` rounds after one warm-up round"""
    out = []
    for r in range(rounds + 1):
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        g.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return statistics.median(out[1:])


def asked_bytes(t, dof, path, down):
    """bytes the kernels ask for, from shapes and tables"""
    nf, nc = [t.sizes(d)[0] for d in range(3)], [t.sizes(d)[1] for d in range(3)]
    if path == "fused":
        box, foot = t.info()["box"], []
        for d in range(3):
            first, count, _ = t.axis(d)
            first, count = first.astype(np.int64), count.astype(np.int64)
            foot.append(sum(int((first[b:b + box[d]] + count[b:b + box[d]]).max() - first[b:b + box[d]].min()) for b in range(0, nf[d], box[d])))
        return 8 * dof * (foot[0] * foot[1] * foot[2] + nf[0] * nf[1] * nf[2])
    cur, total = list(nf if down else nc), 0
    for d in ((2, 1, 0) if down else (0, 1, 2)):
        before = cur[0] * cur[1] * cur[2]
        cur[d] = nc[d] if down else nf[d]
        total += 8 * dof * (before + cur[0] * cur[1] * cur[2])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer.txt"))
    a = ap.parse_args()
    import petiga_amd as P
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = a.size
    say(P.device_info())
    say("IGXTransfer, 2x per axis, %d^3 -> %d^3 elements; wall: host clock over 20 calls, timing off; events: the call's own, median of 10" % (N // 2, N))
    rng = np.random.default_rng(31)
    for p in (2, 3):
        for dof in (1, 4):
            c, f = P.IGX(3, dof), P.IGX(3, dof)
            for i in range(3):
                c.axis_uniform(i, p, N // 2)
                f.axis_uniform(i, p, N)
            c.setup()
            f.setup()
            t = f.transfer(c)
            Xc, Xf, Yf = c.create_vec(), f.create_vec(), f.create_vec()
            Xc.set(rng.uniform(-1, 1, Xc.n))
            nfd, ncd = Xf.n, Xc.n
            floor = 8 * (ncd + nfd)
            copy_ms = wall(f, lambda: Yf.copy_from(Xf))
            say("p = %d, dof %d: %d -> %d entries; IGXVecCopy of the fine length %.3f ms = %.0f GB/s (16 bytes per fine dof); floor %.2f bytes per fine dof; box %s, LDS %d bytes"
                % (p, dof, ncd, nfd, copy_ms, 16 * nfd / copy_ms / 1e6, floor / nfd, t.info()["box"], t.info()["lds_bytes"]))
            for what, path, call in (("prolong", "fused", lambda: t.prolong(Xc, Xf)), ("prolong", "axis", lambda: t.prolong(Xc, Xf)), ("restrict", "axis", lambda: t.restrict(Xf, Xc))):
                if what == "prolong":
                    t.set_path(path)
                w = wall(f, call)
                ev = timed(f, call)[0]
                b = asked_bytes(t, dof, path, what == "restrict")
                say("  %-8s %-6s wall %8.3f ms (events %8.3f ms) = %5.2f x the copy; asks for %6.2f bytes per fine dof (%.2f x the floor) -> %6.0f GB/s asked, %6.0f GB/s of the floor; %s"
                    % (what, path, w, ev, w / copy_ms, b / nfd, b / floor, b / w / 1e6, floor / w / 1e6, f.kernel_name()))
            t.close()
            del Xc, Xf, Yf, c, f
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
