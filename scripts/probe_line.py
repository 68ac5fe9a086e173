"""Usage example of IGX.probe: a Cahn-Hilliard run by IGXTimeStep (p = 2, periodic box, bench.py's parameters) that samples the
concentration along the diagonal of the box every few steps.  The state never leaves the device between the steps; a sample is one
probe evaluation of `--points` points (located once, before the first step) and one small copy.

    python scripts/probe_line.py [--size 32] [--steps 20] [--every 5] [--points 33] [--dt 1e-9]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--points", type=int, default=33)
    ap.add_argument("--dt", type=float, default=1e-9)
    a = ap.parse_args()
    import petiga_amd as P
    print(P.device_info(), flush=True)
    N = a.size
    g = P.IGX(3, 1)
    for i in range(3):
        g.axis_uniform(i, 2, N, periodic=True)
    g.setup()
    g.set_form("cahnhilliard", (1.5, 200.0, 0.63, 1.0, 1.0 / (3.0 * N * N), 1.0))
    U, V = g.create_vec(), g.create_vec()
    U.set(0.63 + 0.05 * (2 * np.random.default_rng(7).random(U.n) - 1))
    V.fill(0.0)
    s = np.linspace(0.0, 1.0, a.points)
    line = g.probe(np.stack([s, s, s], axis=-1), order=1)         # the diagonal (0,0,0) .. (1,1,1); order 1: the gradient is there too
    t, dt, done, resume = 0.0, a.dt, 0, False
    while done < a.steps:
        k = min(a.every, a.steps - done)
        info = g.time_step(U, V, dt, max_steps=k, rho_inf=0.5, t0=t, adapt=True, adapt_rtol=1e-3, adapt_atol=1e-3, resume=resume,
                           method="bicgstab", pc="none", lin_rtol=1e-4, lin_maxit=200, rtol=1e-3, maxit=8)
        if info["reason"] < 0:
            print("the stepper stopped: %s" % info["reason_name"])
            break
        t, dt, done, resume = info["t"], info["dt_next"], done + info["steps"], True
        c = line.evaluate(U)[:, 0]
        dc = line.evaluate(U, 1)[:, 0, :]
        print("step %3d  t = %.3e  c along the diagonal: min %.4f  mean %.4f  max %.4f   max |grad c| %.3f   (%s)"
              % (done, t, c.min(), c.mean(), c.max(), np.sqrt((dc ** 2).sum(axis=1)).max(), g.kernel_name()), flush=True)
    line.close()


if __name__ == "__main__":
    main()
