"""Measurements of the jerk queries next to the potential's and the tidal tensor's at the same shape (raw output:
profiles/jerk_measure.txt).

    python tools/jerk_measure.py

N = 65536 (reference box, distinct masses, eps = 0), theta = 0:
1  fp32 state, M = N: jerk_at against potential_at and tidal_at, jerk() against potentials() and tidal(), on one context, three
   alternating rounds
2  fp64 state: jerk(np.float64), three rounds
Device times are nbody_kernel_time's (HIP events around the queued unit), `call` the median on the host clock round the whole call
(staging, copies and the wait included); every row is warmed up."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def points(m):
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(-1500, 1500, m), rng.uniform(-1500, 1500, m), rng.uniform(-300, 300, m)], 1).astype(np.float32)


def timed(e, call, reps=20, warm=3):
    """(device ms per call, median wall ms per call)"""
    for _ in range(warm):
        call()
    e.kernel_time_reset()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    ms, _ = e.kernel_time()
    return ms / reps, 1e3 * float(np.median(walls))


def main():
    import parallelnbody_amd as nb
    n = 65536
    print("# python tools/jerk_measure.py on one MI355X, one session")
    print("# 1. fp32 state, theta = 0, M = N = 65536, eps = 0: device ms per call")
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=n)
    pts = points(n)
    pv = np.random.default_rng(11).normal(0.0, 300.0, (n, 3)).astype(np.float32)
    with nb.NBodyEngine(n, time_kernels=True) as e:
        e.set_state(posm, vel)
        for rnd in range(3):
            row = {}
            for name, call in (("potential_at", lambda: e.potential_at(pts)), ("tidal_at", lambda: e.tidal_at(pts)),
                               ("jerk_at", lambda: e.jerk_at(pts, pv)), ("potentials", e.potentials), ("tidal", e.tidal), ("jerk", e.jerk)):
                row[name], wall = timed(e, call)
                print(f"round {rnd}  {name:<13s} {row[name]:8.4f} ms  {float(n) * n / (row[name] * 1e-3):.3e} /s  call {wall:7.3f} ms")
            print(f"round {rnd}  jerk_at / potential_at {row['jerk_at'] / row['potential_at']:.3f}   jerk_at / tidal_at "
                  f"{row['jerk_at'] / row['tidal_at']:.3f}   jerk / potentials {row['jerk'] / row['potentials']:.3f}   jerk / tidal "
                  f"{row['jerk'] / row['tidal']:.3f}")
    print("# 2. fp64 state, theta = 0, N = 65536, eps = 0: device ms per call of jerk(np.float64)")
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm.astype(np.float64), vel.astype(np.float64))
        for rnd in range(3):
            ms, wall = timed(e, lambda: e.jerk(np.float64), reps=5, warm=1)
            print(f"round {rnd}  jerk f64      {ms:8.4f} ms  {float(n) * n / (ms * 1e-3):.3e} /s  call {wall:7.3f} ms")


if __name__ == "__main__":
    main()
