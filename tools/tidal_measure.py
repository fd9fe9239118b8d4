"""Measurements of the tidal-tensor queries next to the potential's at the same shape (raw output:
profiles/tidal_measure.txt).

    python tools/tidal_measure.py

1  theta = 0, M = N = 65536 (reference box, distinct masses, eps = 0): tidal_at against potential_at, tidal() against potentials(), on
   one context, three alternating rounds
2  theta = 1, N = 65536 (Plummer sphere): tidal() against potentials() — the whole call (the diagnostic frame + the walk) and the walk
   alone (the call minus compute_forces() on the same context)
Device times are nbody_kernel_time's (HIP events around the queued unit), the clock nbody_kernel_clock's; every row is warmed up."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def points(m):
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(-1500, 1500, m), rng.uniform(-1500, 1500, m), rng.uniform(-300, 300, m)], 1).astype(np.float32)


def timed(e, call, reps=20, warm=3):
    """(device ms per call, shader clock in MHz)"""
    for _ in range(warm):
        call()
    e.kernel_time_reset()
    for _ in range(reps):
        call()
    ms, _ = e.kernel_time()
    return ms / reps, e.kernel_clock()[0]


def main():
    import parallelnbody_amd as nb
    n = 65536
    print(f"# library: {nb._lib.LIB_PATH}")
    print("# 1. theta = 0, M = N = 65536, eps = 0: device ms per call, shader clock")
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=n)
    pts = points(n)
    with nb.NBodyEngine(n, time_kernels=True) as e:
        e.set_state(posm, vel)
        for rnd in range(3):
            row = {}
            for name, call in (("potential_at", lambda: e.potential_at(pts)), ("tidal_at", lambda: e.tidal_at(pts)),
                               ("potentials", e.potentials), ("tidal", e.tidal)):
                row[name] = timed(e, call)
                print(f"round {rnd}  {name:<13s} {row[name][0]:8.4f} ms  {float(n) * n / (row[name][0] * 1e-3):.3e} /s  {row[name][1]:7.1f} MHz")
            print(f"round {rnd}  tidal_at / potential_at {row['tidal_at'][0] / row['potential_at'][0]:.3f}   tidal / potentials "
                  f"{row['tidal'][0] / row['potentials'][0]:.3f}")
    print("# 2. theta = 1, N = 65536, Plummer sphere: device ms per call — compute_forces(), potentials(), tidal(); the walks alone")
    posm, vel = nb.ic_plummer(n, seed=1)
    with nb.NBodyEngine(n, theta=1.0, time_kernels=True) as e:
        e.set_state(posm, vel)
        for rnd in range(3):
            f, _ = timed(e, e.compute_forces)
            p, _ = timed(e, e.potentials)
            t, _ = timed(e, e.tidal)
            print(f"round {rnd}  compute_forces {f:8.4f} ms  potentials {p:8.4f} ms  tidal {t:8.4f} ms  tidal / potentials {t / p:.3f}   "
                  f"walk alone: potential {p - f:7.4f} ms  tidal {t - f:7.4f} ms  ratio {(t - f) / (p - f):.3f}")


if __name__ == "__main__":
    main()
