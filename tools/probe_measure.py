"""Measurements of the field queries and tracers (raw output: profiles/probe_field_and_tracers.txt).

    python tools/probe_measure.py [--parts 1,2,3] [--lib PATH]

1  rate of probe_tile_pk_kernel at M = N = 65536 against forces_tile_pk_kernel on an NBODY_ALGO_TILED context of the same N
2  nbody_field_at for 2^20 points: device time and the whole call
3  what 2^20 tracers add to a step
--lib: another build of the library (part 1's tile-kernel rows only make sense there, e.g. the parent commit's).
Device times are nbody_kernel_time's (HIP events around the queued unit); every row is warmed up first."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(nb, n):
    return nb.ic_reference_box(n, 1000.0, seed=n)            # distinct masses: the kernels' general form


def points(m):
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(-1500, 1500, m), rng.uniform(-1500, 1500, m), rng.uniform(-300, 300, m)], 1).astype(np.float32)


def clock(e):
    mhz, cus = e.kernel_clock()
    return f"{mhz:7.1f} MHz" if mhz > 0 else "    n/a    "


def tile_rate(nb, n, eps, reps=20):
    posm, vel = scene(nb, n)
    with nb.NBodyEngine(n, algorithm=nb._lib.ALGO_TILED, eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        for _ in range(5):
            e.compute_forces()
        e.kernel_time_reset()
        for _ in range(reps):
            e.compute_forces()
        ms, k = e.kernel_time()
        cfg = e.launch_config()
        return ms / k, float(n) * n / (ms / k * 1e-3), clock(e), cfg


def probe_rate(nb, n, m, eps, theta=0.0, reps=20):
    posm, vel = scene(nb, n)
    pts = points(m)
    with nb.NBodyEngine(n, eps=eps, theta=theta, time_kernels=True) as e:
        e.set_state(posm, vel)
        if theta > 0:
            e.compute_forces()
        for _ in range(3):
            e.field_at(pts)
        e.kernel_time_reset()
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            e.field_at(pts)
            walls.append(time.perf_counter() - t0)
        ms, k = e.kernel_time()
        return ms / k, float(n) * m / (ms / k * 1e-3), clock(e), 1e3 * float(np.median(walls))


def step_time(nb, n, theta, tracers, steps=200, timed=False):
    posm, vel = scene(nb, n)
    with nb.NBodyEngine(n, theta=theta, time_kernels=timed) as e:
        e.set_state(posm, vel)
        if tracers:
            e.set_tracers(points(tracers))
        e.step(0.01, 20); e.synchronize()
        if timed:
            e.kernel_time_reset()
        t0 = time.perf_counter()
        e.step(0.01, steps); e.synchronize()
        wall = (time.perf_counter() - t0) / steps
        dev = None
        if timed:
            f_ms, k = e.kernel_time(nb._lib.KERNEL_FORCES)
            u_ms, _ = e.kernel_time(nb._lib.KERNEL_UPDATE)
            dev = (f_ms + u_ms) / k
        return wall * 1e6, dev * 1e3 if dev is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["NBODY_AMD_LIB"] = a.lib
    import parallelnbody_amd as nb
    parts = {int(x) for x in a.parts.split(",")}
    new = hasattr(nb.lib(), "nbody_field_at")
    print(f"# library: {nb._lib.LIB_PATH}  (field queries: {'yes' if new else 'no'})")
    n = 65536
    if 1 in parts:
        print("# 1. M = N = 65536, distinct masses: device ms per pass, interactions/s, shader clock")
        for eps, env, label in ((0.0, None, "eps = 0 (tile kernel: bare tiles outside the own range)"),
                                (0.0, "1", "eps = 0, NBODY_SYM_GUARDED=1 (tile kernel: every tile guarded)"),
                                (0.05, None, "eps = 0.05 (both softened)")):
            if env:
                os.environ["NBODY_SYM_GUARDED"] = env
            ms, rate, clk, cfg = tile_rate(nb, n, eps)
            os.environ.pop("NBODY_SYM_GUARDED", None)
            print(f"forces_tile_pk_kernel  {label:66s} {ms:8.3f} ms  {rate:.3e} /s  {clk}  tile {cfg['tile']} ipt {cfg['i_per_thread']} j_split {cfg['j_split']}")
            if new and not env:
                ms, rate, clk, _ = probe_rate(nb, n, n, eps)
                print(f"probe_tile_pk_kernel   {'eps = %g (always guarded) + probe_fold_kernel' % eps:66s} {ms:8.3f} ms  {rate:.3e} /s  {clk}")
    if 2 in parts and new:
        print("# 2. nbody_field_at, 2^20 points: device ms, whole call ms (staging and copies included)")
        for nn in (2000, 65536):
            for theta in (0.0, 1.0):
                ms, rate, clk, wall = probe_rate(nb, nn, 1 << 20, 0.0, theta=theta, reps=10)
                print(f"N = {nn:6d} theta = {theta:g}: device {ms:8.3f} ms   call {wall:8.3f} ms   {clk}")
    if 3 in parts and new:
        print("# 3. a step with and without 2^20 tracers: wall us per step (200 steps queued, one wait) | device us per step (events)")
        for nn, theta in ((2000, 0.0), (2000, 1.0), (65536, 1.0)):
            for tr in (0, 1 << 20):
                wall, _ = step_time(nb, nn, theta, tr)
                _, dev = step_time(nb, nn, theta, tr, timed=True)
                print(f"N = {nn:6d} theta = {theta:g} tracers = {tr:7d}: {wall:10.1f} us | {dev:10.1f} us")


if __name__ == "__main__":
    main()
