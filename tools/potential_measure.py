"""Measurements of the potential queries (raw output: profiles/potential_measure.txt).

    python tools/potential_measure.py [--parts 1,2,3,4,5]

1  theta = 0 rate at M = N = 65536, eps 0 and 0.05: probe_pot_pk_kernel + pot_fold_kernel (nbody_potential_at) against
   probe_tile_pk_kernel + probe_fold_kernel (nbody_field_at) on the same context, in the same run
2  theta = 1: potentials() at N = 65536 and 2^20 on Plummer spheres — the walk alone (the call's two passes minus the diagnostic
   frame it runs first) against compute_forces() on the same context
3  energy_fast() against energy(): whole calls on the host clock, theta = 0 at N = 65536 and energy_fast() at theta = 1, N = 2^20
4  for information: the largest relative deviation of the theta = 1 potentials from the direct sum at N = 2000
5  energy() at N = 2^20, once (all pairs in fp64: seconds)
Device times are nbody_kernel_time's (HIP events around the queued unit), the clock nbody_kernel_clock's; every row is warmed up."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def points(m):
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(-1500, 1500, m), rng.uniform(-1500, 1500, m), rng.uniform(-300, 300, m)], 1).astype(np.float32)


def clock(e):
    mhz, _ = e.kernel_clock()
    return f"{mhz:7.1f} MHz" if mhz > 0 else "    n/a    "


def timed(e, call, reps, warm=3, dev=True):
    """(device ms per call, passes per call, median wall ms per call, clock); dev = False (a context without timers): the wall time only"""
    for _ in range(warm):
        call()
    if dev:
        e.kernel_time_reset()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    if not dev:
        return None, None, 1e3 * float(np.median(walls)), None
    ms, k = e.kernel_time()
    return ms / reps, k / reps, 1e3 * float(np.median(walls)), clock(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3,4")
    a = ap.parse_args()
    import parallelnbody_amd as nb
    parts = {int(x) for x in a.parts.split(",")}
    print(f"# library: {nb._lib.LIB_PATH}")
    if 1 in parts:
        n = 65536
        print("# 1. M = N = 65536 (reference box, distinct masses), theta = 0: device ms per query, interactions/s, shader clock; three rounds, alternating")
        posm, vel = nb.ic_reference_box(n, 1000.0, seed=n)
        pts = points(n)
        for eps in (0.0, 0.05):
            with nb.NBodyEngine(n, eps=eps, time_kernels=True) as e:
                e.set_state(posm, vel)
                for rnd in range(3):
                    for name, call in (("probe_tile_pk_kernel + probe_fold_kernel (field_at)    ", lambda: e.field_at(pts)),
                                       ("probe_pot_pk_kernel + pot_fold_kernel (potential_at)  ", lambda: e.potential_at(pts)),
                                       ("probe_pot_pk_kernel<SELF> + pot_fold_kernel (potentials)", lambda: e.potentials())):
                        ms, _, wall, clk = timed(e, call, 20)
                        print(f"eps = {eps:<5g} round {rnd}  {name} {ms:8.4f} ms  {float(n) * n / (ms * 1e-3):.3e} /s  {clk}  call {wall:7.3f} ms")
    if 2 in parts:
        print("# 2. theta = 1, Plummer spheres: device ms — compute_forces() (build + walk), potentials() (that + the potential walk), the walk alone, its ratio to compute_forces()")
        for n in (65536, 1 << 20):
            posm, vel = nb.ic_plummer(n, seed=1)
            with nb.NBodyEngine(n, theta=1.0, time_kernels=True) as e:
                e.set_state(posm, vel)
                f_ms, f_k, f_wall, _ = timed(e, e.compute_forces, 20)
                p_ms, p_k, p_wall, _ = timed(e, e.potentials, 20)
                f2_ms, _, _, _ = timed(e, e.compute_forces, 20)
                f = 0.5 * (f_ms + f2_ms)
                print(f"N = {n:8d}: compute_forces {f_ms:8.4f} / {f2_ms:8.4f} ms ({f_k:g} pass)   potentials {p_ms:8.4f} ms ({p_k:g} passes)   "
                      f"walk alone {p_ms - f:8.4f} ms = {(p_ms - f) / f:5.2f} x compute_forces   calls: {f_wall:7.3f} / {p_wall:7.3f} ms")
    if 3 in parts:
        print("# 3. whole calls on the host clock, median of 10 (ms): energy_fast() against energy()")
        n = 65536
        posm, vel = nb.ic_plummer(n, seed=1)
        with nb.NBodyEngine(n, eps=1.0) as e:
            e.set_state(posm, vel)
            _, _, slow, _ = timed(e, e.energy, 10, warm=1, dev=False)
            _, _, fast, _ = timed(e, e.energy_fast, 10, dev=False)
            (k0, p0), (k1, p1) = e.energy(), e.energy_fast()
            print(f"theta = 0 N = {n}: energy {slow:10.3f} ms   energy_fast {fast:8.3f} ms   ({slow / fast:6.1f} x)   pe rel diff {abs(p1 - p0) / abs(p0):.2e}  ke rel diff {abs(k1 - k0) / abs(k0):.1e}")
        n = 1 << 20
        posm, vel = nb.ic_plummer(n, seed=1)
        with nb.NBodyEngine(n, theta=1.0) as e:
            e.set_state(posm, vel)
            _, _, fast, _ = timed(e, e.energy_fast, 10, dev=False)
            _, _, frame, _ = timed(e, e.compute_forces, 10, dev=False)
            k1, p1 = e.energy_fast()
            print(f"theta = 1 N = {n}: energy_fast {fast:8.3f} ms   (compute_forces {frame:8.3f} ms)   ke {k1:.9e} pe {p1:.9e}")
    if 4 in parts:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from bh_pot_ref import direct_potential
        n = 2000
        g = np.load(os.path.join(ROOT, "tests", "golden", "refbox_n2000_seed1.npz"))
        posm, vel = np.ascontiguousarray(g["posm"], np.float32), np.ascontiguousarray(g["vel"], np.float32)
        ref = direct_potential(posm[:, :3], posm[:, 3], posm[:, :3], skip_self=True)
        with nb.NBodyEngine(n, theta=1.0) as e:
            e.set_state(posm, vel)
            got = e.potentials().astype(np.float64)
            _, pe = e.energy_fast()
        dev = np.abs(got - ref) / np.abs(ref)
        pe0 = 0.5 * float(np.sum(posm[:, 3].astype(np.float64) * ref))
        print(f"# 4. theta = 1, N = 2000 (the shipped scene): potentials against the direct sum: max rel deviation {dev.max():.3e}, median {np.median(dev):.3e}; "
              f"pe rel deviation {abs(pe - pe0) / abs(pe0):.3e}")
    if 5 in parts:
        n = 1 << 20
        posm, vel = nb.ic_plummer(n, seed=1)
        with nb.NBodyEngine(n, theta=1.0) as e:
            e.set_state(posm, vel)
            t0 = time.perf_counter()
            k0, p0 = e.energy()
            slow = time.perf_counter() - t0
            k1, p1 = e.energy_fast()
            print(f"# 5. theta = 1 N = {n}: energy() once {slow * 1e3:10.1f} ms   ke {k0:.9e} pe {p0:.9e}   energy_fast pe rel deviation {abs(p1 - p0) / abs(p0):.3e}")


if __name__ == "__main__":
    main()
