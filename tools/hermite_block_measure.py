"""What Hermite block time steps cost and buy on the device (raw output: profiles/hermite_block_measure.txt).

    python tools/hermite_block_measure.py [--out FILE] [--sizes 256,1024,4096,16384,65536] [--table 4096,65536]

Scene: ic_plummer(N) in fp64 with bodies 0 and 1 made a binary of eccentricity 0.5 whose period is 0.0125 (their own masses; the
semi-major axis follows), 45 times shorter than the sphere's median |a| / |j|; eps = 0, eta = 0.02, dt_max = 0.01, 12 levels.
  frame     one frame of dt_max covered by nbody_hermite_block_advance(1) and by nbody_hermite_advance(dt_max) at the same eta, each from
            a valid cache (the first evaluation is outside the window), after one warm-up frame of each:
              wall    host clock around the call and a synchronise, on a context WITHOUT time_kernels — what a user waits for; a block
                      step makes the host wait once, for 16 bytes
              device  nbody_kernel_time (HIP events around the queued units) on a second context WITH time_kernels: forces + update
            and the relative energy error of the frame (nbody_energy before and after)
  table     one block step against the size m of its active set: level_in puts the first m bodies at level 1 of 1, the rest at level 0,
            so the first block step has exactly those m; five repetitions (each a fresh session: restart, begin, step), the median
            wall time, the median device times and which lane shape the evaluation took
Everything is warmed up before it is timed; a toy N measures launches, which is the point of the small rows."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT_MAX, LEVELS, ETA, PERIOD = 0.01, 12, 0.02, 0.0125


def scene(nb, n, G=1.0e4):
    p32, v32 = nb.ic_plummer(n, seed=n)
    p, v = p32.astype(np.float64), v32.astype(np.float64)
    m1, m2 = p[0, 3], p[1, 3]
    M, e = m1 + m2, 0.5
    a = (G * M * (PERIOD / (2 * np.pi)) ** 2) ** (1.0 / 3.0)
    rp, vp = a * (1 - e), np.sqrt(G * M * (1 + e) / (a * (1 - e)))
    centre = np.array([30.0, 20.0, 10.0])
    p[0, :3] = centre + [-rp * m2 / M, 0, 0]; p[1, :3] = centre + [rp * m1 / M, 0, 0]
    v[0, :3] = [0, -vp * m2 / M, 0]; v[1, :3] = [0, vp * m1 / M, 0]
    v[:, 3] = 0.0
    return p, v, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hermite_block_measure.txt"))
    ap.add_argument("--sizes", default="256,1024,4096,16384,65536")
    ap.add_argument("--table", default="4096,65536")
    a = ap.parse_args()
    import parallelnbody_amd as nb
    from parallelnbody_amd import _lib
    F, U = _lib.KERNEL_FORCES, _lib.KERNEL_UPDATE
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    say("# python tools/hermite_block_measure.py on one MI355X, one session")
    say(f"# fp64 state, eps = 0, Plummer sphere + one binary of period {PERIOD}, eta = {ETA}, dt_max = {DT_MAX}, {LEVELS} levels")
    say("# frame: one frame of dt_max; wall = host clock incl. synchronise (no time_kernels), device = nbody_kernel_time forces + update")
    wins = []
    for n in [int(x) for x in a.sizes.split(",")]:
        p, v, sma = scene(nb, n)
        res = {}
        for timed in (False, True):
            with nb.NBodyEngine(n, precision="f64", time_kernels=timed) as e:
                for scheme in ("block", "shared"):
                    for warm in (True, False):
                        e.set_state(p, v)
                        e0 = sum(e.energy())
                        if scheme == "block":
                            e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
                        else:
                            e.hermite_timescale()
                        e.synchronize()
                        if timed:
                            e.kernel_time_reset()
                        t0 = time.perf_counter()
                        if scheme == "block":
                            st = e.hermite_block_advance(1)
                            steps, pairs = st["block_steps"], st["pairs"]
                        else:
                            _, steps = e.hermite_advance(DT_MAX, eta=ETA, dt_max=DT_MAX)
                            pairs = steps * n * n
                        e.synchronize()
                        wall = (time.perf_counter() - t0) * 1e3
                        if warm:
                            continue
                        if timed:
                            res[scheme, "device"] = (e.kernel_time(F)[0], e.kernel_time(U)[0])
                        else:
                            err = abs(sum(e.energy()) - e0) / abs(e0)
                            res[scheme, "wall"] = (wall, steps, pairs, err)
                            if scheme == "block":
                                res["extra"] = (st["body_steps"] / steps, st["level_max"], st["floor_hits"])
        say(f"N={n:6d}  binary a = {sma:.4f}")
        for scheme in ("block", "shared"):
            wall, steps, pairs, err = res[scheme, "wall"]
            f_ms, u_ms = res[scheme, "device"]
            say(f"  frame {scheme:6s} wall {wall:10.3f} ms  device {f_ms + u_ms:10.3f} ms = forces {f_ms:10.3f} + update {u_ms:9.3f}  "
                f"steps {steps:6d}  pairs {pairs:.3e}  |dE/E| {err:.2e}")
        mean_m, level_max, floor = res["extra"]
        ratio = res["shared", "wall"][0] / res["block", "wall"][0]
        say(f"  block: mean active set {mean_m:.1f}, deepest level {level_max}, floor hits {floor}; shared / block wall {ratio:.2f}, "
            f"pairs {res['shared', 'wall'][2] / res['block', 'wall'][2]:.1f}")
        wins.append((n, ratio))
    first = next((n for n, r in wins if r > 1.0 and all(r2 > 1.0 for n2, r2 in wins if n2 >= n)), None)
    say(f"# block stepping wins (wall) from N = {first} on among {[n for n, _ in wins]}" if first else "# block stepping wins at none of these N")

    say()
    say("# table: one block step against its active set's size m (median of 5; wall incl. the wait for 16 bytes and a synchronise)")
    for n in [int(x) for x in a.table.split(",")]:
        p, v, _ = scene(nb, n)
        for m in [x for x in (1, 2, 64, 512, 4096) if x < n] + [n]:
            level_in = np.zeros(n, np.int32)
            level_in[:m] = 1
            rows = {}
            for timed in (False, True):
                with nb.NBodyEngine(n, precision="f64", time_kernels=timed) as e:
                    e.set_state(p, v)
                    got = []
                    for rep in range(6):                           # (the first one warms up)
                        e.hermite_restart()
                        e.hermite_block_begin(DT_MAX, 1, eta=ETA, level_in=level_in)
                        e.synchronize()
                        if timed:
                            e.kernel_time_reset()
                        t0 = time.perf_counter()
                        st = e.hermite_block_advance(1, max_block_steps=1)
                        e.synchronize()
                        wall = (time.perf_counter() - t0) * 1e3
                        assert st["body_steps"] == m, (st, m)
                        got.append((e.kernel_time(F)[0], e.kernel_time(U)[0]) if timed else (wall,))
                    rows[timed] = [statistics.median(c) for c in zip(*got[1:])]
            lanes = 1 if m <= 1024 else 2
            say(f"N={n:6d} m={m:6d}  wall {rows[False][0]:9.4f} ms  device forces {rows[True][0]:9.4f} + update {rows[True][1]:8.4f} ms  "
                f"{lanes} bod{'y' if lanes == 1 else 'ies'} per lane  pairs/s (device forces) {m * n / (rows[True][0] * 1e-3):.3e}")
    out.close()


if __name__ == "__main__":
    main()
