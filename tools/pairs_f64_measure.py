#!/usr/bin/env python3
"""Device and wall time of the fp64 separation census — pair_counts_f64(radii) — beside the radius-count pass, its yardstick, and beside
the route to the same answer without it: k calls of radius_counts_f64 and the host's sums.  On one GPU.

    python tools/pairs_f64_measure.py [--n 65536 1048576] [--rounds 6] [--out profiles/pairs_f64_measure.txt]

One context holds N bodies (fp64 state, a Plummer sphere).  Three regimes of k distinct radii, log-spaced:
    clustering   up to 0.1 of the half-mass radius (from 0.001 of it): most vectors of 64 d2 hold no pair within the largest radius, and
                 the wave leaves the chain of thresholds at the first compare
    spanning     from 0.01 of the half-mass radius to the system's diameter: the largest radius holds every pair, the chain is entered
                 for every vector and left where the vector's smallest d2 lies
    beyond       every radius beyond the diameter (up to 4 of them): every lane passes every threshold, the early exit NEVER fires —
                 the worst case, whatever the radii
Per regime and k in 1, 4, G = 16 and 64 a round runs, one after the other on the same state in the same process: pair_counts_f64 of k
radii, and the k-call route (radius_counts_f64(r).sum(dtype=int64) // 2 per radius), whose answers are asserted equal; once per regime one
radius_counts_f64 pass.  One warm-up round, then --rounds timed ones (at N > 262144 a third of them, at least two; the k-call route at
k = 64 then runs once: it is 64 equal passes).  wall = a host clock round the call(s), which end in a synchronise and the copy of the
results.  device = nbody_kernel_time's event pairs round the N^2 passes.  The measuring runs in a process of its own under a time limit;
if it ends with any status but 0 or runs out of time, nothing more is started on the device.  There is no CPU path: without a device
the run fails."""
import argparse
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 4, 16, 64)


def measure(nb, n, rounds):
    import numpy as np
    G = nb._lib.PAIR_RADII_PER_PASS
    assert G in KS
    p32, v32 = nb.ic_plummer(n, seed=1)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    F = nb._lib.KERNEL_FORCES
    big = n > 262144
    if big:
        rounds = max(2, rounds // 3)
    med = statistics.median
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm, vel)
        r_half = float(e.lagrange_f64((0.5,)).radius[0])
        diameter = 2.0 * float(np.sqrt((posm[:, :3] ** 2).sum(1).max()))
        regimes = (("clustering", 1e-3 * r_half, 0.1 * r_half), ("spanning", 1e-2 * r_half, diameter), ("beyond", 1.01 * diameter, 4.0 * diameter))
        _, cus = e.kernel_clock()
        print(f"# N = {n}, r_half = {r_half:.6g}, diameter <= {diameter:.6g}, {rounds} rounds behind 1 warm-up round; {cus} compute units; "
              f"G = {G} radii to a pass", flush=True)

        def timed(call):
            e.synchronize()
            f0 = e.kernel_time(F)
            t0 = time.perf_counter()
            got = call()
            w = (time.perf_counter() - t0) * 1e3
            f1 = e.kernel_time(F)
            return got, w, f1[0] - f0[0], f1[1] - f0[1]

        for name, lo, hi in regimes:
            sets = {k: (np.geomspace(lo, hi, k) if k > 1 else np.array([hi])) for k in KS}
            wall = {("pairs", k): [] for k in KS}; wall.update({("route", k): [] for k in KS}); wall["pass"] = []
            dev = {key: [] for key in wall}
            answer = {}
            for r in range(rounds + 1):
                got, w, d, p = timed(lambda: e.radius_counts_f64(float(sets[G][-1])))
                assert p == 1
                if r >= 1:
                    wall["pass"].append(w); dev["pass"].append(d)
                for k in KS:
                    got, w, d, p = timed(lambda: e.pair_counts_f64(sets[k]))
                    assert p == (k + G - 1) // G, (k, p)
                    answer[k] = got
                    if r >= 1:
                        wall["pairs", k].append(w); dev["pairs", k].append(d)
                    if k == 1 or (big and k == 64 and r != 1):      # k = 1: the route is the pass above; 64 at a large N: once
                        continue
                    got, w, d, p = timed(lambda: np.array([int(e.radius_counts_f64(float(x)).sum(dtype=np.int64)) // 2 for x in sets[k]], np.int64))
                    assert p == k and got.tolist() == answer[k].tolist(), (name, k)
                    if r >= 1:
                        wall["route", k].append(w); dev["route", k].append(d)
            one = med(dev["pass"])
            print(f"## {name}: k radii log-spaced in [{lo:.6g}, {hi:.6g}]; C(r) at k = {G}: first {int(answer[G][0])}, last {int(answer[G][-1])}", flush=True)
            print(f"radius_counts_f64, one pass  device {one:10.3f} ms (min {min(dev['pass']):10.3f}, max {max(dev['pass']):10.3f})  "
                  f"wall {med(wall['pass']):10.3f} ms", flush=True)
            for k in KS:
                d, w = dev["pairs", k], wall["pairs", k]
                passes = (k + G - 1) // G
                line = (f"pair_counts_f64 k = {k:2d}       device {med(d):10.3f} ms (min {min(d):10.3f}, max {max(d):10.3f})  wall {med(w):10.3f} ms"
                        f"  | {passes} pass(es), each {med(d) / passes / one:6.3f} x the radius-count pass")
                if k > 1:
                    rd, rw = dev["route", k], wall["route", k]
                    line += (f"  | {k} radius_counts_f64 calls + sums: device {med(rd):10.3f} ms, wall {med(rw):10.3f} ms ({len(rw)} run(s))"
                             f"  | route / pair_counts_f64: wall {med(rw) / med(w):7.2f}, device {med(rd) / med(d):7.2f}")
                print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 1 << 20], help="one measuring process per size, in this order")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="internal: measure the first --n in this process")
    ap.add_argument("--limit", type=int, default=900, help="seconds a measuring process may take")
    args = ap.parse_args()
    if args.child:
        import parallelnbody_amd as nb
        if nb.device_count() < 1:
            raise SystemExit("pairs_f64_measure: needs a HIP device")
        measure(nb, args.n[0], args.rounds)
        return 0
    lines = [f"# python tools/pairs_f64_measure.py --n {' '.join(str(n) for n in args.n)} --rounds {args.rounds} on one GPU, one context and one process per N",
             "# fp64 state, Plummer sphere; pair_counts_f64(k radii) against k calls of radius_counts_f64 and the host's sums (the same answers, asserted)",
             "# device = event pairs round the N^2 passes (nbody_kernel_time); wall = host clock round the call(s) incl. synchronise and the copy of the results"]
    print("\n".join(lines), flush=True)
    failed = 0
    for n in args.n:
        cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--rounds", str(args.rounds), "--child"]
        # the child's lines are passed on as they come (a regime at a time), so a run that stalls is seen to stall
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        timer = threading.Timer(args.limit, child.kill)
        timer.start()
        got = []
        for ln in child.stdout:
            got.append(ln.rstrip("\n"))
            print(got[-1], flush=True)
        err = child.stderr.read().strip().splitlines()
        rc = child.wait()
        late = not timer.is_alive()
        timer.cancel()
        lines += got
        if late:
            failed = 1
            lines.append(f"# the measuring process did not finish in {args.limit} s")
        elif rc != 0 or not got:
            failed = 1
            lines.append(f"# the measuring process ended with status {rc}: {err[-1] if err else 'no output'}")
        if failed:
            print(lines[-1], flush=True)
            break                                                  # nothing more is started on the device
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return failed


if __name__ == "__main__":
    sys.exit(main())
