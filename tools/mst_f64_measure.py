#!/usr/bin/env python3
"""Device and wall time of the fp64 minimum spanning tree — mst_f64() — beside the radius-count pass, its yardstick, on one GPU.

    python tools/mst_f64_measure.py [--n 65536 1048576] [--rounds 10] [--out profiles/mst_f64_measure.txt]

One context holds N bodies (fp64 state, a Plummer sphere).  A round runs, one after the other on the same state in the same process:
radius_counts_f64(b) — one N^2 pass with the same loads and the same five-operation d2, a count where the tree's pass has a (value,
index) select; b as tools/groups_f64_measure.py's — and mst_f64().  Two warm-up rounds, then --rounds timed ones (at N > 262144 a third
of them, at least two: a tree is a dozen N^2 passes).  wall = a host clock round the call, which ends in a synchronise and the copy of
the results.  device = nbody_kernel_time's event pairs round the N^2 passes (pass and fold); for mst_f64 that is the sum over its
rounds, and the O(N) kernels, the 4-byte read-backs and the host's sort show only in the wall time.  The library's own host clock
(NBODY_MST_PHASES=1) splits the call into the rounds, the read-back of the edges and the sort.  The measuring runs in a process of its
own under a time limit; if it ends with any status but 0 or runs out of time, nothing more is started on the device.  There is no CPU
path: without a device the run fails."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(nb, n, rounds):
    import numpy as np
    p32, v32 = nb.ic_plummer(n, seed=1)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    F = nb._lib.KERNEL_FORCES
    if n > 262144:
        rounds = max(2, rounds // 3)
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm, vel)
        r_half = float(e.lagrange_f64((0.5,)).radius[0])
        b = 0.2 * (4.0 * np.pi * r_half ** 3 / 3.0 / (n / 2.0)) ** (1.0 / 3.0)
        calls = (("radius_counts_f64", lambda: e.radius_counts_f64(b)), ("mst_f64", e.mst_f64))
        wall = {name: [] for name, _ in calls}
        dev = {name: [] for name, _ in calls}
        summary = None
        for k in range(rounds + 2):
            for name, call in calls:
                e.synchronize()
                f0 = e.kernel_time(F)
                t0 = time.perf_counter()
                got = call()
                w = (time.perf_counter() - t0) * 1e3
                f1 = e.kernel_time(F)
                if name == "mst_f64":
                    summary = got.summary
                    assert f1[1] - f0[1] == summary.rounds, (f1[1] - f0[1], summary)
                else:
                    assert f1[1] - f0[1] == 1, (name, f1[1] - f0[1])
                if k >= 2:
                    wall[name].append(w)
                    dev[name].append(f1[0] - f0[0])
        _, cus = e.kernel_clock()
    med = statistics.median
    print(f"# N = {n}, r_half = {r_half:.6g}, b = {b:.6g}, {rounds} rounds behind 2 warm-up rounds; {cus} compute units")
    print(f"# tree: edges {summary.edges}, components {summary.components}, length {summary.length:.6g}, longest edge "
          f"{summary.longest_d2 ** 0.5:.6g}, rounds {summary.rounds}")
    for name, _ in calls:
        d, w = dev[name], wall[name]
        print(f"{name:20s} device {med(d):10.3f} ms (min {min(d):10.3f}, max {max(d):10.3f})  wall {med(w):10.3f} ms (min {min(w):10.3f}, max {max(w):10.3f})")
    per_pass = med(dev["mst_f64"]) / summary.rounds
    print(f"mst_f64 per pass: device {per_pass:.3f} ms over {summary.rounds} rounds;  / radius_counts_f64 device {per_pass / med(dev['radius_counts_f64']):.3f}")
    print(f"mst_f64 wall - device passes: {med(wall['mst_f64']) - med(dev['mst_f64']):.3f} ms (the O(N) kernels, the read-backs, the sort, the copies out)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 1 << 20], help="one measuring process per size, in this order")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="internal: measure the first --n in this process")
    ap.add_argument("--limit", type=int, default=400, help="seconds a measuring process may take")
    args = ap.parse_args()
    if args.child:
        import parallelnbody_amd as nb
        if nb.device_count() < 1:
            raise SystemExit("mst_f64_measure: needs a HIP device")
        measure(nb, args.n[0], args.rounds)
        return 0
    lines = [f"# python tools/mst_f64_measure.py --n {' '.join(str(n) for n in args.n)} --rounds {args.rounds} on one GPU, one context and one process per N",
             "# fp64 state, Plummer sphere; radius_counts_f64 at b = 0.2 x the mean interparticle distance inside the half-mass radius",
             "# device = event pairs round the N^2 passes (nbody_kernel_time); wall = host clock round the call incl. synchronise and the copy of the results"]
    failed = 0
    for n in args.n:
        cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--rounds", str(args.rounds), "--child"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=dict(os.environ, NBODY_MST_PHASES="1"))
            lines += r.stdout.splitlines()
            phases = [[float(x) for x in m.groups()] for m in re.finditer(r"mst_f64 phases: n \d+ rounds \d+ loop (\S+) readback (\S+) sort (\S+) ms", r.stderr)]
            if r.returncode != 0 or not r.stdout.strip():
                failed = 1
                err = [ln for ln in r.stderr.strip().splitlines() if not ln.startswith("mst_f64 phases")]
                lines.append(f"# the measuring process ended with status {r.returncode}: {err[-1] if err else 'no output'}")
            elif len(phases) > 2:
                loop, back, sort = (statistics.median(col) for col in zip(*phases[2:]))      # behind the two warm-up calls
                lines.append(f"mst_f64 host clock: rounds {loop:.3f} ms, components + read-back of the edges {back:.3f} ms, sort {sort:.3f} ms "
                             f"({100.0 * sort / (loop + back + sort):.2f} % of the three)")
        except subprocess.TimeoutExpired:
            failed = 1
            lines.append(f"# the measuring process did not finish in {args.limit} s")
        if failed:
            break                                                  # nothing more is started on the device
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return failed


if __name__ == "__main__":
    sys.exit(main())
