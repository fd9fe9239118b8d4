#!/usr/bin/env python3
"""Device time of the fp64 pair census — the nearest pass and the partner pass — beside the fp64 potential and jerk passes, on one GPU.

    python tools/census_f64_measure.py [--n 65536] [--rounds 10] [--out profiles/census_f64_measure.txt]

One context holds N bodies (fp64 state, a Plummer sphere); a round runs nearest_f64(), partners_f64(), potentials_f64() and
jerk(np.float64) — the two yardsticks: nbody_get_potentials_f64 for the nearest pass, which does less per pair (no root),
nbody_get_jerk_f64 for the partner pass, which has its LDS and one root — one after the other, so that the four see the same clock and
the same neighbours on the host; two warm-up rounds, then --rounds timed ones.  Times are nbody_kernel_time's event pairs round the
pass (device: the tile kernel and its fold) and a host clock round the call, which ends in a synchronise (wall: with the copy of the
results); median, smallest and largest of the rounds.  The measuring runs in a process of its own under a time limit; if it ends with
any status but 0 or runs out of time, nothing more is started on the device.  There is no CPU path: without a device the run fails."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POT, JERK = "potentials_f64", "jerk (get_jerk_f64)"


def measure(nb, n, rounds, eps):
    import numpy as np
    p32, v32 = nb.ic_plummer(n, seed=1)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    F = nb._lib.KERNEL_FORCES
    with nb.NBodyEngine(n, precision="f64", eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        calls = (("nearest_f64", e.nearest_f64), ("partners_f64", e.partners_f64), (POT, e.potentials_f64), (JERK, lambda: e.jerk(np.float64)))
        rows = {name: [] for name, _ in calls}
        for k in range(rounds + 2):
            for name, call in calls:
                e.synchronize()
                f0 = e.kernel_time(F)
                t0 = time.perf_counter()
                call()
                wall = (time.perf_counter() - t0) * 1e3
                f1 = e.kernel_time(F)
                assert f1[1] - f0[1] == 1, (name, f1[1] - f0[1])   # one pass under NBODY_KERNEL_FORCES
                if k >= 2:
                    rows[name].append((f1[0] - f0[0], wall))
        mhz, cus = e.kernel_clock()
    print(f"# N = {n}, eps = {eps}, {rounds} rounds behind 2 warm-up rounds; {cus} compute units; shader clock of the instrumented force kernels: "
          f"{mhz:.0f} MHz" + (" (none of these passes is instrumented: not measured)" if mhz == 0.0 else ""))
    med = {}
    for name, _ in calls:
        dev = [r[0] for r in rows[name]]; wall = [r[1] for r in rows[name]]
        med[name] = statistics.median(dev)
        print(f"{name:22s} device {med[name]:9.3f} ms (min {min(dev):9.3f}, max {max(dev):9.3f})  {n * n / (med[name] * 1e-3):.3e} pairs/s   "
              f"wall {statistics.median(wall):9.3f} ms")
    print(f"nearest_f64 / potentials_f64 {med['nearest_f64'] / med[POT]:5.3f} (expected <= 1);  partners_f64 / jerk {med['partners_f64'] / med[JERK]:5.3f} "
          f"(expected <= 1)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="internal: measure in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring process may take")
    args = ap.parse_args()
    if args.child:
        import parallelnbody_amd as nb
        if nb.device_count() < 1:
            raise SystemExit("census_f64_measure: needs a HIP device")
        measure(nb, args.n, args.rounds, args.eps)
        return 0
    lines = [f"# python tools/census_f64_measure.py --n {args.n} --rounds {args.rounds} on one GPU, one context, one process",
             "# fp64 state, Plummer sphere; device = nbody_kernel_time (event pairs round the pass), wall = host clock round the call incl. synchronise "
             "and the copy of the results", "# pairs/s = N N / the median device time; the yardsticks are the fp64 potential and jerk passes of the same context"]
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--rounds", str(args.rounds), "--eps", str(args.eps), "--child"]
    failed = 0
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        lines += r.stdout.splitlines()
        if r.returncode != 0 or not r.stdout.strip():
            failed = 1
            lines.append(f"# the measuring process ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else 'no output'}")
    except subprocess.TimeoutExpired:
        failed = 1
        lines.append(f"# the measuring process did not finish in {args.limit} s")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return failed


if __name__ == "__main__":
    sys.exit(main())
