#!/usr/bin/env python3
"""Device time of the fp64 neighbour census — neighbours_f64(k) for k = 1, 6 and 8 — beside the nearest pass of the pair census and the
fp64 potential pass, on one GPU.

    python tools/neighbours_f64_measure.py [--n 65536] [--rounds 10] [--out profiles/neighbours_f64_measure.txt]

One context holds N bodies (fp64 state, a Plummer sphere); a round runs neighbours_f64(1), neighbours_f64(6), neighbours_f64(8),
density_f64(6), core_f64(6), nearest_f64() and potentials_f64() — the last two are the yardsticks: the nearest pass is the kernel the
neighbour pass is a sibling of (one minimum where this keeps a sorted list), the potential pass the tile loop both descend from — one
after the other, alternating, so that all see the same clock and the same neighbours on the host; two warm-up rounds, then --rounds
timed ones.  Times are nbody_kernel_time's event pairs round the pass (device: the tile kernel and its fold, every slab of them; the
core's reductions are not part of the pass) and a host clock round the call, which ends in a synchronise (wall: with the copy of the
results — and, for core_f64, the reductions and mass_within); median, smallest and largest of the rounds.  The measuring runs in a
process of its own under a time limit; if it ends with any status but 0 or runs out of time, nothing more is started on the device.
There is no CPU path: without a device the run fails."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEAR, POT = "nearest_f64", "potentials_f64"
JERK_MS = 4.7                                                      # the fp64 jerk pass at N = 65536 (profiles/census_f64_measure.txt)


def measure(nb, n, rounds):
    import numpy as np
    p32, v32 = nb.ic_plummer(n, seed=1)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    F = nb._lib.KERNEL_FORCES
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm, vel)
        calls = (("neighbours_f64(1)", lambda: e.neighbours_f64(1)), ("neighbours_f64(6)", lambda: e.neighbours_f64(6)),
                 ("neighbours_f64(8)", lambda: e.neighbours_f64(8)), ("density_f64(6)", lambda: e.density_f64(6)),
                 ("core_f64(6)", lambda: e.core_f64(6)), (NEAR, e.nearest_f64), (POT, e.potentials_f64))
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
        _, cus = e.kernel_clock()
    print(f"# N = {n}, eps = 0, {rounds} rounds behind 2 warm-up rounds; {cus} compute units")
    med = {}
    for name, _ in calls:
        dev = [r[0] for r in rows[name]]; wall = [r[1] for r in rows[name]]
        med[name] = statistics.median(dev)
        print(f"{name:20s} device {med[name]:9.3f} ms (min {min(dev):9.3f}, max {max(dev):9.3f})  {n * n / (med[name] * 1e-3):.3e} pairs/s   "
              f"wall {statistics.median(wall):9.3f} ms")
    for k in (1, 6, 8):
        t = med[f"neighbours_f64({k})"]
        print(f"neighbours_f64({k}) / nearest_f64 {t / med[NEAR]:6.3f};  / potentials_f64 {t / med[POT]:6.3f};  / the jerk pass's {JERK_MS} ms "
              f"{t / JERK_MS:6.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="internal: measure in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring process may take")
    args = ap.parse_args()
    if args.child:
        import parallelnbody_amd as nb
        if nb.device_count() < 1:
            raise SystemExit("neighbours_f64_measure: needs a HIP device")
        measure(nb, args.n, args.rounds)
        return 0
    lines = [f"# python tools/neighbours_f64_measure.py --n {args.n} --rounds {args.rounds} on one GPU, one context, one process",
             "# fp64 state, Plummer sphere; device = nbody_kernel_time (event pairs round the pass), wall = host clock round the call incl. synchronise "
             "and the copy of the results", "# pairs/s = N N / the median device time; the yardsticks are the nearest pass and the fp64 potential pass of the same context"]
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--rounds", str(args.rounds), "--child"]
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
