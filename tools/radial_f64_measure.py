#!/usr/bin/env python3
"""Device and wall time of the fp64 radial census — radial_order_f64() and lagrange_f64() — beside what it replaces, on one GPU.

    python tools/radial_f64_measure.py [--n 65536 1048576] [--rounds 10] [--out profiles/radial_f64_measure.txt]

One context holds N bodies (fp64 state, a Plummer sphere); the centre is core_f64(6)'s.  A round runs, one after the other on the same
state: radial_order_f64(centre), lagrange_f64(nine fractions, centre), mass_within at one radius and at 64 radii (the unit cost of the
bisection the census replaces: about 50 such passes per radius), core_f64(6), and the host route — state(np.float64), d2, np.argsort(kind=
"stable") and np.cumsum in numpy.  Two warm-up rounds, then --rounds timed ones.  wall = a host clock round the call, which ends in a
synchronise and the copy of the results.  device = event pairs: for core_f64 nbody_kernel_time's round its pass; for the census the
library's own event pairs round its four phases — keys (the key kernel and its memset), sort (the histogram fold and the eight radix
passes), scan (three launches), select (two) — which it records and prints under NBODY_RADIAL_PHASES=1; those rounds are separate from
the wall rounds, since they wait once more.  mass_within and the host route have no device timer: wall only.  The measuring runs in a
process of its own under a time limit; if it ends with any status but 0 or runs out of time, nothing more is started on the device.
There is no CPU path: without a device the run fails."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9)
PHASES = ("keys", "sort", "scan", "select")


def phased(call, rounds):
    """[{phase: ms}] of `rounds` calls under NBODY_RADIAL_PHASES=1, read from what the library prints to stderr"""
    sys.stderr.flush()
    keep = os.dup(2)
    rows = []
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["NBODY_RADIAL_PHASES"] = "1"
        try:
            for _ in range(rounds + 2):
                call()
        finally:
            del os.environ["NBODY_RADIAL_PHASES"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        for ln in tmp.read().decode().splitlines():
            m = re.match(r"radial_f64 phases: n \d+ k \d+ keys (\S+) sort (\S+) scan (\S+) select (\S+) ms", ln)
            if m:
                rows.append(dict(zip(PHASES, (float(x) for x in m.groups()))))
    assert len(rows) == rounds + 2, len(rows)
    return rows[2:]


def measure(nb, n, rounds):
    import numpy as np
    p32, v32 = nb.ic_plummer(n, seed=1)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    F = nb._lib.KERNEL_FORCES
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm, vel)
        centre = e.core_f64(6).centre
        r_half = float(e.lagrange_f64((0.5,), centre).radius[0])
        r64 = np.linspace(0.1, 2.0, 64) * r_half

        def host_route():
            p, _, _ = e.state(np.float64)
            d = p[:, :3] - centre
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            order = np.argsort(d2, kind="stable")
            return order, np.cumsum(p[order, 3])

        calls = (("radial_order_f64", lambda: e.radial_order_f64(centre)), ("lagrange_f64(9)", lambda: e.lagrange_f64(FRACTIONS, centre)),
                 ("mass_within(1)", lambda: e.mass_within(centre, [r_half])), ("mass_within(64)", lambda: e.mass_within(centre, r64)),
                 ("core_f64(6)", lambda: e.core_f64(6)), ("host argsort route", host_route))
        wall = {name: [] for name, _ in calls}
        core_dev = []
        for k in range(rounds + 2):
            for name, call in calls:
                e.synchronize()
                f0 = e.kernel_time(F)
                t0 = time.perf_counter()
                call()
                w = (time.perf_counter() - t0) * 1e3
                f1 = e.kernel_time(F)
                assert f1[1] - f0[1] == (1 if name == "core_f64(6)" else 0), (name, f1[1] - f0[1])   # the census is no pass
                if k >= 2:
                    wall[name].append(w)
                    if name == "core_f64(6)":
                        core_dev.append(f1[0] - f0[0])
        phases = {"radial_order_f64": phased(calls[0][1], rounds), "lagrange_f64(9)": phased(calls[1][1], rounds)}
        _, cus = e.kernel_clock()
    print(f"# N = {n}, eps = 0, {rounds} rounds behind 2 warm-up rounds; {cus} compute units")
    med = statistics.median
    for name, _ in calls:
        w = wall[name]
        dev = ""
        if name in phases:
            tot = [sum(r.values()) for r in phases[name]]
            dev = f"device {med(tot):9.3f} ms (min {min(tot):9.3f}, max {max(tot):9.3f})  "
        elif name == "core_f64(6)":
            dev = f"device {med(core_dev):9.3f} ms (min {min(core_dev):9.3f}, max {max(core_dev):9.3f})  "
        print(f"{name:20s} {dev:56s}wall {med(w):9.3f} ms (min {min(w):9.3f}, max {max(w):9.3f})")
    for name, rows in phases.items():
        print(f"{name:20s} device by phase: " + "  ".join(f"{p} {med([r[p] for r in rows]):.3f}" for p in PHASES) + " ms")
    w = {name: med(v) for name, v in wall.items()}
    print(f"radial_order_f64 wall / host argsort route {w['radial_order_f64'] / w['host argsort route']:.4f};  "
          f"lagrange_f64(9) wall / 50 x mass_within(1) {w['lagrange_f64(9)'] / (50.0 * w['mass_within(1)']):.4f};  "
          f"/ core_f64(6) {w['lagrange_f64(9)'] / w['core_f64(6)']:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 1 << 20], help="one measuring process per size, in this order")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="internal: measure the first --n in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds a measuring process may take")
    args = ap.parse_args()
    if args.child:
        import parallelnbody_amd as nb
        if nb.device_count() < 1:
            raise SystemExit("radial_f64_measure: needs a HIP device")
        measure(nb, args.n[0], args.rounds)
        return 0
    lines = [f"# python tools/radial_f64_measure.py --n {' '.join(str(n) for n in args.n)} --rounds {args.rounds} on one GPU, one context and one process per N",
             "# fp64 state, Plummer sphere, centre = core_f64(6)'s; wall = host clock round the call incl. synchronise and the copy of the results",
             "# device = event pairs: the census's four phases (NBODY_RADIAL_PHASES=1, rounds of their own), core_f64's pass (nbody_kernel_time)"]
    failed = 0
    for n in args.n:
        cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--rounds", str(args.rounds), "--child"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            lines += r.stdout.splitlines()
            if r.returncode != 0 or not r.stdout.strip():
                failed = 1
                lines.append(f"# the measuring process ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else 'no output'}")
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
