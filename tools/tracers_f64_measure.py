#!/usr/bin/env python3
"""Device time of the fp64 point passes and of Hermite steps that carry fp64 tracers, on one GPU.

    python tools/tracers_f64_measure.py [--n 65536] [--out profiles/tracers_f64_measure.txt]

Every part runs in a process of its own under its own time limit.  Behind a part that ends with any status but 0, prints nothing or runs
out of time NOTHING MORE IS STARTED on the device (a fault comes back from the library as an error code, so the part's status is 1): the
run ends there with what it has and status 1.
       points M   one point jerk pass (nbody_jerk_at_f64) and one point snap pass (the tracers' pass of nbody_hermite6_step: the forces
                  time of a step with M tracers less that of a step without) at N bodies, beside the bodies' own jerk and snap passes of
                  the same context (m = N): pairs per second and the ratio to the body pass's
       steps      a whole nbody_hermite_step and nbody_hermite6_step at N bodies without tracers, with M = N tracers, and on a context that
                  holds the tracers as N more bodies of mass 0
Times are nbody_kernel_time's event pairs (device) and a host clock round the call and a synchronise (wall); medians of --reps runs
behind one warm-up.  There is no CPU path: without a device the parts fail."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 1e-7                                                          # a step that leaves the scene what it is


def scene(nb, n, m, seed=1):
    import numpy as np
    p32, v32 = nb.ic_plummer(n, seed=seed)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    tpos = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
    tvel = rng.normal(0.0, float(np.abs(vel[:, :3]).std()), (m, 3))
    return posm, vel, tpos, tvel


def timed(nb, e, call, reps):
    """(wall ms, forces ms, update ms, forces passes) of call(): medians over reps behind one warm-up."""
    F, U = nb._lib.KERNEL_FORCES, nb._lib.KERNEL_UPDATE
    rows = []
    for k in range(reps + 1):
        e.synchronize()
        f0, u0 = e.kernel_time(F), e.kernel_time(U)
        t0 = time.perf_counter()
        call()
        e.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        f1, u1 = e.kernel_time(F), e.kernel_time(U)
        if k:
            rows.append((wall, f1[0] - f0[0], u1[0] - u0[0], f1[1] - f0[1]))
    return tuple(statistics.median(r[c] for r in rows) for c in range(4))


def part_points(nb, n, m, reps):
    import numpy as np
    posm, vel, tpos, tvel = scene(nb, n, m)
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm, vel)
        _, body_jerk, _, _ = timed(nb, e, lambda: e.jerk(np.float64), reps)
        _, point_jerk, _, k = timed(nb, e, lambda: e.jerk_at_f64(tpos, tvel), reps)
        assert k == 1
        e.hermite6_step(DT, 1)
        _, body_snap, _, k = timed(nb, e, lambda: e.hermite6_step(DT, 1), reps)
        assert k == 1
        e.set_tracers_f64(tpos, tvel)
        e.hermite6_step(DT, 1)
        _, both_snap, _, k = timed(nb, e, lambda: e.hermite6_step(DT, 1), reps)
        assert k == 2
        point_snap = both_snap - body_snap
    bj, bs = n * n / (body_jerk * 1e-3), n * n / (body_snap * 1e-3)
    pj, ps = m * n / (point_jerk * 1e-3), m * n / (point_snap * 1e-3)
    print(f"N={n:6d} M={m:8d} jerk  point pass {point_jerk:10.4f} ms  {pj:.3e} pairs/s   body pass (m = N) {body_jerk:9.4f} ms  {bj:.3e} pairs/s   "
          f"ratio {pj / bj:5.3f}")
    print(f"N={n:6d} M={m:8d} snap  point pass {point_snap:10.4f} ms  {ps:.3e} pairs/s   body pass (m = N) {body_snap:9.4f} ms  {bs:.3e} pairs/s   "
          f"ratio {ps / bs:5.3f}")


def part_steps(nb, n, reps):
    import numpy as np
    m = n
    posm, vel, tpos, tvel = scene(nb, n, m)
    tp = np.zeros((m, 4)); tv = np.zeros((m, 4))
    tp[:, :3] = tpos; tv[:, :3] = tvel
    rows = {}
    for order in (4, 6):
        step = (lambda x: x.hermite_step(DT, 1)) if order == 4 else (lambda x: x.hermite6_step(DT, 1))
        with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
            e.set_state(posm, vel)
            step(e)
            rows[order, "bodies alone"] = timed(nb, e, lambda: step(e), reps)
            e.set_tracers_f64(tpos, tvel)
            step(e)
            rows[order, "with tracers"] = timed(nb, e, lambda: step(e), reps)
        with nb.NBodyEngine(n + m, precision="f64", time_kernels=True) as e:
            e.set_state(np.concatenate([posm, tp]), np.concatenate([vel, tv]))
            step(e)
            rows[order, "as massless bodies"] = timed(nb, e, lambda: step(e), reps)
        for how in ("bodies alone", "with tracers", "as massless bodies"):
            wall, f, u, k = rows[order, how]
            print(f"N={n:6d} M={m:6d} order {order} step {how:19s} wall {wall:9.3f} ms  device {f + u:9.3f} ms = forces {f:9.3f} ({int(k)} passes) + update {u:7.3f}")
        alone, carry, app = (rows[order, h][1] + rows[order, h][2] for h in ("bodies alone", "with tracers", "as massless bodies"))
        print(f"N={n:6d} M={m:6d} order {order}: carrying the tracers costs {carry - alone:.3f} ms a step ({carry / alone:.2f} x the bodies' step); "
              f"appending them as massless bodies {app - alone:.3f} ms ({app / alone:.2f} x): {(app - alone) / (carry - alone):.2f} x the tracers' cost")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default=None, help="internal: run one part in this process (points:M or steps)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    args = ap.parse_args()
    if args.part:
        import parallelnbody_amd as nb
        if nb.device_count() < 1:
            raise SystemExit("tracers_f64_measure: needs a HIP device")
        if args.part.startswith("points:"):
            part_points(nb, args.n, int(args.part.split(":")[1]), args.reps)
        else:
            part_steps(nb, args.n, args.reps)
        return 0
    lines = [f"# python tools/tracers_f64_measure.py --n {args.n} on one GPU, one session; every part a process of its own",
             "# fp64 state, eps = 0, Plummer sphere, random moving points inside it; device = nbody_kernel_time (event pairs), wall = host clock incl. "
             f"synchronise; medians of {args.reps} behind a warm-up",
             "# pairs/s of a point pass = M N / its device time; the yardstick is the body pass of the same context, N N / its device time"]
    failed = 0
    for part in ("points:1024", f"points:{args.n}", "points:1048576", "steps"):
        cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--reps", str(args.reps), "--part", part]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            lines += r.stdout.splitlines()
            if r.returncode != 0 or not r.stdout.strip():
                failed += 1
                lines.append(f"# part {part} ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else 'no output'}")
                lines.append("# nothing more is started on the device")
                break
        except subprocess.TimeoutExpired:
            failed += 1
            lines += [f"# part {part} did not finish in {args.limit} s: nothing more is started on the device"]
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
