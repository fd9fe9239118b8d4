"""What carrying fp64 tracers in a Hermite block session costs against the way there was before (raw output:
profiles/block_tracers_measure.txt).

    python tools/block_tracers_measure.py [--out FILE] [--sizes 16384,65536] [--orders 4,6]

Scene: tools/hermite_block_measure.py's — ic_plummer(N) in fp64 with bodies 0 and 1 a binary of period 0.0125, eps = 0, dt_max = 0.01,
12 levels, eta = 0.02 (fourth order) / 0.5 (sixth) — and M tracers drawn inside the sphere (normal, the bodies' own spread in position
and velocity), M = 1024 and M = N.  One frame of dt_max from begin's own start rule, two ways:
  carried    nbody_hermite[6]_block_begin_tracers on N bodies with M tracers: (m_b + m_t) N pairs a block step
  appended   the YARDSTICK, which needs nothing of this feature: the tracers as M bodies of mass 0 behind the bodies, through
             nbody_hermite[6]_block_begin on N + M bodies: (m_b + m_t) (N + M) pairs a block step, the same schedule
Every (order, N, M, way) runs in a process of its own: a warm-up frame, then five frames, each from the same uploaded state (the start's
evaluation is outside the window); the medians of
  wall       host clock around nbody_hermite[6]_block_advance(1) and a synchronise, on a context WITHOUT time_kernels
  device     nbody_kernel_time on a second context WITH time_kernels: forces and update apart
and the frame's block steps, pairs and — carried — the steps in which no body was due."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DT_MAX, LEVELS = 0.01, 12
ETAS = {4: 0.02, 6: 0.5}
REPS = 5


def tracers(p, v, m):
    rng = np.random.default_rng(9000 + m)
    return (rng.normal(0.0, float(np.abs(p[:, :3]).std()), (m, 3)), rng.normal(0.0, float(np.abs(v[:, :3]).std()), (m, 3)))


def frame_part(order, n, m, way):
    import parallelnbody_amd as nb
    from parallelnbody_amd import _lib
    from hermite_block_measure import scene
    F, U = _lib.KERNEL_FORCES, _lib.KERNEL_UPDATE
    p, v, _ = scene(nb, n)
    tp, tv = tracers(p, v, m)
    prefix = "hermite" if order == 4 else "hermite6"
    if way == "appended":
        pad = np.zeros((m, 1))
        p, v = np.concatenate([p, np.hstack([tp, pad])]), np.concatenate([v, np.hstack([tv, pad])])
    res = {"order": order, "n": n, "m": m, "way": way}
    for timed in (False, True):
        with nb.NBodyEngine(len(p), precision="f64", time_kernels=timed) as e:
            got = []
            for rep in range(REPS + 1):                            # (the first one warms up)
                e.set_state(p, v)
                if way == "carried":
                    e.set_tracers_f64(tp, tv)
                    getattr(e, prefix + "_block_begin_tracers")(DT_MAX, LEVELS, eta=ETAS[order])
                else:
                    getattr(e, prefix + "_block_begin")(DT_MAX, LEVELS, eta=ETAS[order])
                e.synchronize()
                if timed:
                    e.kernel_time_reset()
                t0 = time.perf_counter()
                st = getattr(e, prefix + "_block_advance")(1)
                e.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                got.append((e.kernel_time(F)[0], e.kernel_time(U)[0]) if timed else (wall,))
            med = [statistics.median(c) for c in zip(*got[1:])]
            if timed:
                res["forces_ms"], res["update_ms"] = med
            else:
                res.update(wall_ms=med[0], steps=st["block_steps"], pairs=st["pairs"], only=0)
                if way == "carried":
                    ts = getattr(e, prefix + "_block_tracers_state")()[2]
                    res.update(pairs=st["pairs"] + ts["pairs"], only=ts["tracer_only_steps"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_tracers_measure.txt"))
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--orders", default="4,6")
    ap.add_argument("--ways", default="carried,appended", help="appended alone runs on a build without the feature")
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--part", help="(internal) run one part in this process and print its result as JSON")
    a = ap.parse_args()
    if a.part:
        order, n, m, way = a.part.split(":")
        print("RESULT " + json.dumps(frame_part(int(order), int(n), int(m), way)), flush=True)
        return 0
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    def part(spec):
        """The part in a fresh process under the time limit; None ends the run."""
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", spec], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say(f"# part {spec}: no result within {a.limit} s; the run ends here")
            return None
        lines = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            say(f"# part {spec}: exit status {r.returncode}; the run ends here\n# " + r.stderr.strip().replace("\n", "\n# ")[-2000:])
            return None
        return json.loads(lines[-1][7:])

    say("# python tools/block_tracers_measure.py on one MI355X, one session; every part a process of its own")
    say(f"# fp64 state, eps = 0, Plummer sphere + one binary of period 0.0125, dt_max = {DT_MAX}, {LEVELS} levels, eta = {ETAS[4]} / {ETAS[6]}")
    say(f"# one frame of dt_max from begin's start rule: medians of {REPS} behind a warm-up; wall incl. synchronise (no time_kernels),")
    say("# device = nbody_kernel_time forces + update; per step = device / block steps")
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            for m in (1024, n):
                got = {}
                for way in a.ways.split(","):
                    r = part(f"{order}:{n}:{m}:{way}")
                    if r is None:
                        return 1
                    got[way] = r
                    dev = r["forces_ms"] + r["update_ms"]
                    say(f"order {order} N={n:6d} M={m:6d} {way:8s} wall {r['wall_ms']:9.3f} ms  device {dev:9.3f} ms = forces {r['forces_ms']:9.3f} + "
                        f"update {r['update_ms']:8.3f}  block steps {r['steps']:5d} (tracer-only {r['only']:4d})  pairs {r['pairs']:.4e}  "
                        f"per step: wall {1e3 * r['wall_ms'] / r['steps']:7.1f} us, device {1e3 * dev / r['steps']:7.1f} us")
                if len(got) == 2:
                    c, y = got["carried"], got["appended"]
                    say(f"      carried / appended: wall {c['wall_ms'] / y['wall_ms']:.3f}, device "
                        f"{(c['forces_ms'] + c['update_ms']) / (y['forces_ms'] + y['update_ms']):.3f}, pairs {c['pairs'] / y['pairs']:.3f}, "
                        f"block steps {c['steps']} / {y['steps']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
