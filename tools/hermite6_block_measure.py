"""What sixth-order Hermite block time steps cost and buy on the device (raw output: profiles/hermite6_block_measure.txt).

    python tools/hermite6_block_measure.py [--out FILE] [--sizes 4096,16384,65536] [--table 65536] [--limit SECONDS]

Scene: tools/hermite_block_measure.py's — ic_plummer(N) in fp64 with bodies 0 and 1 a binary of eccentricity 0.5 and period 0.0125;
eps = 0, dt_max = 0.01, 12 levels.  Every part is a process of its own under a time limit of its own; a part that fails or runs out of
time ends the run (nothing more is started on the device).
  frame     one frame of dt_max, after one warm-up frame of the same kind from the same start, by
              block6   nbody_hermite6_block_advance(1) at eta = 0.5
              block4   nbody_hermite_block_advance(1) at eta = 0.02
              shared6  nbody_hermite6_advance(dt_max) at eta = 0.5
            each from a valid cache (the first evaluation is outside the window):
              wall    host clock around the call and a synchronise, on a context WITHOUT time_kernels
              device  nbody_kernel_time forces + update on a second context WITH time_kernels
            block steps (steps), mean active set, pairs, and the relative energy error of the frame (nbody_energy before and after).
            The comparison that matters is block6 against block4 AT COMPARABLE ENERGY ERROR: where the two errors differ by more than a
            factor of 10, one more block6 row follows with eta scaled by (error4 / error6)^(1/6), and says so.
  table     one block step against the size m of its active set (level_in puts the first m bodies at level 1 of 1), both orders: the
            median of five repetitions (each a fresh session: restart, begin, step) of the wall time and the device times."""
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
ETAS = {"block6": 0.5, "block4": 0.02, "shared6": 0.5}


def frame_part(n, scheme, eta):
    import parallelnbody_amd as nb
    from parallelnbody_amd import _lib
    from hermite_block_measure import scene
    F, U = _lib.KERNEL_FORCES, _lib.KERNEL_UPDATE
    p, v, _ = scene(nb, n)
    res = {"n": n, "scheme": scheme, "eta": eta}
    for timed in (False, True):
        with nb.NBodyEngine(n, precision="f64", time_kernels=timed) as e:
            for warm in (True, False):
                e.set_state(p, v)
                e0 = sum(e.energy())
                if scheme == "block6":
                    e.hermite6_block_begin(DT_MAX, LEVELS, eta=eta)
                elif scheme == "block4":
                    e.hermite_block_begin(DT_MAX, LEVELS, eta=eta)
                else:
                    e.hermite6_timescale()
                e.synchronize()
                if timed:
                    e.kernel_time_reset()
                t0 = time.perf_counter()
                if scheme == "shared6":
                    _, steps = e.hermite6_advance(DT_MAX, eta=eta, dt_max=DT_MAX)
                    st = {"block_steps": steps, "body_steps": steps * n, "pairs": steps * n * n, "level_max": 0, "floor_hits": 0}
                else:
                    st = (e.hermite6_block_advance if scheme == "block6" else e.hermite_block_advance)(1)
                e.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                if warm:
                    continue
                if timed:
                    res["forces_ms"], res["update_ms"] = e.kernel_time(F)[0], e.kernel_time(U)[0]
                else:
                    res.update(wall_ms=wall, steps=st["block_steps"], mean_m=st["body_steps"] / st["block_steps"], pairs=st["pairs"],
                               level_max=st["level_max"], floor_hits=st["floor_hits"], err=abs(sum(e.energy()) - e0) / abs(e0))
    return res


def table_part(n, m, order):
    import parallelnbody_amd as nb
    from parallelnbody_amd import _lib
    from hermite_block_measure import scene
    F, U = _lib.KERNEL_FORCES, _lib.KERNEL_UPDATE
    p, v, _ = scene(nb, n)
    level_in = np.zeros(n, np.int32)
    level_in[:m] = 1
    rows = {}
    for timed in (False, True):
        with nb.NBodyEngine(n, precision="f64", time_kernels=timed) as e:
            e.set_state(p, v)
            begin, advance = (e.hermite6_block_begin, e.hermite6_block_advance) if order == 6 else (e.hermite_block_begin, e.hermite_block_advance)
            got = []
            for rep in range(6):                                   # (the first one warms up)
                e.hermite_restart()
                begin(DT_MAX, 1, eta=ETAS["block6" if order == 6 else "block4"], level_in=level_in)
                e.synchronize()
                if timed:
                    e.kernel_time_reset()
                t0 = time.perf_counter()
                st = advance(1, max_block_steps=1)
                e.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                assert st["body_steps"] == m, (st, m)
                got.append((e.kernel_time(F)[0], e.kernel_time(U)[0]) if timed else (wall,))
            rows[timed] = [statistics.median(c) for c in zip(*got[1:])]
    return {"n": n, "m": m, "order": order, "wall_ms": rows[False][0], "forces_ms": rows[True][0], "update_ms": rows[True][1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hermite6_block_measure.txt"))
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--table", default="65536")
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--part", help="(internal) run one part in this process and print its result as JSON")
    a = ap.parse_args()
    if a.part:
        kind, *args = a.part.split(":")
        res = frame_part(int(args[0]), args[1], float(args[2])) if kind == "frame" else table_part(int(args[0]), int(args[1]), int(args[2]))
        print("RESULT " + json.dumps(res), flush=True)
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

    def frame_line(r, note=""):
        say(f"  frame {r['scheme']:7s} eta {r['eta']:<6.4g} wall {r['wall_ms']:10.3f} ms  device {r['forces_ms'] + r['update_ms']:10.3f} ms = forces "
            f"{r['forces_ms']:10.3f} + update {r['update_ms']:9.3f}  steps {r['steps']:6d}  mean m {r['mean_m']:9.1f}  pairs {r['pairs']:.3e}  "
            f"|dE/E| {r['err']:.2e}  deepest level {r['level_max']}  floor hits {r['floor_hits']}{note}")

    say("# python tools/hermite6_block_measure.py on one MI355X, one session; every part a process of its own")
    say(f"# fp64 state, eps = 0, Plummer sphere + one binary of period 0.0125, dt_max = {DT_MAX}, {LEVELS} levels")
    say("# frame: one warmed-up frame of dt_max; wall = host clock incl. synchronise (no time_kernels), device = nbody_kernel_time forces + update")
    for n in [int(x) for x in a.sizes.split(",")]:
        say(f"N={n:6d}")
        got = {}
        for scheme in ("block6", "block4", "shared6"):
            r = part(f"frame:{n}:{scheme}:{ETAS[scheme]}")
            if r is None:
                return 1
            got[scheme] = r
            frame_line(r)
        e6, e4 = got["block6"]["err"], got["block4"]["err"]
        if e6 > 0 and e4 > 0 and not (0.1 <= e6 / e4 <= 10.0):
            eta = min(1.5, max(0.05, ETAS["block6"] * (e4 / e6) ** (1.0 / 6.0)))
            r = part(f"frame:{n}:block6:{eta:.4g}")
            if r is None:
                return 1
            frame_line(r, f"  <- eta adjusted: |dE/E| of block6 at 0.5 and block4 at 0.02 differ by {e6 / e4:.3g}")
            got["block6"] = r
        b6, b4, s6 = got["block6"], got["block4"], got["shared6"]
        say(f"  block4 / block6 (eta {b6['eta']:.4g}): wall {b4['wall_ms'] / b6['wall_ms']:.2f}, device {(b4['forces_ms'] + b4['update_ms']) / (b6['forces_ms'] + b6['update_ms']):.2f}, "
            f"pairs {b4['pairs'] / b6['pairs']:.2f}, block steps {b4['steps'] / b6['steps']:.2f}, |dE/E| {b4['err'] / b6['err']:.3g};  "
            f"shared6 / block6: wall {s6['wall_ms'] / b6['wall_ms']:.2f}, pairs {s6['pairs'] / b6['pairs']:.1f}")
    say()
    say("# table: one block step against its active set's size m (median of 5; wall incl. the wait for 16 bytes and a synchronise)")
    for n in [int(x) for x in a.table.split(",") if x]:
        for m in [x for x in (1, 64, 512, 4096) if x < n] + [n]:
            for order in (6, 4):
                r = part(f"table:{n}:{m}:{order}")
                if r is None:
                    return 1
                lanes = 1 if m <= 1024 else 2
                say(f"N={n:6d} m={m:6d} order {order}  wall {r['wall_ms']:9.4f} ms  device forces {r['forces_ms']:9.4f} + update {r['update_ms']:8.4f} ms  "
                    f"{lanes} bod{'y' if lanes == 1 else 'ies'} per lane  pairs/s (device forces) {m * n / (r['forces_ms'] * 1e-3):.3e}")
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
