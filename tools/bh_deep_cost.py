"""What a deep context (nbody_set_bh_max_depth) costs, against a default one, at theta = 1.0 (OctreeSearch.cpp:85).
    python3 tools/bh_deep_cost.py [N ...]          (default: 2000 65536 1048576)
  ordinary frames  step(0.01, K) on scenes with no body below level 42 (box scene up to 16384 bodies, Plummer sphere above; and the
                   box scene with a runaway body that holds Size at 1e9): wall time per frame at limit 42 and at limit 200, best of 5
  deep frames      the same runaway scene with a pair 1e-4 apart at |x| ~ 500 (a tree of ~50 levels): one frame at limit 200 — the
                   attempt handed back, the cold sort, the deep build, the walk — against one frame of the scene without the pair,
                   force passes (compute_forces: the bodies stay where they are, so every pass is a deep frame), best of 9
N <= 4096 goes through the larger systems' sort and build in a deep frame; the ordinary frame there is the one-workgroup build."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import parallelnbody_amd as nb


def scene(n, kind):
    if kind == "plummer":
        return nb.ic_plummer(n, seed=1)
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=1)
    if kind in ("runaway", "deep"):
        posm[0, :3] = (1.0e9, -2.0e8, 3.0e8); posm[0, 3] = np.float32(1e-6)
        posm[1, :3] = (500.25, 300.5, -200.75); vel[:3, :3] = 0.0
        posm[2, :3] = posm[1, :3] + np.float32(1e-4 if kind == "deep" else 5.0)
    return posm, vel


def frames_us(n, kind, limit, k):
    posm, vel = scene(n, kind)
    best = 1e30
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_bh_max_depth(limit)
        for _ in range(5):
            e.set_state(posm, vel)
            e.step(0.01, 2); e.synchronize()
            t0 = time.perf_counter()
            e.step(0.01, k); e.synchronize()
            best = min(best, (time.perf_counter() - t0) / k)
    return best * 1e6


def pass_us(n, kind, limit):
    posm, vel = scene(n, kind)
    best = 1e30
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_bh_max_depth(limit)
        e.set_state(posm, vel)
        e.compute_forces(); e.synchronize()
        for _ in range(9):
            t0 = time.perf_counter()
            e.compute_forces(); e.synchronize()
            best = min(best, time.perf_counter() - t0)
        levels = e.bh_stats()["levels"]
    return best * 1e6, levels


sizes = [int(a) for a in sys.argv[1:]] or [2000, 65536, 1 << 20]
for n in sizes:
    k = 200 if n <= 16384 else (100 if n <= 262144 else 50)
    for kind in (("box" if n <= 16384 else "plummer"), "runaway"):
        a, b = frames_us(n, kind, 42, k), frames_us(n, kind, 200, k)
        print(f"N={n:8d} {kind:8s} ordinary frames: limit 42 {a:9.1f} us  limit 200 {b:9.1f} us  ({b - a:+.1f} us)", flush=True)
    base, lb = pass_us(n, "runaway", 200)
    deep, ld = pass_us(n, "deep", 200)
    print(f"N={n:8d} force pass at limit 200: runaway scene {base:9.1f} us ({lb} levels), with the deep pair {deep:9.1f} us "
          f"({ld} levels): a deep frame costs {deep - base:+.1f} us", flush=True)
