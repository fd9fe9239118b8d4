#!/usr/bin/env python3
"""Device and wall time of the fp64 group census — radius_counts_f64() and groups_f64() — beside a yardstick pass and a host route, on one
GPU.

    python tools/groups_f64_measure.py [--n 65536 1048576] [--rounds 10] [--out profiles/groups_f64_measure.txt]

One context holds N bodies (fp64 state, a Plummer sphere).  The linking length is b = 0.2 x the mean interparticle distance inside the
half-mass radius r_h (lagrange_f64 about the density centre): b = 0.2 (4 pi r_h^3 / 3 / (N / 2))^(1/3).  A round runs, one after the other
on the same state: nearest_f64() — the pair census's pass, the yardstick for one N^2 pass: three fp64 operations per pair where the new
pass does five —, radius_counts_f64(b), groups_f64(b).  Two warm-up rounds, then --rounds timed ones (at N > 262144 a third of them, at
least two: a groups call is several N^2 passes).  wall = a host clock round the call, which ends in a synchronise and the copy of the
results.  device = nbody_kernel_time's event pairs round the N^2 passes (pass and fold); for groups_f64 that is the sum over its rounds,
and the O(N) kernels and 4-byte read-backs between the passes show only in the wall time.  The host route, in wall time, once behind the
rounds: state(np.float64), then scipy's cKDTree.query_pairs and connected_components where scipy is importable, else the blockwise numpy
of tests/groups_f64_ref.py; the output says which.  The measuring runs in a process of its own under a time limit; if it ends with any
status but 0 or runs out of time, nothing more is started on the device.  There is no CPU path: without a device the run fails."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_route(e, b):
    """(what ran, groups, seconds): the labels on the host from a read-back of the state"""
    import numpy as np
    t0 = time.perf_counter()
    p, _, _ = e.state(np.float64)
    n = p.shape[0]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
        pairs = cKDTree(p[:, :3]).query_pairs(b, output_type="ndarray")
        graph = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
        groups, _ = connected_components(graph, directed=False)
        what = "scipy cKDTree.query_pairs + connected_components"
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import groups_f64_ref as R
        groups = R.groups(p, b)["summary"].groups
        what = "blockwise numpy + union-find (tests/groups_f64_ref.py)"
    return what, int(groups), time.perf_counter() - t0


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
        calls = (("nearest_f64", e.nearest_f64), ("radius_counts_f64", lambda: e.radius_counts_f64(b)), ("groups_f64", lambda: e.groups_f64(b)))
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
                if name == "groups_f64":
                    summary = got.summary
                    assert f1[1] - f0[1] == summary.rounds, (f1[1] - f0[1], summary)
                else:
                    assert f1[1] - f0[1] == 1, (name, f1[1] - f0[1])
                if k >= 2:
                    wall[name].append(w)
                    dev[name].append(f1[0] - f0[0])
        what, host_groups, host_s = host_route(e, b)
        _, cus = e.kernel_clock()
    print(f"# N = {n}, r_half = {r_half:.6g}, b = {b:.6g}, {rounds} rounds behind 2 warm-up rounds; {cus} compute units")
    print(f"# groups {summary.groups}, multiples {summary.multiples}, largest {summary.largest_members} bodies, links {summary.links}, "
          f"rounds {summary.rounds}")
    med = statistics.median
    for name, _ in calls:
        d, w = dev[name], wall[name]
        print(f"{name:20s} device {med(d):10.3f} ms (min {min(d):10.3f}, max {max(d):10.3f})  wall {med(w):10.3f} ms (min {min(w):10.3f}, max {max(w):10.3f})")
    print(f"groups_f64 per round: device {med(dev['groups_f64']) / summary.rounds:.3f} ms over {summary.rounds} rounds")
    print(f"host route ({what}): wall {host_s * 1e3:.1f} ms, one run, {host_groups} groups"
          + ("" if host_groups == summary.groups else "  (the tree's distances round differently: a count may differ at a tie)"))
    print(f"radius_counts_f64 device / nearest_f64 device {med(dev['radius_counts_f64']) / med(dev['nearest_f64']):.3f};  "
          f"groups_f64 wall / host route {med(wall['groups_f64']) / (host_s * 1e3):.4f}")


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
            raise SystemExit("groups_f64_measure: needs a HIP device")
        measure(nb, args.n[0], args.rounds)
        return 0
    lines = [f"# python tools/groups_f64_measure.py --n {' '.join(str(n) for n in args.n)} --rounds {args.rounds} on one GPU, one context and one process per N",
             "# fp64 state, Plummer sphere, b = 0.2 x the mean interparticle distance inside the half-mass radius",
             "# device = event pairs round the N^2 passes (nbody_kernel_time); wall = host clock round the call incl. synchronise and the copy of the results"]
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
