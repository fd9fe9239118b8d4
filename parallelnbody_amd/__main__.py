"""Command-line replay of the reference's scene: the parameter surface of BP_ScreenUI
(NParticles, BoxSize, DeltaTime, Pause via --dt 0) driving the AOctreeSearch-shaped engine.

    python -m parallelnbody_amd --n 2000 --size 1000 --dt 0.01 --steps 600          # the shipped scene
    python -m parallelnbody_amd --plummer --n 65536 --eps 1 --steps 100 --energy-every 20
    python -m parallelnbody_amd --n 2000 --steps 300 --checkpoint run.ckpt ; python -m parallelnbody_amd --n 2000 --resume run.ckpt --steps 300
    python -m parallelnbody_amd --n 2000 --theta 1.0 --steps 600 --trajectory run.trj --trajectory-every 10   # as shipped: Barnes-Hut, theta = 1
    python -m parallelnbody_amd --n 2000 --theta 1.0 --eps 5 --steps 600          # Barnes-Hut with every accepted node's term softened
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --integrator hermite --eta 0.02 --dt 0.05 --steps 20 --energy-every 5
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --integrator hermite-block --levels 12 --dt 0.05 --steps 20 --energy-every 5
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --integrator hermite6 --eta 0.5 --dt 0.05 --steps 20 --energy-every 5
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --integrator hermite6-block --levels 12 --eta 0.5 --dt 0.05 --steps 20 --energy-every 5
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --steps 20 --core-every 5 --core-k 6       # density centre and core radius
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --steps 20 --lagrange-every 5 --lagrange-fractions 0.1,0.5,0.9   # Lagrangian radii
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --steps 20 --groups-every 5 --linking-length 0.02   # friends-of-friends groups
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --steps 20 --mst-every 5       # minimum spanning tree: length, mean and longest edge
    python -m parallelnbody_amd --plummer --n 4096 --precision f64 --steps 20 --pairs-every 5 --pair-radii 0.01,0.02,0.05,0.1   # pairs within each radius

Trajectory file (nothing in the reference to mirror): header `NBDYTRJ1`, int32 n, int32 reserved, then per
dumped frame int64 frame number + n x 3 float32 positions — `read_trajectory(path)` returns (frames, positions[k, n, 3]).
"""
import argparse
import json
import sys
import time

import numpy as np

from . import NBodyEngine, ic_plummer, ic_reference_box
from .engine import LAGRANGE_FRACTIONS


TRJ_MAGIC = b"NBDYTRJ1"


def read_trajectory(path):
    """(frame numbers [k], positions [k, n, 3] float32) of a file written by --trajectory."""
    with open(path, "rb") as f:
        if f.read(8) != TRJ_MAGIC:
            raise ValueError(f"{path}: not a trajectory file")
        n = int(np.frombuffer(f.read(8), np.int32)[0])
        rec = np.dtype([("frame", "<i8"), ("pos", "<f4", (n, 3))])
        data = np.frombuffer(f.read(), rec)
    return data["frame"].copy(), data["pos"].copy()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m parallelnbody_amd", description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=2000, help="NParticles (BP_ScreenUI default 2000)")
    ap.add_argument("--size", type=float, default=1000.0, help="BoxSize (BP_ScreenUI default 1000)")
    ap.add_argument("--dt", type=float, default=0.01, help="DeltaTime = PhDeltaTime (default 0.01; <= 0 pauses)")
    ap.add_argument("--steps", type=int, default=100, help="frames to advance")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--plummer", action="store_true", help="seeded Plummer sphere instead of CreateSpacePoints' box")
    ap.add_argument("--eps", type=float, default=0.0, help="softening length (reference: 0)")
    ap.add_argument("--G", type=float, default=1.0e4, help="gravitational constant (reference: 1e4)")
    ap.add_argument("--precision", default="f32", choices=["f32", "f32_kahan", "f64"])
    ap.add_argument("--integrator", default="kickdrift", choices=["kickdrift", "hermite", "hermite-block", "hermite6", "hermite6-block"],
                    help="kickdrift: the reference's v += dt a; x += dt v (default).  hermite: the fourth-order Hermite "
                         "predictor-corrector (needs --precision f64, theta = 0): one step of --dt per frame, or with --eta "
                         "adaptive shared steps that cover --dt per frame.  hermite-block: the same scheme with a step per body, "
                         "--dt 2^-level with level 0 .. --levels chosen by --eta (default 0.02); every frame of --dt ends synchronised"
                         ".  hermite6: the sixth-order Hermite predictor-corrector on the snap pass (--precision f64, theta = 0), "
                         "driven like hermite: one step of --dt per frame, or with --eta adaptive shared steps dt = eta t — no "
                         "square root in this criterion: 0.5 does what 0.01 does for hermite (--eta 0 < eta; without it steps are fixed).  "
                         "hermite6-block: the sixth-order scheme with a step per body, driven like hermite-block (--levels, default 12; "
                         "--eta, default 0.5, multiplies the sixth-root time scale directly)")
    ap.add_argument("--levels", type=int, default=None,
                    help="--integrator hermite-block and hermite6-block: the deepest level, 0 .. 40 (default 12): the smallest step is --dt 2^-levels")
    ap.add_argument("--eta", type=float, default=None,
                    help="--integrator hermite: Aarseth's accuracy parameter; every frame of length --dt is covered by adaptive steps "
                         "dt = sqrt(eta) t (0.01 t for a frame's first step after a restart)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--energy-every", type=int, default=0, help="print kinetic/potential energy every K frames")
    ap.add_argument("--fast-energy", action="store_true",
                    help="energy lines come from energy_fast(): the potential energy from the per-body potentials — at theta > 0 the "
                         "walk of the tree of the current positions, about one force pass instead of all pairs (plain f32 only; at "
                         "theta > 0 the stored accelerations become those of the current positions, the trajectory is unchanged)")
    ap.add_argument("--moments-every", type=int, default=0,
                    help="print |P|, |L|, the centre of mass, |net force|, |net torque| and the virial every K frames (one O(N) pass on "
                         "the device; force, torque and virial are those of the accelerations the last step stored)")
    ap.add_argument("--core-every", type=int, default=0,
                    help="print the density centre, the core radius, the densest body and the core mass every K frames (--precision f64 "
                         "only: one neighbour pass over all pairs and two O(N) reductions on the device; Casertano & Hut's local "
                         "densities in NBODY6's convention)")
    ap.add_argument("--core-k", type=int, default=6, help="--core-every: the neighbour that sets a body's density sphere, 2 .. 8 (default 6)")
    ap.add_argument("--lagrange-every", type=int, default=0,
                    help="print the Lagrangian radii about the density centre every K frames (--precision f64 only: the neighbour pass "
                         "of --core-every for the centre — --core-k is shared —, then one sort by distance and a cumulative mass on the "
                         "device)")
    ap.add_argument("--lagrange-fractions", default=None,
                    help="--lagrange-every: the mass fractions, f,f,... each in (0, 1], at most 64 (default "
                         "0.01,0.02,0.05,0.1,0.2,0.3,0.5,0.7,0.9)")
    ap.add_argument("--groups-every", type=int, default=0,
                    help="print the friends-of-friends groups at --linking-length every K frames: their number, the multiples, the "
                         "largest group's label and size, and the links (--precision f64 only: a few passes over all pairs on the "
                         "device, one per round of the group finder)")
    ap.add_argument("--linking-length", type=float, default=None,
                    help="--groups-every: bodies closer than this are linked, finite and >= 0")
    ap.add_argument("--mst-every", type=int, default=0,
                    help="print the Euclidean minimum spanning tree every K frames: its edges, components, total length, mean and longest "
                         "edge, and the rounds taken (--precision f64 only: a few passes over all pairs on the device, one per Boruvka "
                         "round)")
    ap.add_argument("--pairs-every", type=int, default=0,
                    help="print the pair counts at --pair-radii every K frames: the unordered pairs of bodies within each radius "
                         "(--precision f64 only: one pass over all pairs on the device per 16 distinct radii)")
    ap.add_argument("--pair-radii", default=None,
                    help="--pairs-every: the radii, r,r,... each finite and >= 0, in any order, at most 64")
    ap.add_argument("--checkpoint", help="write the final state here")
    ap.add_argument("--resume", help="start from this checkpoint instead of fresh initial conditions")
    ap.add_argument("--dump-positions", help="write the final positions (n x 3 float32, .npy)")
    ap.add_argument("--theta", type=float, default=None,
                    help="opening angle: 0 = exact all-pairs (default); 1.0 = the reference's shipped Barnes-Hut walk.  With "
                         "--resume: the file's own opening angle unless this option says otherwise (then it is announced)")
    ap.add_argument("--bh-max-depth", type=int, default=None,
                    help="the deepest Barnes-Hut tree a frame may build, 42 .. 200 (default 42: deeper frames are refused)")
    ap.add_argument("--sync-energy", action="store_true",
                    help="energy lines also carry the total with the staggered velocity pulled to the positions' time "
                         "(v_n = v_{n-1/2} + dt/2 a_n: one extra force pass per line.  Positions, velocities and — at theta > 0 — "
                         "the root of the next tree are not touched, so the trajectory is the same with and without; the stored "
                         "accelerations are those of the extra pass)")
    ap.add_argument("--leapfrog-start", action="store_true",
                    help="fresh runs only: store v_{-1/2} = v_0 - dt/2 a_0, so the update (v += dt a; x += dt v) is a proper leapfrog")
    ap.add_argument("--trajectory", help="write positions every --trajectory-every frames to this file (read_trajectory reads it back)")
    ap.add_argument("--trajectory-every", type=int, default=1)
    a = ap.parse_args(argv)

    if a.trajectory_every < 1:
        ap.error("--trajectory-every must be >= 1")
    if a.core_every < 0:
        ap.error("--core-every must be >= 0")
    if a.core_every > 0 and a.precision != "f64":
        ap.error("--core-every needs --precision f64: the neighbour census runs on fp64 contexts only")
    if a.core_every > 0 and not 2 <= a.core_k <= 8:
        ap.error("--core-k must be 2 .. 8")
    if a.lagrange_every < 0:
        ap.error("--lagrange-every must be >= 0")
    if a.lagrange_every > 0 and a.precision != "f64":
        ap.error("--lagrange-every needs --precision f64: the radial census runs on fp64 contexts only")
    if a.lagrange_every > 0 and not 2 <= a.core_k <= 8:
        ap.error("--core-k must be 2 .. 8")
    if a.lagrange_fractions is not None and a.lagrange_every == 0:
        ap.error("--lagrange-fractions belongs to --lagrange-every")
    if a.groups_every < 0:
        ap.error("--groups-every must be >= 0")
    if a.groups_every > 0 and a.precision != "f64":
        ap.error("--groups-every needs --precision f64: the group census runs on fp64 contexts only")
    if a.groups_every > 0 and a.linking_length is None:
        ap.error("--groups-every needs --linking-length")
    if a.linking_length is not None and a.groups_every == 0:
        ap.error("--linking-length belongs to --groups-every")
    if a.linking_length is not None and not (0.0 <= a.linking_length < float("inf")):
        ap.error("--linking-length must be finite and >= 0")
    if a.mst_every < 0:
        ap.error("--mst-every must be >= 0")
    if a.mst_every > 0 and a.precision != "f64":
        ap.error("--mst-every needs --precision f64: the minimum spanning tree runs on fp64 contexts only")
    if a.pairs_every < 0:
        ap.error("--pairs-every must be >= 0")
    if a.pairs_every > 0 and a.precision != "f64":
        ap.error("--pairs-every needs --precision f64: the separation census runs on fp64 contexts only")
    if a.pairs_every > 0 and a.pair_radii is None:
        ap.error("--pairs-every needs --pair-radii")
    if a.pair_radii is not None and a.pairs_every == 0:
        ap.error("--pair-radii belongs to --pairs-every")
    pair_radii = ()
    if a.pair_radii is not None:
        try:
            pair_radii = tuple(float(r) for r in a.pair_radii.split(","))
        except ValueError:
            pair_radii = ()
        if not 1 <= len(pair_radii) <= 64 or not all(0.0 <= r < float("inf") for r in pair_radii):
            ap.error("--pair-radii must be 1 .. 64 comma-separated radii, each finite and >= 0")
    fractions = LAGRANGE_FRACTIONS
    if a.lagrange_fractions is not None:
        try:
            fractions = tuple(float(f) for f in a.lagrange_fractions.split(","))
        except ValueError:
            fractions = ()
        if not 1 <= len(fractions) <= 64 or not all(0.0 < f <= 1.0 for f in fractions):
            ap.error("--lagrange-fractions must be 1 .. 64 numbers f,f,... each in (0, 1]")
    block6 = a.integrator == "hermite6-block"                        # the same demands and exclusions as hermite-block
    block = a.integrator == "hermite-block" or block6
    hermite = a.integrator == "hermite" or block
    six = a.integrator == "hermite6"                                 # the same demands and exclusions as hermite
    hermite = hermite or six
    if hermite and a.precision != "f64":
        ap.error(f"--integrator {a.integrator} needs --precision f64")
    if hermite and (a.theta or a.leapfrog_start or a.sync_energy):
        ap.error("--integrator hermite steps synchronised velocities at theta = 0: not with --theta, --leapfrog-start or --sync-energy")
    if a.eta is not None and not (hermite and a.eta > 0):
        ap.error("--eta belongs to --integrator hermite and hermite-block and must be > 0")
    if a.levels is not None and not (block and 0 <= a.levels <= 40):
        ap.error("--levels belongs to --integrator hermite-block and hermite6-block and must be 0 .. 40")
    posm, vel = (ic_plummer(a.n, G=a.G, seed=a.seed) if a.plummer else ic_reference_box(a.n, a.size, seed=a.seed))
    with NBodyEngine(a.n, device=a.device, precision=a.precision, G=a.G, eps=a.eps, theta=a.theta or 0.0) as e:
        e.set_state(posm, vel)
        start = e.load_checkpoint(a.resume) if a.resume else 0
        if a.resume and a.theta is not None and e.theta() != np.float32(a.theta):
            print(f"--resume: {a.resume} was written at theta = {e.theta():g}; continuing at --theta {a.theta:g} as asked "
                  "(not the trajectory the file belongs to)", file=sys.stderr)
            e.set_theta(a.theta)
        if a.bh_max_depth is not None:
            e.set_bh_max_depth(a.bh_max_depth)
        f64 = a.precision == "f64"
        if a.leapfrog_start and not a.resume and a.dt > 0:
            e.compute_forces()
            p0, v0, a0 = e.state(np.float64 if f64 else np.float32)
            v0[:, :3] = (v0[:, :3].astype(np.float64) - 0.5 * a.dt * a0[:, :3].astype(np.float64)).astype(v0.dtype)
            e.set_state(p0, v0)

        def energies():
            ke, pe = e.energy_fast() if a.fast_energy else e.energy()
            out = {"kinetic": ke, "potential": pe, "total": ke + pe}
            if a.sync_energy:
                e.compute_forces()                               # a(x_n); positions and velocities are not touched
                p, v, acc = e.state(np.float64)
                vs = v[:, :3] + 0.5 * a.dt * acc[:, :3]
                out["total_synchronised"] = 0.5 * float((p[:, 3] * (vs ** 2).sum(1)).sum()) + pe
            return out
        session = []
        def advance(frames):
            if not hermite:
                e.step(a.dt, frames)
            elif block:
                if a.dt > 0 and frames > 0:
                    if not session:                              # one session for the run: nothing below ends it
                        if block6:
                            e.hermite6_block_begin(a.dt, 12 if a.levels is None else a.levels, eta=a.eta or 0.5)
                        else:
                            e.hermite_block_begin(a.dt, 12 if a.levels is None else a.levels, eta=a.eta or 0.02)
                        session.append(True)
                    (e.hermite6_block_advance if block6 else e.hermite_block_advance)(frames)
            elif six and a.eta is None:
                e.hermite6_step(a.dt, frames)
            elif six:
                for _ in range(frames if a.dt > 0 else 0):
                    e.hermite6_advance(a.dt, eta=a.eta)
            elif a.eta is None:
                e.hermite_step(a.dt, frames)
            else:
                for _ in range(frames if a.dt > 0 else 0):
                    e.hermite_advance(a.dt, eta=a.eta)
        trj = None
        if a.trajectory:
            trj = open(a.trajectory, "wb")
            trj.write(TRJ_MAGIC + np.array([a.n, 0], np.int32).tobytes())
            frame_buf = np.empty((a.n, 3), np.float32)
            e.pin(frame_buf)                                     # frames land in it by one DMA
        # advance in chunks that end on every frame somebody wants to see
        marks = [m for m in (a.energy_every, a.moments_every, a.core_every, a.lagrange_every, a.groups_every, a.mst_every, a.pairs_every, a.trajectory_every if trj else 0) if m > 0]
        if a.energy_every > 0 and a.sync_energy and not a.resume:
            print(json.dumps({"frame": start, **energies()}), flush=True)
        t0 = time.perf_counter()
        done = 0
        while done < a.steps:
            k = min([a.steps - done] + [m - (start + done) % m for m in marks])
            advance(k)
            done += k
            frame = start + done
            if a.energy_every > 0 and frame % a.energy_every == 0:
                print(json.dumps({"frame": frame, **energies()}), flush=True)
            if a.moments_every > 0 and frame % a.moments_every == 0:
                m = e.moments()
                norm = lambda v: float(np.sqrt((np.asarray(v) ** 2).sum()))
                print(json.dumps({"frame": frame, "moments": {"P": norm(m.p), "L": norm(m.l), "com": [float(c) for c in m.com],
                                                              "net_force": norm(m.force), "net_torque": norm(m.torque),
                                                              "virial": m.virial}}), flush=True)
            if a.core_every > 0 and frame % a.core_every == 0:
                c = e.core_f64(a.core_k)
                print(json.dumps({"frame": frame, "core": {"k": c.k, "centre": [float(x) for x in c.centre], "core_radius": c.core_radius,
                                                           "densest": c.densest, "rho_max": c.rho_max, "used": c.used,
                                                           "core_mass": c.core_mass, "core_count": c.core_count}}), flush=True)
            if a.lagrange_every > 0 and frame % a.lagrange_every == 0:
                g = e.lagrange_f64(fractions, k=a.core_k)
                print(json.dumps({"frame": frame, "lagrange": {"centre": [float(x) for x in g.centre], "total_mass": g.total_mass,
                                                               "fractions": [float(f) for f in g.fraction],
                                                               "radii": [float(r) for r in g.radius],
                                                               "bodies": [int(b) for b in g.body],
                                                               "counts": [int(c) for c in g.count]}}), flush=True)
            if a.groups_every > 0 and frame % a.groups_every == 0:
                g = e.groups_f64(a.linking_length).summary
                print(json.dumps({"frame": frame, "groups": {"linking_length": a.linking_length, "groups": g.groups,
                                                             "multiples": g.multiples, "largest": g.largest,
                                                             "largest_members": g.largest_members, "links": g.links}}), flush=True)
            if a.mst_every > 0 and frame % a.mst_every == 0:
                t = e.mst_f64().summary
                print(json.dumps({"frame": frame, "mst": {"edges": t.edges, "components": t.components, "length": t.length,
                                                          "mean_edge": t.length / t.edges if t.edges else 0.0,
                                                          "longest_edge": float(np.sqrt(t.longest_d2)), "rounds": t.rounds}}), flush=True)
            if a.pairs_every > 0 and frame % a.pairs_every == 0:
                counts = e.pair_counts_f64(pair_radii)
                print(json.dumps({"frame": frame, "pairs": {"radii": list(pair_radii), "counts": [int(c) for c in counts]}}), flush=True)
            if trj and frame % a.trajectory_every == 0:
                e.positions(out=frame_buf)
                trj.write(np.int64(frame).tobytes() + frame_buf.tobytes())
        e.synchronize()
        if trj:
            trj.close()
        wall = time.perf_counter() - t0
        size = e.bounds()
        if a.checkpoint:
            e.save_checkpoint(a.checkpoint)
        if a.dump_positions:
            np.save(a.dump_positions, e.positions())
        cfg = e.launch_config()
        print(json.dumps({"n": a.n, "frames": a.steps, "first_frame": start, "dt": a.dt, "wall_s": wall,
                          "frames_per_s": a.steps / wall if wall > 0 else None,
                          "pair_interactions_per_s": a.n * a.n * a.steps / wall if wall > 0 and a.dt > 0 else 0.0,
                          "Size": size, "algorithm": cfg["algorithm"], "steps_done": e.steps_done()}))


if __name__ == "__main__":
    main()
