"""What tests/golden/reference_*.npz hold and how they are recorded from the compiled reference (oracle/_ref/nbody_ref).

Shared by tests/golden/make_reference_golden.py (writes the files), tests/test_reference_build.py (holds them to the binary, no GPU)
and tests/test_reference_parity_gpu.py (holds the device to them; reads the files only — inputs() and the readers below — and never
the reference or oracle/_ref/).

A scene file:   dt; records0 (the inputs; the shipped scene takes them from refbox_n2000_seed1.npz instead); size[F], com[F,3]: Size
                and the root's centre of mass of frames 1..F; record_frames[k] and records[k,n]: the FParticle records after those
                frames; draw_frames[j], boxes[j,n,4], order[j,n]: what DrawOctreeBoxes drew in those frames with ShowOctree on — the
                boxes (Center, Extent) in the order drawn and the body whose point followed each box.
forces_theta0:  acc_<scene>[n,3]: the reference's Octree at theta = 0 (root: origin 0, ComputeCubeSize's Size): its all-pairs order."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARTICLE_DTYPE = np.dtype([("Mass", "<f4"), ("Position", "<f4", (3,)), ("Velocity", "<f4", (3,)), ("Acceleration", "<f4", (3,))])
DT = 0.01                                         # OctreeSearch.cpp:8
DEVICE_DEPTH = 42                                 # the device refuses deeper trees (include/nbody.h: nbody_set_bh_max_depth)
SCENES = {"refbox_n2000": 3, "n1": 4, "n2": 4, "n9": 4, "n300": 4}     # name -> frames
FORCES = ("n300", "refbox_n2000")
NAMES = tuple(SCENES) + ("forces_theta0",)


def file_name(name):
    return "reference_" + name + ".npz"


def _records(pos, mass, vel):
    q = np.zeros(len(mass), PARTICLE_DTYPE)
    q["Mass"], q["Position"], q["Velocity"] = mass, pos, vel
    return q


def _new_inputs(name):
    """A scene as CreateSpacePoints lays it out (OctreeSearch.cpp:58-72): a flat box, speeds of 250 to 500, body 0 heavy and at rest
    at the origin."""
    n = int(name[1:])
    rng = np.random.default_rng([49, n])
    pos = rng.uniform(-1, 1, (n, 3)) * (200.0, 200.0, 20.0)
    d = rng.normal(0, 1, (n, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(250, 500, (n, 1))
    mass = rng.uniform(1, 5000, n)
    if n == 1:
        return _records(pos, mass, vel)           # (one body, off the origin: Size > 0)
    pos[0], vel[0], mass[0] = 0.0, 0.0, 5000.0
    if n == 300:
        pos[5, 0] = 0.0                           # ON an octant boundary of the first root (GetOctant's >=, OctreeSearch.h:52-54) ...
        pos[6, 1] = -0.0                          # ... and from the other side of zero
        pos[7, :] = (0.0, 37.5, -0.0)
        mass[rng.random(n) < 0.2] = 0.0           # some massless bodies: they feel, and pull nothing
        mass[0] = 5000.0
    return _records(pos, mass, vel)


def inputs(name, stored=True):
    """The records a scene starts from: the committed ones (stored=True), or freshly made."""
    if name == "refbox_n2000":                    # the shipped scene: CreateSpacePoints(2000, 1000) as the product's generator seeds it
        g = np.load(os.path.join(GOLDEN, "refbox_n2000_seed1.npz"))
        return _records(g["posm"][:, :3], g["posm"][:, 3], g["vel"][:, :3])
    if stored:
        return np.load(os.path.join(GOLDEN, file_name(name)))["records0"]
    return _new_inputs(name)


def load(name):
    return np.load(os.path.join(GOLDEN, file_name(name)))


def record(name, ref, oracle, stored_inputs=True):
    """The arrays of one fixture, from the binary (ref = oracle.reference).  Asserts what the fixtures promise: trees no deeper than the
    device takes, and the oracle's bytes equal to the reference's under the default reading of the cube (pow_mode 0) and under the
    device's (pow_mode 3)."""
    if name == "forces_theta0":
        out = {}
        for scene in FORCES:
            q0 = inputs(scene, stored_inputs)
            size = oracle.bounds_f32(q0["Position"])
            assert oracle.octree_depth_f32(q0["Position"]) <= DEVICE_DEPTH
            out["acc_" + scene] = ref.run(q0, [ref.forces_command(0.0, (0.0, 0.0, 0.0), size)])[0]["acc"]
        return out

    frames = SCENES[name]
    q0 = inputs(name, stored_inputs)
    n = len(q0)
    assert len(np.unique(q0["Position"], axis=0)) == n
    got = ref.run(q0, [ref.ticks_command(DT, frames, True)])[0]
    keep = [frames] if name == "refbox_n2000" else list(range(1, frames + 1))          # frames whose records / draw calls are stored
    boxes, orders = [], []
    state = {pm: (q0.copy(), None, 0.0) for pm in (0, 3)}
    for f in range(1, frames + 1):
        before = state[0][0]["Position"].copy()
        origin = (0.0, 0.0, 0.0) if state[0][1] is None else state[0][1]
        for pm in (0, 3):
            q, com, size = state[pm]
            com, size = oracle.tick_aos_f32(q, DT, theta=1.0, root_com=com, size=size, pow_mode=pm)
            assert oracle.last_max_depth() <= DEVICE_DEPTH, (name, f, oracle.last_max_depth())
            assert q.tobytes() == got[f - 1]["records"].tobytes(), (name, f, pm)
            assert np.float32(size).tobytes() == got[f - 1]["size"].tobytes() and com.tobytes() == got[f - 1]["com"].tobytes(), (name, f, pm)
            state[pm] = (q, com, size)
        if f in keep:
            b, points = ref.draw_sequence(got[f - 1]["calls"])
            want_b, order = oracle.octree_leaves_f32(before, q0["Mass"], root_origin=origin, root_size=got[f - 1]["size"])
            after = got[f - 1]["records"]["Position"]
            assert len(np.unique(after, axis=0)) == n                                   # (so the points name their bodies)
            assert points.tobytes() == after[order].tobytes() and b.tobytes() == want_b.tobytes(), (name, f)
            boxes.append(b)
            orders.append(order.astype(np.int32))
    out = {"dt": np.float32(DT),
           "size": np.array([fr["size"] for fr in got], np.float32), "com": np.array([fr["com"] for fr in got], np.float32),
           "record_frames": np.array(keep, np.int32), "records": np.stack([got[f - 1]["records"] for f in keep]),
           "draw_frames": np.array(keep, np.int32), "boxes": np.stack(boxes), "order": np.stack(orders)}
    if name != "refbox_n2000":
        out["records0"] = q0
    return out
