"""Front end of oracle/ref_driver.cpp: finds (or builds) oracle/_ref/nbody_ref — the reference's own OctreeSearch.cpp, compiled
unchanged against oracle/ue4_standin/ — writes its scene files, runs it as a child process and reads its result files.
TEST INFRASTRUCTURE ONLY: tests/test_reference_build.py, tests/golden/make_reference_golden.py and, for the file format alone
(`run(binary=...)` on the adapter program), tests/test_reference_parity_gpu.py.

The reference does not terminate on coincident bodies or on bodies no fp32 centre can separate (Octree::Add, OctreeSearch.h:60-81,
recurses for ever).  So the program always runs as a child under TIME_LIMIT seconds, and callers send it only scenes whose insertion
depth the oracle has measured (`oracle.octree_depth_f32`, `oracle.last_max_depth()` after every oracle frame): at most MAX_DEPTH.
A non-zero exit status or a time-out raises; it is a failure, never a reason to skip.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

from .oracle import PARTICLE_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
BINARY = os.path.join(_HERE, "_ref", "nbody_ref")
TIME_LIMIT = 60      # seconds per run of the program
MAX_DEPTH = 150      # deepest insertion (root = 0) a scene sent to the reference may reach; the oracle itself cuts off at 200

CALL_DTYPE = np.dtype([("kind", "<i4"), ("v", "<f4", (6,))])   # ref_driver.cpp's DrawCall: 0 = box (Center, Extent), 1 = point (Position, Size)


def reference_dir():
    """Where the reference's sources are looked for (the Makefile's REFERENCE_DIR)."""
    return os.environ.get("REFERENCE_DIR", "/root/reference")


def have_sources():
    return os.path.isfile(os.path.join(reference_dir(), "Source", "NBody", "OctreeSearch.cpp"))


def build():
    """`make reference`: compiles _ref/nbody_ref where the reference's sources exist, and leaves _ref/ untouched where they do not.
    Returns the binary's path, or None if there is none."""
    if have_sources():
        subprocess.check_call(["make", "-C", _HERE, "--no-print-directory", "reference", "REFERENCE_DIR=" + reference_dir()],
                              stdout=subprocess.DEVNULL)
    return BINARY if os.path.isfile(BINARY) else None


def available():
    """Can a test run the reference?  False in one case only: no binary and no sources to build it from."""
    return os.path.isfile(BINARY) or have_sources()


def particles(pos, mass, vel=None):
    q = np.zeros(len(mass), PARTICLE_DTYPE)
    q["Mass"] = mass
    q["Position"] = pos
    if vel is not None:
        q["Velocity"] = np.asarray(vel)[:, :3]
    return q


def _hex(x):
    return float(np.float32(x)).hex()          # every bit of the float survives strtof


def ticks_command(dt, frames, show_octree=True):
    return ("ticks", _hex(dt), int(frames), int(bool(show_octree)))


def forces_command(theta, origin=(0.0, 0.0, 0.0), size=0.0):
    return ("forces", _hex(theta), _hex(origin[0]), _hex(origin[1]), _hex(origin[2]), _hex(size))


def run(records, commands, binary=None, env=None):
    """Run the program on one scene.  `commands`: what ticks_command / forces_command return.  Returns one entry per command:
    ticks  -> list of frames, each {"records", "size", "com", "calls"} (calls: CALL_DTYPE, in the order drawn)
    forces -> {"acc": [n,3], "com": [3]}"""
    binary = binary or build()
    if binary is None:
        raise FileNotFoundError("oracle/_ref/nbody_ref is not built and the reference's sources are not at " + reference_dir())
    records = np.ascontiguousarray(records)
    assert records.dtype == PARTICLE_DTYPE and records.ndim == 1 and records.shape[0] >= 1
    n = records.shape[0]
    with tempfile.TemporaryDirectory(prefix="nbody_ref_") as tmp:
        scene, result = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "result.bin")
        with open(scene, "wb") as f:
            f.write(b"NBSCENE1" + struct.pack("<i", n) + records.tobytes())
            f.write("".join(" ".join(str(w) for w in c) + "\n" for c in commands).encode())
        out = subprocess.run([binary, scene, result], capture_output=True, text=True, timeout=TIME_LIMIT, env=env)
        if out.returncode != 0:
            raise RuntimeError(f"{os.path.basename(binary)} exit status {out.returncode}: {out.stderr.strip()}")
        blob = open(result, "rb").read()
    assert blob[:8] == b"NBRESLT1", blob[:8]
    at = 8

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(blob, dtype, count, at).copy()
        at += a.nbytes
        return a

    results = []
    for c in commands:
        if c[0] == "ticks":
            frames = []
            for _ in range(c[2]):
                rec = take(PARTICLE_DTYPE, n)
                size = take("<f4", 1)[0]
                com = take("<f4", 3)
                calls = take(CALL_DTYPE, int(take("<i4", 1)[0]))
                frames.append({"records": rec, "size": size, "com": com, "calls": calls})
            results.append(frames)
        else:
            results.append({"acc": take("<f4", 3 * n).reshape(n, 3), "com": take("<f4", 3)})
    assert at == len(blob), (at, len(blob))
    return results


def draw_sequence(calls):
    """(boxes[k,4] = Center and Extent.X of the boxes, points[m,3]) of one frame's calls, each in the order drawn; asserts what
    DrawOctreeBoxes promises (OctreeSearch.cpp:39-41): a cube, and — when boxes are drawn at all — box, point, box, point ..."""
    box = calls[calls["kind"] == 0]["v"]
    point = calls[calls["kind"] == 1]["v"]
    assert len(box) + len(point) == len(calls)
    assert (box[:, 3] == box[:, 4]).all() and (box[:, 3] == box[:, 5]).all()
    assert (point[:, 3] == np.float32(10.0)).all()
    if len(box):
        assert len(box) == len(point) and (calls["kind"] == np.tile([0, 1], len(box))).all()
    return np.ascontiguousarray(box[:, :4]), np.ascontiguousarray(point[:, :3])
