"""ctypes front end of tests/cpp/bh_probe_ref.c — the reference's octree walked from points that are not bodies.  TEST
INFRASTRUCTURE ONLY: the yardstick of nbody_field_at and of the tracers at theta > 0."""
import ctypes
import os
import subprocess

import numpy as np

G = 1.0e4                    # OctreeSearch.h:104
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "bh_probe_ref.c")


def eps2f(eps):
    """eps * eps in double, rounded once to fp32 — what the engine passes to its walks."""
    return np.float32(float(eps) * float(eps))


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class ProbeRef:
    """Built with gcc into `workdir` (the flags of tests/bh_softened_ref.py: -O2, -ffp-contract=off, no fast math)."""

    def __init__(self, workdir):
        so = os.path.join(str(workdir), "libbh_probe_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                               "-Werror", "-shared", SRC, "-o", so, "-lm"])
        L = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        L.bhp_field_f32.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.c_float,
                                    ctypes.c_int, ctypes.c_int, fp, fp, fp, ctypes.POINTER(ctypes.c_int)]
        L.bhp_field_f32.restype = ctypes.c_int
        self._L = L

    def field(self, pos, mass, points, theta, eps=0.0, root_origin=(0.0, 0.0, 0.0), root_size=None, div_mode=0, g=G):
        """CreateOctree of the bodies (pos, mass) and the walk from every row of `points`: (acc[m, 3], root CoM, node count).
        root_size: ComputeCubeSize's by default."""
        pos = np.ascontiguousarray(pos, np.float32)
        mass = np.ascontiguousarray(mass, np.float32)
        pts = np.ascontiguousarray(points, np.float32)
        n, m = pos.shape[0], pts.shape[0]
        assert pos.shape == (n, 3) and pts.shape == (m, 3) and mass.shape == (n,)
        if root_size is None:
            root_size = float(np.max(np.abs(pos))) if n else 0.0
        origin = np.ascontiguousarray(root_origin, np.float32)
        acc = np.zeros((m, 3), np.float32)
        com = np.zeros(3, np.float32)
        cnt = ctypes.c_int(0)
        rc = self._L.bhp_field_f32(n, _fp(pos), _fp(mass), _fp(origin), np.float32(root_size), np.float32(theta), float(g), eps2f(eps),
                                   div_mode, m, _fp(pts), _fp(acc), _fp(com), ctypes.byref(cnt))
        if rc:
            raise RuntimeError(f"bhp_field_f32 rc={rc} (1 = past depth 200)")
        return acc, com, cnt.value
