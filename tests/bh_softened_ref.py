"""ctypes front end of tests/cpp/bh_softened_ref.c — the oracle's octree path with Plummer softening in the walk's term.  TEST
INFRASTRUCTURE ONLY: the yardstick of the engine's softened Barnes-Hut walks (the oracle's own walk has no eps)."""
import ctypes
import os
import subprocess

import numpy as np

G = 1.0e4                    # OctreeSearch.h:104
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "bh_softened_ref.c")


def eps2f(eps):
    """eps * eps in double, rounded once to fp32 — what the engine passes to its walks (and the fp32 oracle's direct law uses)."""
    return np.float32(float(eps) * float(eps))


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class SoftenedRef:
    """Built with gcc into `workdir` (the flags of the oracle's Makefile that matter: -O2, -ffp-contract=off, no fast math)."""

    def __init__(self, workdir):
        so = os.path.join(str(workdir), "libbh_softened_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                               "-Werror", "-shared", SRC, "-o", so, "-lm"])
        L = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        L.bhs_octree_f32.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.c_float,
                                     ctypes.c_int, fp, fp, ctypes.POINTER(ctypes.c_int)]
        L.bhs_octree_f32.restype = ctypes.c_int
        L.bhs_tick_aos_f32.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.c_float,
                                       ctypes.c_int, fp, fp]
        L.bhs_tick_aos_f32.restype = ctypes.c_int
        self._L = L

    def forces(self, pos, mass, theta, eps=0.0, root_origin=(0.0, 0.0, 0.0), root_size=None, div_mode=0, g=G):
        """CreateOctree and every body's softened walk: (acc[n, 3], root CoM, node count).  root_size: ComputeCubeSize's by default."""
        pos = np.ascontiguousarray(pos, np.float32)
        mass = np.ascontiguousarray(mass, np.float32)
        n = pos.shape[0]
        if root_size is None:
            root_size = float(np.max(np.abs(pos))) if n else 0.0
        origin = np.ascontiguousarray(root_origin, np.float32)
        acc = np.zeros((n, 3), np.float32)
        com = np.zeros(3, np.float32)
        cnt = ctypes.c_int(0)
        rc = self._L.bhs_octree_f32(n, _fp(pos), _fp(mass), _fp(origin), np.float32(root_size), np.float32(theta), float(g),
                                    eps2f(eps), div_mode, _fp(acc), _fp(com), ctypes.byref(cnt))
        if rc:
            raise RuntimeError(f"bhs_octree_f32 rc={rc} (1 = past depth 200)")
        return acc, com, cnt.value

    def tick(self, particles, dt, theta, eps=0.0, root_com=None, div_mode=0, g=G):
        """One Tick on FParticle records (40 bytes each), in place.  Returns (root CoM, Size) as the oracle's tick_aos_f32 does."""
        assert particles.dtype.itemsize == 40 and particles.flags.c_contiguous
        com = np.zeros(3, np.float32) if root_com is None else np.array(root_com, np.float32)
        size = ctypes.c_float(0.0)
        rc = self._L.bhs_tick_aos_f32(particles.shape[0], particles.ctypes.data, np.float32(dt), np.float32(theta), float(g),
                                      eps2f(eps), div_mode, _fp(com), ctypes.byref(size))
        if rc:
            raise RuntimeError(f"bhs_tick_aos_f32 rc={rc}")
        return com, size.value
