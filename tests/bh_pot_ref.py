"""ctypes front end of tests/cpp/bh_pot_ref.c — the reference's octree walked from arbitrary points, returning the potential next to
the acceleration.  TEST INFRASTRUCTURE ONLY: the yardstick of nbody_potential_at, nbody_get_potentials and nbody_energy_fast at
theta > 0."""
import ctypes
import os
import subprocess

import numpy as np

from bh_probe_ref import G, eps2f

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "bh_pot_ref.c")


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class PotRef:
    """Built with gcc into `workdir` (the flags of tests/bh_probe_ref.py: -O2, -ffp-contract=off, no fast math)."""

    def __init__(self, workdir):
        so = os.path.join(str(workdir), "libbh_pot_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                               "-Werror", "-shared", SRC, "-o", so, "-lm"])
        L = ctypes.CDLL(so)
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        L.bhpot_walk_f32.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.c_float,
                                     ctypes.c_int, ctypes.c_int, fp, fp, dp, fp, fp, fp, ctypes.POINTER(ctypes.c_int)]
        L.bhpot_walk_f32.restype = ctypes.c_int
        self._L = L

    def walk(self, pos, mass, points, theta, eps=0.0, root_origin=(0.0, 0.0, 0.0), root_size=None, div_mode=0, g=G):
        """CreateOctree of the bodies (pos, mass) and the walk from every row of `points`: a dict with acc [m,3] float32, phi64 [m]
        float64 (minus the fp64 sum in walk order), phi [m] float32 (phi64 rounded once), root_com [3], root_mass, nodes.
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
        phi64 = np.zeros(m, np.float64)
        phi = np.zeros(m, np.float32)
        com = np.zeros(3, np.float32)
        rmass = ctypes.c_float(0.0)
        cnt = ctypes.c_int(0)
        rc = self._L.bhpot_walk_f32(n, _fp(pos), _fp(mass), _fp(origin), np.float32(root_size), np.float32(theta), float(g), eps2f(eps),
                                    div_mode, m, _fp(pts), _fp(acc), phi64.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _fp(phi),
                                    _fp(com), ctypes.byref(rmass), ctypes.byref(cnt))
        if rc:
            raise RuntimeError(f"bhpot_walk_f32 rc={rc} (1 = past depth 200)")
        return {"acc": acc, "phi64": phi64, "phi": phi, "root_com": com, "root_mass": rmass.value, "nodes": cnt.value}


def direct_potential(pos, mass, pts, eps=0.0, g=G, skip_self=False):
    """numpy fp64 direct sum: phi(x) = -sum_j g m_j / sqrt(|x - x_j|^2 + eps^2); with eps == 0 a pair at distance 0 adds nothing.
    skip_self: pts are the bodies themselves and row k leaves body k out by index."""
    pos = np.asarray(pos, np.float64); mass = np.asarray(mass, np.float64); pts = np.asarray(pts, np.float64)
    out = np.empty(pts.shape[0], np.float64)
    e2 = float(eps) * float(eps)
    blk = max(16, min(1024, 2_000_000 // max(1, pos.shape[0])))
    for a in range(0, pts.shape[0], blk):
        d = pts[a:a + blk, None, :] - pos[None, :, :]
        r2 = (d * d).sum(-1) + e2
        with np.errstate(divide="ignore"):
            inv = np.where(r2 > 0.0, 1.0 / np.sqrt(r2), 0.0)
        if skip_self:
            k = np.arange(a, min(a + blk, pts.shape[0]))
            inv[k - a, k] = 0.0
        out[a:a + blk] = -g * (inv * mass[None, :]).sum(1)
    return out
