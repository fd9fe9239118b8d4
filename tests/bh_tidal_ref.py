"""ctypes front end of tests/cpp/bh_tidal_ref.c — the reference's octree walked from arbitrary points, returning the tidal tensor next
to the acceleration — and the numpy fp64 direct sum of the theta == 0 definition.  TEST INFRASTRUCTURE ONLY: the yardsticks of
nbody_tidal_at, nbody_get_tidal and nbody_tidal_time."""
import ctypes
import os
import subprocess

import numpy as np

from bh_probe_ref import G, eps2f

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "bh_tidal_ref.c")


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class TidalRef:
    """Built with gcc into `workdir` (the flags of tests/bh_pot_ref.py: -O2, -ffp-contract=off, no fast math)."""

    def __init__(self, workdir):
        so = os.path.join(str(workdir), "libbh_tidal_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                               "-Werror", "-shared", SRC, "-o", so, "-lm"])
        L = ctypes.CDLL(so)
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        L.bhtidal_walk_f32.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.c_float,
                                       ctypes.c_int, ctypes.c_int, fp, fp, dp, fp, fp, fp, ctypes.POINTER(ctypes.c_int)]
        L.bhtidal_walk_f32.restype = ctypes.c_int
        self._L = L

    def walk(self, pos, mass, points, theta, eps=0.0, root_origin=(0.0, 0.0, 0.0), root_size=None, div_mode=0, g=G):
        """CreateOctree of the bodies (pos, mass) and the walk from every row of `points`: a dict with acc [m,3] float32, t64 [m,6]
        float64 (xx, yy, zz, xy, xz, yz from the fp64 sums in walk order), t [m,6] float32 (t64 rounded once), root_com [3], root_mass,
        nodes.  root_size: ComputeCubeSize's by default."""
        pos = np.ascontiguousarray(pos, np.float32)
        mass = np.ascontiguousarray(mass, np.float32)
        pts = np.ascontiguousarray(points, np.float32)
        n, m = pos.shape[0], pts.shape[0]
        assert pos.shape == (n, 3) and pts.shape == (m, 3) and mass.shape == (n,)
        if root_size is None:
            root_size = float(np.max(np.abs(pos))) if n else 0.0
        origin = np.ascontiguousarray(root_origin, np.float32)
        acc = np.zeros((m, 3), np.float32)
        t64 = np.zeros((m, 6), np.float64)
        t = np.zeros((m, 6), np.float32)
        com = np.zeros(3, np.float32)
        rmass = ctypes.c_float(0.0)
        cnt = ctypes.c_int(0)
        rc = self._L.bhtidal_walk_f32(n, _fp(pos), _fp(mass), _fp(origin), np.float32(root_size), np.float32(theta), float(g), eps2f(eps),
                                      div_mode, m, _fp(pts), _fp(acc), t64.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _fp(t),
                                      _fp(com), ctypes.byref(rmass), ctypes.byref(cnt))
        if rc:
            raise RuntimeError(f"bhtidal_walk_f32 rc={rc} (1 = past depth 200)")
        return {"acc": acc, "t64": t64, "t": t, "root_com": com, "root_mass": rmass.value, "nodes": cnt.value}


def direct_tidal(pos, mass, pts, eps=0.0, skip_self=False, g=G):
    """numpy fp64 direct sum: T_ab(x) = sum_j g m_j [3 d_a d_b / s^5 - delta_ab / s^3], d = x_j - x, s^2 = |d|^2 + eps^2, as [m,6]
    (xx, yy, zz, xy, xz, yz); with eps == 0 a pair at distance 0 adds nothing.  skip_self: pts are the bodies themselves and row k
    leaves body k out by index."""
    pos = np.asarray(pos, np.float64); mass = np.asarray(mass, np.float64); pts = np.asarray(pts, np.float64)
    out = np.empty((pts.shape[0], 6), np.float64)
    e2 = float(eps) * float(eps)
    blk = max(16, min(1024, 2_000_000 // max(1, pos.shape[0])))
    for a in range(0, pts.shape[0], blk):
        d = pos[None, :, :] - pts[a:a + blk, None, :]
        r2 = (d * d).sum(-1) + e2
        with np.errstate(divide="ignore"):
            inv = np.where(r2 > 0.0, 1.0 / np.sqrt(np.where(r2 > 0.0, r2, 1.0)), 0.0)
        if skip_self:
            k = np.arange(a, min(a + blk, pts.shape[0]))
            inv[k - a, k] = 0.0
        q = g * mass[None, :] * inv * inv * inv                   # g m / s^3
        u = d * inv[:, :, None]                                   # d / s
        h = 3.0 * q
        qs = q.sum(1)
        o = out[a:a + blk]
        o[:, 0] = (h * u[:, :, 0] * u[:, :, 0]).sum(1) - qs
        o[:, 1] = (h * u[:, :, 1] * u[:, :, 1]).sum(1) - qs
        o[:, 2] = (h * u[:, :, 2] * u[:, :, 2]).sum(1) - qs
        o[:, 3] = (h * u[:, :, 0] * u[:, :, 1]).sum(1)
        o[:, 4] = (h * u[:, :, 0] * u[:, :, 2]).sum(1)
        o[:, 5] = (h * u[:, :, 1] * u[:, :, 2]).sum(1)
    return out


def frob(t):
    """||T||_F of [m,6] tensors (xx, yy, zz, xy, xz, yz): the off-diagonal entries counted twice."""
    t = np.asarray(t, np.float64)
    return np.sqrt((t[:, :3] ** 2).sum(1) + 2.0 * (t[:, 3:] ** 2).sum(1))


def n2_of(t64):
    """The squared Frobenius norm as nbody_tidal_time forms it, operation by operation in fp64."""
    t = np.asarray(t64, np.float64)
    xx, yy, zz, xy, xz, yz = (t[:, c] for c in range(6))
    return (xx * xx + yy * yy) + zz * zz + 2.0 * ((xy * xy + xz * xz) + yz * yz)


def emulate_tidal_f32(pos, mass, pts, eps=0.0, skip_self=False, g=G, chunk=256):
    """The theta == 0 kernels' arithmetic restated in numpy, for sizing tolerances only (no test calls it): the pair term in fp32
    operation by operation with a correctly rounded root where the device has a 1-ulp one, a fused multiply-add as an fp64 product
    and sum rounded once to fp32, one chain per `chunk` bodies in body order, the chunks added in fp64, T_aa = S_aa - Q there."""
    f32 = np.float32
    pos = np.asarray(pos, f32); pts = np.asarray(pts, f32)
    gm = (np.asarray(mass, f32) * f32(g)).astype(f32)
    m, n = pts.shape[0], pos.shape[0]
    e2 = f32(float(eps) * float(eps))
    tot = np.zeros((m, 7), np.float64)
    idx = np.arange(m)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)

    for c0 in range(0, n, chunk):
        s = np.zeros((m, 7), f32)
        for j in range(c0, min(c0 + chunk, n)):
            dx, dy, dz = pos[j, 0] - pts[:, 0], pos[j, 1] - pts[:, 1], pos[j, 2] - pts[:, 2]
            w = fma(dz, dz, np.full(m, e2, f32)); w = fma(dy, dy, w); w = fma(dx, dx, w)
            with np.errstate(divide="ignore"):
                t = np.where(w > 0, f32(1) / np.sqrt(np.where(w > 0, w, f32(1))), f32(0)).astype(f32)
            if skip_self:
                t = np.where(idx == j, f32(0), t)
            gg = gm[j] * t; g2 = gg * t
            nx, ny, nz = dx * t, dy * t, dz * t
            h = (g2 * f32(3)) * t
            hx, hy, hz = h * nx, h * ny, h * nz
            s[:, 0] = fma(hx, nx, s[:, 0]); s[:, 3] = fma(hx, ny, s[:, 3]); s[:, 4] = fma(hx, nz, s[:, 4])
            s[:, 1] = fma(hy, ny, s[:, 1]); s[:, 5] = fma(hy, nz, s[:, 5]); s[:, 2] = fma(hz, nz, s[:, 2])
            s[:, 6] = fma(g2, t, s[:, 6])
        tot += s.astype(np.float64)
    out = tot[:, :6].copy()
    out[:, :3] -= tot[:, 6:7]
    return out
