"""The yardsticks of nbody_jerk_at, nbody_get_jerk, nbody_get_jerk_f64 and nbody_jerk_time: the plain numpy sum of the definition in
float64 and np.longdouble, and the two kernels' arithmetic restated on the CPU.  TEST INFRASTRUCTURE ONLY.

With d = x_j - x, w = v_j - v, s^2 = |d|^2 + eps^2:
    a(x) = sum_j G m_j d / s^3        j(x, v) = sum_j G m_j [ w / s^3 - 3 (d . w) d / s^5 ]
With eps == 0 a pair at distance 0 adds nothing to either sum."""
import numpy as np

from bh_probe_ref import G


def probe_geometry(n_total):
    """(j_split, j_chunk) of kernels_probe.hip: chunks of whole 256-body tiles, at most 128 of them."""
    chunk = max(1, ((n_total + 127) // 128 + 255) // 256) * 256
    return (n_total + chunk - 1) // chunk, chunk


def direct_jerk(pos, mass, vel, pts, pvel=None, eps=0.0, skip_self=False, dtype=np.float64, g=G):
    """(acc, jerk), [m,3] each in `dtype` (np.float64 or np.longdouble): the sum of the definition over all bodies at the points `pts`
    moving with `pvel` (None: at rest).  skip_self: the points are the bodies themselves and row k leaves body k out by index."""
    pos = np.asarray(pos, dtype); mass = np.asarray(mass, dtype); vel = np.asarray(vel, dtype)[:, :3]
    pts = np.asarray(pts, dtype)
    pvel = np.zeros_like(pts) if pvel is None else np.asarray(pvel, dtype)[:, :3]
    m, n = pts.shape[0], pos.shape[0]
    acc = np.empty((m, 3), dtype); jerk = np.empty((m, 3), dtype)
    e2 = dtype(eps) * dtype(eps)
    one, three = dtype(1), dtype(3)
    blk = max(16, min(1024, 1_000_000 // max(1, n)))
    for a in range(0, m, blk):
        d = pos[None, :, :] - pts[a:a + blk, None, :]
        w = vel[None, :, :] - pvel[a:a + blk, None, :]
        s2 = (d * d).sum(-1) + e2
        ok = s2 > 0
        inv = np.where(ok, one / np.sqrt(np.where(ok, s2, one)), dtype(0))
        if skip_self:
            k = np.arange(a, min(a + blk, m))
            inv[k - a, k] = 0
        q = dtype(g) * mass[None, :] * inv * inv * inv            # g m / s^3
        k3 = three * (d * w).sum(-1) * inv * inv                   # 3 (d . w) / s^2
        acc[a:a + blk] = (q[:, :, None] * d).sum(1)
        jerk[a:a + blk] = (q[:, :, None] * (w - k3[:, :, None] * d)).sum(1)
    return acc, jerk


def rel(got, ref):
    """|got - ref| / |ref| per row; a row whose reference is exactly zero must be exactly zero."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    den = np.linalg.norm(ref, axis=1)
    zero = den == 0.0
    assert not got[zero].any()
    return np.where(zero, 0.0, np.linalg.norm(got - ref, axis=1) / np.where(zero, 1.0, den))


def k_of(acc64, jerk64):
    """k_i = |j_i|^2 / |a_i|^2 as nbody_jerk_time forms it, operation by operation in fp64: 0 / 0 is 0, x / 0 is +inf, not finite is +inf."""
    a = np.asarray(acc64, np.float64); j = np.asarray(jerk64, np.float64)
    a2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    j2 = (j[:, 0] * j[:, 0] + j[:, 1] * j[:, 1]) + j[:, 2] * j[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where((j2 == 0.0) & (a2 == 0.0), 0.0, j2 / a2)
    return np.where(np.isfinite(k), k, np.inf)


def jerk_time_of(acc64, jerk64):
    """(t_min, body) of nbody_jerk_time from the unrounded vectors: the largest k, the lowest index that attains it."""
    k = k_of(acc64, jerk64)
    body = int(np.argmax(k))                                      # (the first of equal maxima)
    kmax = float(k[body])
    with np.errstate(divide="ignore"):
        t = np.inf if kmax == 0.0 else (float(np.float64(1.0) / np.sqrt(np.float64(kmax))) if np.isfinite(kmax) else 0.0)
    return t, body


def emulate_jerk_f32(pos, mass, vel, pts, pvel=None, eps=0.0, skip_self=False, g=G):
    """probe_jerk_pk_kernel's arithmetic restated in numpy, for sizing tolerances: the pair term in fp32 operation by operation — the
    root correctly rounded where the device has a 1-ulp one, a fused multiply-add as an fp64 product and sum rounded once to fp32 —, one
    chain per chunk of probe_geometry in body order, the chunks added in fp64.  Returns (acc, jerk) as float64 [m,3]: the fold's
    unrounded values."""
    f32, f64 = np.float32, np.float64
    pos = np.asarray(pos, f32); pts = np.asarray(pts, f32); vel = np.asarray(vel, f32)[:, :3]
    pvel = np.zeros_like(pts) if pvel is None else np.asarray(pvel, f32)[:, :3]
    gm = (np.asarray(mass, f32) * f32(g)).astype(f32)
    m, n = pts.shape[0], pos.shape[0]
    e2 = f32(float(eps) * float(eps))
    chunk = probe_geometry(n)[1]
    tot = np.zeros((m, 6), f64)
    idx = np.arange(m)

    def fma(a, b, c):
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)

    for c0 in range(0, n, chunk):
        j = np.arange(c0, min(c0 + chunk, n))
        d = pos[None, j, :] - pts[:, None, :]                     # [m, chunk, 3]
        w = vel[None, j, :] - pvel[:, None, :]
        s2 = fma(d[..., 2], d[..., 2], np.full((m, j.size), e2, f32))
        s2 = fma(d[..., 1], d[..., 1], s2)
        s2 = fma(d[..., 0], d[..., 0], s2)
        ok = s2 > 0
        t = np.where(ok, 1.0 / np.sqrt(np.where(ok, s2, f32(1)).astype(f64)), 0.0).astype(f32)
        if skip_self:
            t = np.where(idx[:, None] == j[None, :], f32(0), t)
        gg = gm[None, j] * t; g2 = gg * t; q = g2 * t
        nv = d * t[..., None]
        k = nv[..., 2] * w[..., 2]
        k = fma(nv[..., 1], w[..., 1], k)
        k = fma(nv[..., 0], w[..., 0], k)
        k3 = k * f32(-3)
        u = fma(k3[..., None], nv, w)
        terms = np.concatenate([d, u], axis=2)                    # what q multiplies: (d, u)
        s = np.zeros((m, 6), f32)
        for b in range(j.size):                                   # the six chains, in body order
            s = fma(q[:, b, None], terms[:, b, :], s)
        tot += s.astype(f64)
    return tot[:, :3].copy(), tot[:, 3:].copy()


def emulate_jerk_f64(pos, mass, vel, eps=0.0, g=G):
    """the fp64 jerk kernel's sums (deriv_tile64.h) in the kernel's order, for the bodies themselves: fp64 per pair, one chain per chunk of
    probe_geometry in body order, the chunks added in chunk order.  Multiplies and adds are numpy's own (no fused multiply-add, a
    correctly rounded root): the order of the sums is the kernel's, not its last bit."""
    f64 = np.float64
    pos = np.asarray(pos, f64); vel = np.asarray(vel, f64)[:, :3]
    gm = np.asarray(mass, f64) * f64(g)
    n = pos.shape[0]
    e2 = f64(eps) * f64(eps)
    chunk = probe_geometry(n)[1]
    tot = np.zeros((n, 6), f64)
    idx = np.arange(n)
    for c0 in range(0, n, chunk):
        j = np.arange(c0, min(c0 + chunk, n))
        d = pos[None, j, :] - pos[:, None, :]
        w = vel[None, j, :] - vel[:, None, :]
        s2 = d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + (d[..., 2] * d[..., 2] + e2))
        ok = (s2 > 0) & (idx[:, None] != j[None, :])
        t = np.where(ok, 1.0 / np.sqrt(np.where(ok, s2, 1.0)), 0.0)
        t2 = t * t
        q = (gm[None, j] * t) * t2
        dw = d[..., 0] * w[..., 0] + (d[..., 1] * w[..., 1] + d[..., 2] * w[..., 2])
        k3 = -3.0 * (dw * t2)
        u = k3[..., None] * d + w
        terms = np.concatenate([d, u], axis=2)
        s = np.zeros((n, 6), f64)
        for b in range(j.size):
            s = q[:, b, None] * terms[:, b, :] + s
        tot += s
    return tot[:, :3].copy(), tot[:, 3:].copy()


def probe_velocities(m, seed=11, scale=300.0):
    """Velocities for m probe points: normal, of the shipped scene's scale (its bodies move at 375 on average)."""
    return (np.random.default_rng(seed).normal(0.0, scale, (m, 3))).astype(np.float32)
