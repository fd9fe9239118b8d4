"""The yardstick of nbody_get_snap_f64 and of nbody_hermite6_step, nbody_hermite6_timescale and nbody_hermite6_advance: the snap's pair sum in
float64 and np.longdouble, the snap kernel's chunked operation order restated, and Nitadori & Makino's sixth-order shared-step P(EC)
Hermite scheme in numpy, operation by operation as kernels_snap.hip performs it — every line of predict / correct / hermite6_k is one
correctly rounded fp64 operation per bracket, in the order written, so that a step computed here from the device's own (a, j, s) equals
the device's in every bit.  The (a, j, s) themselves come from `evaluate`: by default the plain fp64 direct sum below (for trajectories,
orders and step counts), in the GPU tests a second context's nbody_get_snap_f64.  TEST INFRASTRUCTURE ONLY.

With d = x_j - x_i, w = v_j - v_i, b = acc_j - acc_i (acc: a per-body INPUT array), s^2 = |d|^2 + eps^2, t = 1 / s:
    A_ij = G m_j d t^3        J_ij = G m_j w t^3 - 3 al A_ij        S_ij = G m_j b t^3 - 6 al J_ij - 3 be A_ij
    al = (d . w) t^2          be = (w . w + d . b) t^2 + al^2
With eps == 0 a pair at distance 0 adds nothing to any sum; a body leaves itself out by index."""
import numpy as np

from jerk_ref import G, direct_jerk, jerk_time_of, probe_geometry


def direct_snap(posm, vel, acc_in=None, eps=0.0, dtype=np.float64, g=G, rows=None):
    """(a, j, s) of the bodies, [n,3] each in `dtype` (np.float64 or np.longdouble): the sums of the definition, the body itself left
    out by index.  acc_in None: the bodies' own accelerations in `dtype` — the physical snap of the state.  rows: the bodies to answer
    for (an index array; the results are [len(rows),3]); None: all of them."""
    pos = np.asarray(posm, dtype)[:, :3]; mass = np.asarray(posm, dtype)[:, 3]; v = np.asarray(vel, dtype)[:, :3]
    n = pos.shape[0]
    if acc_in is None:
        acc_in = direct_jerk(pos, mass, v, pos, v, eps=eps, skip_self=True, dtype=dtype, g=g)[0]
    ain = np.asarray(acc_in, dtype)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    m = rows.size
    a = np.empty((m, 3), dtype); j = np.empty((m, 3), dtype); s = np.empty((m, 3), dtype)
    e2 = dtype(eps) * dtype(eps)
    one = dtype(1)
    blk = max(16, min(1024, 500_000 // max(1, n)))
    for lo in range(0, m, blk):
        hi = min(lo + blk, m)
        k = rows[lo:hi]
        d = pos[None, :, :] - pos[k, None, :]
        w = v[None, :, :] - v[k, None, :]
        b = ain[None, :, :] - ain[k, None, :]
        s2 = (d * d).sum(-1) + e2
        ok = s2 > 0
        inv = np.where(ok, one / np.sqrt(np.where(ok, s2, one)), dtype(0))
        inv[np.arange(hi - lo), k] = 0
        t2 = inv * inv
        q = (dtype(g) * mass[None, :] * inv * t2)[:, :, None]      # g m / s^3
        al = ((d * w).sum(-1) * t2)[:, :, None]
        be = ((w * w).sum(-1) + (d * b).sum(-1))[:, :, None] * t2[:, :, None] + al * al
        A = q * d
        J = q * w - dtype(3) * al * A
        S = q * b - dtype(6) * al * J - dtype(3) * be * A
        a[lo:hi] = A.sum(1); j[lo:hi] = J.sum(1); s[lo:hi] = S.sum(1)
    return a, j, s


def emulate_snap_f64(posm, vel, acc_in, eps=0.0, g=G):
    """the fp64 snap kernel's sums (deriv_tile64.h) in the kernel's order: fp64 per pair, the kernel's own sequence of operations, one chain per chunk of
    probe_geometry in body order, the chunks added in chunk order.  Multiplies and adds are numpy's own (no fused multiply-add, a
    correctly rounded root): the ORDER is the kernel's, not its last bit."""
    f64 = np.float64
    pos = np.asarray(posm, f64)[:, :3]; v = np.asarray(vel, f64)[:, :3]; ain = np.asarray(acc_in, f64)
    gm = np.asarray(posm, f64)[:, 3] * f64(g)
    n = pos.shape[0]
    e2 = f64(eps) * f64(eps)
    chunk = probe_geometry(n)[1]
    tot = np.zeros((n, 9), f64)
    idx = np.arange(n)
    for c0 in range(0, n, chunk):
        jx = np.arange(c0, min(c0 + chunk, n))
        d = pos[None, jx, :] - pos[:, None, :]
        w = v[None, jx, :] - v[:, None, :]
        b = ain[None, jx, :] - ain[:, None, :]
        s2 = d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + (d[..., 2] * d[..., 2] + e2))
        ok = (s2 > 0) & (idx[:, None] != jx[None, :])
        t = np.where(ok, 1.0 / np.sqrt(np.where(ok, s2, 1.0)), 0.0)
        t2 = t * t
        q = (gm[None, jx] * t) * t2
        dw = d[..., 0] * w[..., 0] + (d[..., 1] * w[..., 1] + d[..., 2] * w[..., 2])
        k3 = -3.0 * (dw * t2)
        u = k3[..., None] * d + w
        ww = w[..., 0] * w[..., 0] + (w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2])
        db = d[..., 0] * b[..., 0] + (d[..., 1] * b[..., 1] + d[..., 2] * b[..., 2])
        al = dw * t2
        be = al * al + (ww + db) * t2
        k6 = 2.0 * k3
        m3 = -3.0 * be
        gv = m3[..., None] * d + (k6[..., None] * u + b)
        terms = np.concatenate([d, u, gv], axis=2)                # what q multiplies: (d, u, g)
        s = np.zeros((n, 9), f64)
        for col in range(jx.size):                                # the nine chains, in body order
            s = q[:, col, None] * terms[:, col, :] + s
        tot += s
    return tot[:, :3].copy(), tot[:, 3:6].copy(), tot[:, 6:].copy()


def predict(posm, vel, a0, j0, s0, a3, dt):
    """(xp, vp, ap): xp = ((((x + dt v) + c2 a0) + c3 j0) + c4 s0) + c5 a3, vp = (((v + dt a0) + c2 j0) + c3 s0) + c4 a3,
    ap = ((a0 + dt j0) + c2 s0) + c3 a3; xp.w = m, vp.w = 0.  xp, vp are [n,4], ap is [n,3]."""
    dt = np.float64(dt)
    d2 = dt * dt
    c2, c3, c4, c5 = d2 * 0.5, (d2 * dt) / 6.0, (d2 * d2) / 24.0, ((d2 * d2) * dt) / 120.0
    x, v = posm[:, :3], vel[:, :3]
    xp = np.empty_like(posm); vp = np.zeros_like(vel)
    xp[:, :3] = ((((x + dt * v) + c2 * a0) + c3 * j0) + c4 * s0) + c5 * a3
    xp[:, 3] = posm[:, 3]
    vp[:, :3] = (((v + dt * a0) + c2 * j0) + c3 * s0) + c4 * a3
    ap = ((a0 + dt * j0) + c2 * s0) + c3 * a3
    return xp, vp, ap


def correct(posm, vel, a0, j0, s0, a1, j1, s1, dt):
    """(posm1, vel1, a3, a4, a5) from the (a1, j1, s1) of the predicted state: the corrected state — mass and the velocity's fourth
    component as they were — and the third to fifth derivative of a at the new time."""
    dt = np.float64(dt)
    d2 = dt * dt
    ch, c2, c10, c120 = dt * 0.5, d2 * 0.5, d2 / 10.0, (d2 * dt) / 120.0
    d3, d4 = d2 * dt, d2 * d2
    d5 = d4 * dt
    x, v = posm[:, :3], vel[:, :3]
    v1 = v + ((ch * (a0 + a1) + c10 * (j0 - j1)) + c120 * (s0 + s1))
    x1 = x + ((ch * (v + v1) + c10 * (a0 - a1)) + c120 * (j0 + j1))
    R1 = ((a1 - a0) - dt * j0) - c2 * s0
    R2 = dt * ((j1 - j0) - dt * s0)
    R3 = d2 * (s1 - s0)
    X = ((60.0 * R1) - (24.0 * R2)) + (3.0 * R3)
    Y = ((168.0 * R2) - (360.0 * R1)) - (24.0 * R3)
    Z = ((720.0 * R1) - (360.0 * R2)) + (60.0 * R3)
    a3 = ((X + Y) + 0.5 * Z) / d3
    a4 = (Y + Z) / d4
    a5 = Z / d5
    p1 = posm.copy(); w1 = vel.copy()
    p1[:, :3] = x1; w1[:, :3] = v1
    return p1, w1, a3, a4, a5


def norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def hermite6_k(a0, j0, s0, a3, a4, a5):
    """k_i = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2): 0 / 0 counts as 0, x / 0 as +inf, a value that is not finite as +inf."""
    A0, J0, S0, A3, A4, A5 = (norm3(x) for x in (a0, j0, s0, a3, a4, a5))
    num, den = A3 * A5 + A4 * A4, A0 * S0 + J0 * J0
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where((num == 0.0) & (den == 0.0), 0.0, num / den)
    return np.where(np.isfinite(k), k, np.inf)


def timescale(a0, j0, s0, a3=None, a4=None, a5=None):
    """(t_min, body, kind) of nbody_hermite6_timescale: with derivatives kind 1, t = 1 / cbrt(sqrt(max k)); without, kind 0,
    nbody_jerk_time's |a| / |j|.  The largest k, the lowest index that attains it; +inf for k == 0, 0 for a k that is not finite."""
    if a3 is None:
        t, body = jerk_time_of(a0, j0)
        return t, body, 0
    k = hermite6_k(a0, j0, s0, a3, a4, a5)
    body = int(np.argmax(k))
    kmax = float(k[body])
    t = np.inf if kmax == 0.0 else (float(np.float64(1.0) / np.cbrt(np.sqrt(np.float64(kmax)))) if np.isfinite(kmax) else 0.0)
    return t, body, 1


class Hermite6:
    """A context's sixth-order Hermite state on the CPU: (posm, vel), the cache (a0, j0, s0, a3, a4, a5) and the two drivers.
    evaluate(posm, vel, acc_in) returns (a, j, s); acc_in None asks for the physical snap (the state's own accelerations as input)."""

    def __init__(self, posm, vel, eps=0.0, g=G, evaluate=None):
        self.posm = np.array(posm, np.float64); self.vel = np.array(vel, np.float64)
        self.evaluate = evaluate or (lambda p, v, ain: direct_snap(p, v, ain, eps=eps, g=g))
        self.a0 = self.j0 = self.s0 = self.a3 = self.a4 = self.a5 = None
        self.evaluations = 0

    def _eval(self, p, v, ain):
        self.evaluations += 1
        return self.evaluate(p, v, ain)

    def restart(self):
        self.a0 = self.j0 = self.s0 = self.a3 = self.a4 = self.a5 = None

    def enter(self):
        if self.a0 is None:
            self.a0, self.j0, self.s0 = self._eval(self.posm, self.vel, None)

    def step(self, dt, nsteps=1):
        if not dt > 0:
            return
        for _ in range(nsteps):
            self.enter()
            a3 = np.zeros_like(self.a0) if self.a3 is None else self.a3
            xp, vp, ap = predict(self.posm, self.vel, self.a0, self.j0, self.s0, a3, dt)
            a1, j1, s1 = self._eval(xp, vp, ap)
            self.posm, self.vel, self.a3, self.a4, self.a5 = correct(self.posm, self.vel, self.a0, self.j0, self.s0, a1, j1, s1, dt)
            self.a0, self.j0, self.s0 = a1, j1, s1

    def timescale(self):
        self.enter()
        return timescale(self.a0, self.j0, self.s0, self.a3, self.a4, self.a5)

    def advance(self, t_span, eta=0.5, eta_start=0.01, dt_max=np.inf, max_steps=2 ** 31):
        """(t_done, steps, [dt of every step]) of nbody_hermite6_advance: dt = min(dt_max, eta t) — no square root."""
        t_acc, steps, dts = 0.0, 0, []
        while t_acc < t_span and steps < max_steps:
            t, body, kind = self.timescale()
            dt = min(dt_max, eta * t if kind == 1 else eta_start * t)
            rest = t_span - t_acc
            last = dt >= rest
            if last:
                dt = rest
            if not (dt > 0 and np.isfinite(dt)):
                raise FloatingPointError(f"dt = {dt} at body {body}")
            self.step(dt)
            t_acc = t_span if last else t_acc + dt
            steps += 1
            dts.append(dt)
        return t_acc, steps, dts
