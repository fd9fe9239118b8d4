"""The yardstick of nbody_hermite_step, nbody_hermite_timescale and nbody_hermite_advance: Makino & Aarseth's shared-step P(EC) Hermite
scheme restated in numpy, operation by operation as kernels_hermite.hip performs it — every line below is one correctly rounded fp64
operation per bracket, in the order written, so that a step computed here from the device's own (a, j) equals the device's in every
bit.  The (a, j) themselves come from `evaluate`: by default the plain fp64 direct sum of tests/jerk_ref.py (for trajectories, orders
and step counts), in the GPU tests a second context's nbody_get_jerk_f64.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from jerk_ref import G, direct_jerk, jerk_time_of


def direct(posm, vel, eps=0.0, g=G):
    """(a, j) of the bodies, [n,3] float64 each: the definition's sum, the body itself left out by index."""
    return direct_jerk(posm[:, :3], posm[:, 3], vel, posm[:, :3], vel, eps=eps, skip_self=True, g=g)


def predict(posm, vel, a0, j0, dt):
    """(xp, vp), [n,4] each: xp = ((x + c1 v) + c2 a0) + c3 j0, vp = (v + c1 a0) + c2 j0; xp.w = m, vp.w = 0."""
    dt = np.float64(dt)
    c1, c2, c3 = dt, (dt * dt) * 0.5, ((dt * dt) * dt) / 6.0
    x, v = posm[:, :3], vel[:, :3]
    xp = np.empty_like(posm); vp = np.zeros_like(vel)
    xp[:, :3] = ((x + c1 * v) + c2 * a0) + c3 * j0
    xp[:, 3] = posm[:, 3]
    vp[:, :3] = (v + c1 * a0) + c2 * j0
    return xp, vp


def correct(posm, vel, a0, j0, a1, j1, dt):
    """(posm1, vel1, a2, a3) from the (a1, j1) of the predicted state: the corrected state — mass and the velocity's fourth component as
    they were — and the second and third derivative of a at the new time."""
    dt = np.float64(dt)
    ch, c12, d2, d3 = dt * 0.5, (dt * dt) / 12.0, dt * dt, (dt * dt) * dt
    x, v = posm[:, :3], vel[:, :3]
    v1 = v + (ch * (a0 + a1) + c12 * (j0 - j1))
    x1 = x + (ch * (v + v1) + c12 * (a0 - a1))
    da = a0 - a1
    a2_0 = ((-6.0 * da) - dt * ((4.0 * j0) + (2.0 * j1))) / d2
    a3 = ((12.0 * da) + (6.0 * dt) * (j0 + j1)) / d3
    a2_1 = a2_0 + dt * a3
    p1 = posm.copy(); w1 = vel.copy()
    p1[:, :3] = x1; w1[:, :3] = v1
    return p1, w1, a2_1, a3


def norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def aarseth_k(a0, j0, a2, a3):
    """k_i = (J C + S S) / (A S + J J): 0 / 0 counts as 0, x / 0 as +inf, a value that is not finite as +inf."""
    A, J, S, C = norm3(a0), norm3(j0), norm3(a2), norm3(a3)
    num, den = J * C + S * S, A * S + J * J
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where((num == 0.0) & (den == 0.0), 0.0, num / den)
    return np.where(np.isfinite(k), k, np.inf)


def timescale(a0, j0, a2=None, a3=None):
    """(t_min, body, kind) of nbody_hermite_timescale: with derivatives kind 1, Aarseth's criterion; without, kind 0, nbody_jerk_time's
    |a| / |j|.  The largest k, the lowest index that attains it; t = 1 / sqrt(k), +inf for k == 0, 0 for a k that is not finite."""
    if a2 is None:
        t, body = jerk_time_of(a0, j0)
        return t, body, 0
    k = aarseth_k(a0, j0, a2, a3)
    body = int(np.argmax(k))
    kmax = float(k[body])
    t = np.inf if kmax == 0.0 else (float(np.float64(1.0) / np.sqrt(np.float64(kmax))) if np.isfinite(kmax) else 0.0)
    return t, body, 1


class Hermite:
    """A context's Hermite state on the CPU: (posm, vel), the cache (a0, j0, a2, a3) and the two drivers."""

    def __init__(self, posm, vel, eps=0.0, g=G, evaluate=None):
        self.posm = np.array(posm, np.float64); self.vel = np.array(vel, np.float64)
        self.evaluate = evaluate or (lambda p, v: direct(p, v, eps, g))
        self.a0 = self.j0 = self.a2 = self.a3 = None
        self.evaluations = 0

    def _eval(self, p, v):
        self.evaluations += 1
        return self.evaluate(p, v)

    def restart(self):
        self.a0 = self.j0 = self.a2 = self.a3 = None

    def enter(self):
        if self.a0 is None:
            self.a0, self.j0 = self._eval(self.posm, self.vel)

    def step(self, dt, nsteps=1):
        if not dt > 0:
            return
        for _ in range(nsteps):
            self.enter()
            xp, vp = predict(self.posm, self.vel, self.a0, self.j0, dt)
            a1, j1 = self._eval(xp, vp)
            self.posm, self.vel, self.a2, self.a3 = correct(self.posm, self.vel, self.a0, self.j0, a1, j1, dt)
            self.a0, self.j0 = a1, j1

    def timescale(self):
        self.enter()
        return timescale(self.a0, self.j0, self.a2, self.a3)

    def advance(self, t_span, eta=0.02, eta_start=0.01, dt_max=np.inf, max_steps=2 ** 31):
        """(t_done, steps, [dt of every step]) of nbody_hermite_advance."""
        t_acc, steps, dts = 0.0, 0, []
        root_eta = float(np.sqrt(np.float64(eta)))
        while t_acc < t_span and steps < max_steps:
            t, body, kind = self.timescale()
            dt = min(dt_max, root_eta * t if kind == 1 else eta_start * t)
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


def kick_drift(posm, vel, dt, nsteps, eps=0.0, g=G):
    """The engine's own nbody_step in fp64: v += dt a; x += dt v."""
    p = np.array(posm, np.float64); v = np.array(vel, np.float64)
    for _ in range(nsteps):
        a, _ = direct(p, v, eps, g)
        v[:, :3] = v[:, :3] + dt * a
        p[:, :3] = p[:, :3] + dt * v[:, :3]
    return p, v


def kepler(e, m1=1000.0, m2=3000.0, a=100.0, g=G):
    """(posm, vel, period): two bodies on a Kepler orbit of eccentricity e and semi-major axis a in the x-y plane, at pericentre, the
    centre of mass at rest on the origin."""
    M = m1 + m2
    rp = a * (1.0 - e)
    vp = np.sqrt(g * M * (1.0 + e) / (a * (1.0 - e)))
    posm = np.zeros((2, 4)); vel = np.zeros((2, 4))
    posm[0] = [-rp * m2 / M, 0.0, 0.0, m1]
    posm[1] = [rp * m1 / M, 0.0, 0.0, m2]
    vel[0, 1] = -vp * m2 / M
    vel[1, 1] = vp * m1 / M
    return posm, vel, float(2.0 * np.pi * np.sqrt(a ** 3 / (g * M)))
