"""The yardstick of the fp64 tracers (nbody_set_tracers_f64) and of nbody_jerk_at_f64: the shared-step Hermite drivers of
tests/hermite_ref.py and tests/hermite6_ref.py carrying massless points beside the bodies, as include/nbody.h states it — the tracers are
predicted with the step's dt, evaluated in the field of the bodies' PREDICTED state, corrected by the bodies' corrector, and nothing of
theirs enters anything the bodies get.  Predictor and corrector are hermite_ref's / hermite6_ref's own functions (one correctly rounded
fp64 operation per bracket), applied to the tracers' arrays.  The point evaluator is pluggable: by default the plain direct sums below
(no pair is dropped by index: a point is nobody), in a GPU test it may be a context's jerk_at_f64.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import hermite6_ref as H6
import hermite_ref as H
from jerk_ref import G, direct_jerk


def point_jerk(posm, vel, pts, pvel, eps=0.0, dtype=np.float64, g=G):
    """(a, j) at the points `pts` moving with `pvel` from ALL bodies: [m,3] each in `dtype`."""
    return direct_jerk(posm[:, :3], posm[:, 3], vel, pts, pvel, eps=eps, skip_self=False, dtype=dtype, g=g)


def point_snap(posm, vel, acc_in, pts, pvel, pacc, eps=0.0, dtype=np.float64, g=G):
    """(a, j, s) at the points from ALL bodies, given the bodies' input accelerations acc_in and the points' pacc: the sums of
    hermite6_ref.direct_snap with the i side taken from the points and no pair dropped by index."""
    pos = np.asarray(posm, dtype)[:, :3]; mass = np.asarray(posm, dtype)[:, 3]; v = np.asarray(vel, dtype)[:, :3]
    ain = np.asarray(acc_in, dtype)
    x = np.asarray(pts, dtype)[:, :3]; xv = np.asarray(pvel, dtype)[:, :3]; xa = np.asarray(pacc, dtype)[:, :3]
    m, n = x.shape[0], pos.shape[0]
    a = np.empty((m, 3), dtype); j = np.empty((m, 3), dtype); s = np.empty((m, 3), dtype)
    e2 = dtype(eps) * dtype(eps)
    one = dtype(1)
    blk = max(16, min(1024, 500_000 // max(1, n)))
    for lo in range(0, m, blk):
        hi = min(lo + blk, m)
        d = pos[None, :, :] - x[lo:hi, None, :]
        w = v[None, :, :] - xv[lo:hi, None, :]
        b = ain[None, :, :] - xa[lo:hi, None, :]
        s2 = (d * d).sum(-1) + e2
        ok = s2 > 0
        inv = np.where(ok, one / np.sqrt(np.where(ok, s2, one)), dtype(0))
        t2 = inv * inv
        q = (dtype(g) * mass[None, :] * inv * t2)[:, :, None]
        al = ((d * w).sum(-1) * t2)[:, :, None]
        be = ((w * w).sum(-1) + (d * b).sum(-1))[:, :, None] * t2[:, :, None] + al * al
        A = q * d
        J = q * w - dtype(3) * al * A
        S = q * b - dtype(6) * al * J - dtype(3) * be * A
        a[lo:hi] = A.sum(1); j[lo:hi] = J.sum(1); s[lo:hi] = S.sum(1)
    return a, j, s


def four(a):
    """[m,3] -> [m,4] with a fourth column of zeros (a tracer has no mass; a velocity's fourth component is 0)."""
    a = np.asarray(a, np.float64)
    out = np.zeros((a.shape[0], 4))
    out[:, :3] = a[:, :3]
    return out


class Hermite(H.Hermite):
    """hermite_ref.Hermite with tracers: (tpos, tvel) [m,4], their cache (ta0, tj0, ta2, ta3).  points(posm, vel, pts, pvel) -> (a, j)."""

    def __init__(self, posm, vel, tpos, tvel=None, eps=0.0, g=G, evaluate=None, points=None):
        super().__init__(posm, vel, eps=eps, g=g, evaluate=evaluate)
        self.tpos = four(tpos); self.tvel = four(np.zeros_like(self.tpos) if tvel is None else tvel)
        self.points = points or (lambda p, v, x, xv: point_jerk(p, v, x[:, :3], xv[:, :3], eps=eps, g=g))
        self.ta0 = self.tj0 = self.ta2 = self.ta3 = None
        self.point_evaluations = 0

    def _points(self, p, v, x, xv):
        self.point_evaluations += 1
        return self.points(p, v, x, xv)

    def restart(self):
        super().restart()
        self.ta0 = self.tj0 = self.ta2 = self.ta3 = None

    def enter(self):
        super().enter()
        if self.ta0 is None:
            self.ta0, self.tj0 = self._points(self.posm, self.vel, self.tpos, self.tvel)

    def step(self, dt, nsteps=1):
        if not dt > 0:
            return
        for _ in range(nsteps):
            self.enter()
            xp, vp = H.predict(self.posm, self.vel, self.a0, self.j0, dt)
            txp, tvp = H.predict(self.tpos, self.tvel, self.ta0, self.tj0, dt)
            a1, j1 = self._eval(xp, vp)
            ta1, tj1 = self._points(xp, vp, txp, tvp)               # the field the bodies' own evaluation uses
            self.posm, self.vel, self.a2, self.a3 = H.correct(self.posm, self.vel, self.a0, self.j0, a1, j1, dt)
            self.tpos, self.tvel, self.ta2, self.ta3 = H.correct(self.tpos, self.tvel, self.ta0, self.tj0, ta1, tj1, dt)
            self.a0, self.j0 = a1, j1
            self.ta0, self.tj0 = ta1, tj1

    def tracers_timescale(self):
        self.enter()
        return H.timescale(self.ta0, self.tj0, self.ta2, self.ta3)


class Hermite6(H6.Hermite6):
    """hermite6_ref.Hermite6 with tracers.  points(posm, vel, acc_in, pts, pvel, pacc) -> (a, j, s); at a start the tracers' input
    acceleration is the point jerk sum's a (points_jerk(posm, vel, pts, pvel) -> (a, j)) and the bodies' is their cached a0."""

    def __init__(self, posm, vel, tpos, tvel=None, eps=0.0, g=G, evaluate=None, points=None, points_jerk=None):
        super().__init__(posm, vel, eps=eps, g=g, evaluate=evaluate)
        self.tpos = four(tpos); self.tvel = four(np.zeros_like(self.tpos) if tvel is None else tvel)
        self.points = points or (lambda p, v, ain, x, xv, xa: point_snap(p, v, ain, x, xv, xa, eps=eps, g=g))
        self.points_jerk = points_jerk or (lambda p, v, x, xv: point_jerk(p, v, x[:, :3], xv[:, :3], eps=eps, g=g))
        self.ta0 = self.tj0 = self.ts0 = self.ta3 = self.ta4 = self.ta5 = None
        self.point_evaluations = 0

    def restart(self):
        super().restart()
        self.ta0 = self.tj0 = self.ts0 = self.ta3 = self.ta4 = self.ta5 = None

    def enter(self):
        super().enter()
        if self.ta0 is None:
            ta = self.points_jerk(self.posm, self.vel, self.tpos, self.tvel)[0]
            self.ta0, self.tj0, self.ts0 = self.points(self.posm, self.vel, self.a0, self.tpos, self.tvel, ta)
            self.point_evaluations += 2

    def step(self, dt, nsteps=1):
        if not dt > 0:
            return
        for _ in range(nsteps):
            self.enter()
            a3 = np.zeros_like(self.a0) if self.a3 is None else self.a3
            ta3 = np.zeros_like(self.ta0) if self.ta3 is None else self.ta3
            xp, vp, ap = H6.predict(self.posm, self.vel, self.a0, self.j0, self.s0, a3, dt)
            txp, tvp, tap = H6.predict(self.tpos, self.tvel, self.ta0, self.tj0, self.ts0, ta3, dt)
            a1, j1, s1 = self._eval(xp, vp, ap)
            ta1, tj1, ts1 = self.points(xp, vp, ap, txp, tvp, tap)
            self.point_evaluations += 1
            self.posm, self.vel, self.a3, self.a4, self.a5 = H6.correct(self.posm, self.vel, self.a0, self.j0, self.s0, a1, j1, s1, dt)
            self.tpos, self.tvel, self.ta3, self.ta4, self.ta5 = H6.correct(self.tpos, self.tvel, self.ta0, self.tj0, self.ts0, ta1, tj1, ts1, dt)
            self.a0, self.j0, self.s0 = a1, j1, s1
            self.ta0, self.tj0, self.ts0 = ta1, tj1, ts1

    def tracers_timescale(self):
        self.enter()
        return H6.timescale(self.ta0, self.tj0, self.ts0, self.ta3, self.ta4, self.ta5)


def circular_tracer(mass=4000.0, r=100.0, g=G):
    """(posm, vel, tpos, tvel, period): ONE body at rest on the origin (it feels nothing and stays) and a tracer on the circular orbit
    of radius r round it, in the x-y plane — hermite_ref.kepler(0)'s relative orbit (M = 4000, a = 100)."""
    posm = np.array([[0.0, 0.0, 0.0, mass]]); vel = np.zeros((1, 4))
    vc = np.sqrt(g * mass / r)
    tpos = np.array([[r, 0.0, 0.0]]); tvel = np.array([[0.0, vc, 0.0]])
    return posm, vel, tpos, tvel, float(2.0 * np.pi * np.sqrt(r ** 3 / (g * mass)))
