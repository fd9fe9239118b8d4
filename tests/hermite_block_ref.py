"""The yardstick of nbody_hermite_block_begin / _advance / _get: the Hermite block time steps restated in numpy on hermite_ref's predict,
correct and aarseth_k — every line one correctly rounded fp64 operation per bracket, in the order kernels_hermite_block.hip performs it,
so that a block step computed here from the device's own (a, j) equals the device's in every bit.  `evaluate(posm, vel)` returns the
(a, j) of ALL bodies of a state (the rows of the active ones are taken from it): by default the plain fp64 direct sum, in the GPU tests a
second context's nbody_get_jerk_f64.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import hermite_ref as H
from jerk_ref import G, k_of


def level_of(dt_c, dt_max, levels):
    """(kw, floor_hit) of nbody_hermite_block_level: the smallest k in 0 .. levels with ldexp(dt_max, -k) <= dt_c; none: (levels, True)."""
    for k in range(levels + 1):
        if np.ldexp(np.float64(dt_max), -k) <= dt_c:
            return k, False
    return levels, True


def time_of_k(k):
    """t per body: +inf for k == 0, 0 for a k that is not finite, else 1.0 / sqrt(k)."""
    k = np.asarray(k, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.float64(1.0) / np.sqrt(k)
    return np.where(k == 0.0, np.inf, np.where(np.isfinite(k), t, 0.0))


class HermiteBlock:
    """A block session on the CPU: (posm, vel) with body i at T[i] ticks, its level, the cache (a0, j0, a2, a3) and the totals."""

    def __init__(self, posm, vel, dt_max, levels, eta=0.02, eta_start=0.01, level_in=None, eps=0.0, g=G, evaluate=None, cache=None):
        self.posm = np.array(posm, np.float64); self.vel = np.array(vel, np.float64)
        self.n = len(self.posm)
        self.evaluate = evaluate or (lambda p, v: H.direct(p, v, eps, g))
        self.dt_max, self.L = np.float64(dt_max), int(levels)
        self.tick = np.ldexp(self.dt_max, -self.L)
        self.root_eta = np.sqrt(np.float64(eta))
        self.evaluations = 0
        self.floor_hits = 0
        if cache is None:                                          # one pass at the stored state
            self.a0, self.j0 = (np.array(x) for x in self._eval(self.posm, self.vel))
            self.a2, self.a3 = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        else:                                                      # the shared cache, as a step left it
            self.a0, self.j0, self.a2, self.a3 = (np.array(x, np.float64) for x in cache)
        self.T = np.zeros(self.n, np.int64)
        if level_in is not None:
            self.level = np.array(level_in, np.int32)
            assert self.level.shape == (self.n,) and self.level.min() >= 0 and self.level.max() <= self.L
        else:
            dt_c = np.float64(eta_start) * time_of_k(k_of(self.a0, self.j0))
            self.level = np.zeros(self.n, np.int32)
            for i in range(self.n):
                self.level[i], hit = level_of(dt_c[i], self.dt_max, self.L)
                self.floor_hits += hit
        self.ticks = 0
        self.block_steps = self.body_steps = self.pairs = 0
        self.sizes = []                                            # m of every block step

    def _eval(self, p, v):
        self.evaluations += 1
        return self.evaluate(p, v)

    def steps_in_ticks(self):
        return np.int64(1) << (self.L - self.level).astype(np.int64)

    def block_step(self):
        due = self.T + self.steps_in_ticks()
        t_next = int(due.min())
        act = np.flatnonzero(due == t_next)                        # ascending body index
        dt = ((t_next - self.T).astype(np.float64) * self.tick)[:, None]
        one = lambda d: d[0, 0] if d.size == 1 else d            # (hermite_ref takes a scalar or a column, not a column of one)
        xp, vp = H.predict(self.posm, self.vel, self.a0, self.j0, one(dt))
        a1, j1 = self._eval(xp, vp)
        a1, j1 = a1[act], j1[act]
        p1, w1, a2, a3 = H.correct(self.posm[act], self.vel[act], self.a0[act], self.j0[act], a1, j1, one(dt[act]))
        self.posm[act], self.vel[act] = p1, w1
        self.a0[act], self.j0[act], self.a2[act], self.a3[act] = a1, j1, a2, a3
        self.T[act] = t_next
        dt_c = self.root_eta * time_of_k(H.aarseth_k(a1, j1, a2, a3))
        for q, i in enumerate(act):
            kw, hit = level_of(dt_c[q], self.dt_max, self.L)
            self.floor_hits += hit
            k = int(self.level[i])
            if kw > k:
                self.level[i] = kw
            elif kw < k and t_next % (1 << (self.L - k + 1)) == 0:
                self.level[i] = k - 1
        self.ticks = t_next
        self.block_steps += 1; self.body_steps += len(act); self.pairs += len(act) * self.n
        self.sizes.append(len(act))
        return act

    def advance(self, frames=1, max_block_steps=2 ** 62):
        frame = 1 << self.L
        target = self.ticks if frames == 0 else (self.ticks // frame + frames) * frame
        taken = 0
        while self.ticks < target and taken < max_block_steps:
            self.block_step()
            taken += 1
        return self.stats()

    def stats(self):
        return {"synchronised": self.ticks % (1 << self.L) == 0, "ticks": self.ticks, "frames_done": self.ticks >> self.L,
                "block_steps": self.block_steps, "body_steps": self.body_steps, "pairs": self.pairs, "floor_hits": self.floor_hits,
                "level_min": int(self.level.min()), "level_max": int(self.level.max())}


def binary_in_cluster(posm, vel, offset=(30.0, 20.0, 10.0), a=1.0, e=0.5, g=G):
    """The test scene: bodies 0 and 1 of (posm, vel) replaced by hermite_ref.kepler(e, a = a) of their own masses, the pair's centre of
    mass at `offset` from the origin, at rest."""
    p = np.array(posm, np.float64); v = np.array(vel, np.float64)
    bp, bv, period = H.kepler(e, m1=p[0, 3], m2=p[1, 3], a=a, g=g)
    p[:2, :3] = bp[:, :3] + np.asarray(offset, np.float64)
    v[:2, :3] = bv[:, :3]
    return p, v, period


def energy(posm, vel, eps=0.0, g=G):
    """Kinetic + potential energy in fp64 (a direct sum), for the error of a frame."""
    x, m = posm[:, :3], posm[:, 3]
    ke = 0.5 * float((m * (vel[:, :3] ** 2).sum(1)).sum())
    d = x[:, None, :] - x[None, :, :]
    r = np.sqrt((d ** 2).sum(2) + eps * eps)
    iu = np.triu_indices(len(x), 1)
    pe = -g * float((m[:, None] * m[None, :])[iu].__truediv__(r[iu]).sum())
    return ke + pe
