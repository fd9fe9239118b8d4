"""The yardstick of nbody_hermite6_block_begin / _advance / _get: the sixth-order Hermite block time steps restated in numpy on
hermite6_ref's predict, correct and hermite6_k and hermite_block_ref's times and levels — every line one correctly rounded fp64 operation
per bracket, in the order kernels_hermite6_block.hip performs it, so that a block step computed here from the device's own (a, j, s)
equals the device's in every bit.  `evaluate(posm, vel, acc_in)` returns the (a, j, s) of ALL bodies of a state (the rows of the active
ones are taken from it); acc_in None asks for the physical snap (the start).  By default the plain fp64 direct sum, in the GPU tests a
second context's snap(acc_in).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import hermite6_ref as H6
from hermite_block_ref import level_of, time_of_k
from jerk_ref import G, k_of


def level6_of(kk, dt_max, levels, eta):
    """(kw, floor_hit) of nbody_hermite6_block_level: r = sqrt(kk), e3 = (eta eta) eta; the smallest k in 0 .. levels with
    ((h h) h) r <= e3, h = ldexp(dt_max, -k); none: (levels, True).  No cube root anywhere."""
    kk, eta = np.float64(kk), np.float64(eta)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r = np.sqrt(kk)
        e3 = (eta * eta) * eta
        for k in range(levels + 1):
            h = np.ldexp(np.float64(dt_max), -k)
            if ((h * h) * h) * r <= e3:
                return k, False
    return levels, True


class Hermite6Block:
    """A sixth-order block session on the CPU: (posm, vel) with body i at T[i] ticks, its level, the cache (a0, j0, s0, a3, a4, a5) and
    the totals.  cache: the six arrays a shared step left; None: the start (one evaluation with acc_in None, a3 = a4 = a5 = 0)."""

    def __init__(self, posm, vel, dt_max, levels, eta=0.5, eta_start=0.01, level_in=None, eps=0.0, g=G, evaluate=None, cache=None):
        self.posm = np.array(posm, np.float64); self.vel = np.array(vel, np.float64)
        self.n = len(self.posm)
        self.evaluate = evaluate or (lambda p, v, ain: H6.direct_snap(p, v, ain, eps=eps, g=g))
        self.dt_max, self.L = np.float64(dt_max), int(levels)
        self.tick = np.ldexp(self.dt_max, -self.L)
        self.eta = np.float64(eta)
        self.evaluations = 0
        self.floor_hits = 0
        if cache is None:
            self.a0, self.j0, self.s0 = (np.array(x) for x in self._eval(self.posm, self.vel, None))
            self.a3, self.a4, self.a5 = (np.zeros((self.n, 3)) for _ in range(3))
        else:
            self.a0, self.j0, self.s0, self.a3, self.a4, self.a5 = (np.array(x, np.float64) for x in cache)
        self.T = np.zeros(self.n, np.int64)
        if level_in is not None:
            self.level = np.array(level_in, np.int32)
            assert self.level.shape == (self.n,) and self.level.min() >= 0 and self.level.max() <= self.L
        else:                                                      # the fourth-order begin's start rule on (a0, j0)
            dt_c = np.float64(eta_start) * time_of_k(k_of(self.a0, self.j0))
            self.level = np.zeros(self.n, np.int32)
            for i in range(self.n):
                self.level[i], hit = level_of(dt_c[i], self.dt_max, self.L)
                self.floor_hits += hit
        self.ticks = 0
        self.block_steps = self.body_steps = self.pairs = 0
        self.sizes = []                                            # m of every block step

    def _eval(self, p, v, ain):
        self.evaluations += 1
        return self.evaluate(p, v, ain)

    def block_step(self):
        due = self.T + (np.int64(1) << (self.L - self.level).astype(np.int64))
        t_next = int(due.min())
        act = np.flatnonzero(due == t_next)                        # ascending body index
        dt = ((t_next - self.T).astype(np.float64) * self.tick)[:, None]
        one = lambda d: d[0, 0] if d.size == 1 else d            # (hermite6_ref takes a scalar or a column, not a column of one)
        xp, vp, ap = H6.predict(self.posm, self.vel, self.a0, self.j0, self.s0, self.a3, one(dt))
        a1, j1, s1 = self._eval(xp, vp, ap)
        a1, j1, s1 = a1[act], j1[act], s1[act]
        p1, w1, a3, a4, a5 = H6.correct(self.posm[act], self.vel[act], self.a0[act], self.j0[act], self.s0[act], a1, j1, s1, one(dt[act]))
        self.posm[act], self.vel[act] = p1, w1
        self.a0[act], self.j0[act], self.s0[act], self.a3[act], self.a4[act], self.a5[act] = a1, j1, s1, a3, a4, a5
        self.T[act] = t_next
        kk = H6.hermite6_k(a1, j1, s1, a3, a4, a5)
        for q, i in enumerate(act):
            kw, hit = level6_of(kk[q], self.dt_max, self.L, self.eta)
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
