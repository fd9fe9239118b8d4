"""The yardstick of nbody_hermite[6]_block_begin_tracers: the JOINT schedule of a block session that carries fp64 tracers, restated in
numpy on hermite_block_ref.HermiteBlock and hermite6_block_ref.Hermite6Block — one session of theirs for the bodies, one for the tracers
(bodies of mass 0 that nothing feels), driven together:
  T_next = min over bodies AND tracers of T + step; the bodies' list and the tracers' list, each in ascending index, either may be empty;
  everything is predicted to T_next; the due bodies are evaluated against the predicted bodies and corrected; the due tracers are
  evaluated in the field of the bodies' PREDICTED state (taken before the bodies' corrector wrote the stored one) and corrected by the
  same corrector with their own dt and the same level and alignment rules.
A set nobody of which is due keeps every byte: its session is simply not stepped.  `field(bp, bv, ba, x, v, a, own)` is the pluggable
evaluator: the rows (a, j) — with ba and a given: (a, j, s) — at the points (x, v[, a]) from the bodies (bp, bv[, ba]); own[k] is the
body index point k IS (its own pair is dropped) or -1.  seq_field is the strictly sequential sum.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from hermite6_block_ref import Hermite6Block
from hermite_block_ref import HermiteBlock
from jerk_ref import G
import hermite6_ref as H6
import hermite_ref as H


def seq_field(bp, bv, ba, x, v, a, own, eps=0.0, g=G):
    """Every sum one chain over the bodies in index order, one correctly rounded operation per bracket.  A pair with s2 == 0, and a
    point's own pair, add nothing; a body of mass 0 adds 0 * finite = 0: exactly nothing."""
    k = len(x)
    A, J, S = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, 3))
    snap = ba is not None
    dot = lambda p, q: (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
    for j in range(len(bp)):
        d, w = bp[j, :3] - x[:, :3], bv[j, :3] - v[:, :3]
        s2 = dot(d, d) + eps * eps
        with np.errstate(divide="ignore"):
            t = np.where((s2 > 0.0) & (own != j), 1.0 / np.sqrt(s2), 0.0)
        t2 = t * t
        q = ((g * bp[j, 3]) * t) * t2
        al = dot(d, w) * t2
        u = w - (3.0 * al)[:, None] * d
        A = A + q[:, None] * d
        J = J + q[:, None] * u
        if snap:
            b = ba[j, :3] - a[:, :3]
            be = (dot(w, w) + dot(d, b)) * t2 + al * al
            S = S + q[:, None] * ((b - (6.0 * al)[:, None] * u) - (3.0 * be)[:, None] * d)
    return (A, J, S) if snap else (A, J)


class BlockTracers:
    """order 4 or 6.  .bodies and .tracers are the two sessions; block_steps, tracer_only_steps and sizes ((m_b, m_t) per block step)
    are the joint totals; the bodies' own totals stay in .bodies, the tracers' in .tracers (body_steps there = tracer steps)."""

    def __init__(self, order, posm, vel, tpos, tvel, dt_max, levels, eta, eta_start=0.01, level_in=None, tracer_level_in=None,
                 field=None, eps=0.0, g=G):
        assert order in (4, 6)
        self.order, self.L = order, int(levels)
        self.field = field or (lambda *args: seq_field(*args, eps=eps, g=g))
        m = len(tpos)
        tp, tv = np.zeros((m, 4)), np.zeros((m, 4))
        tp[:, :3], tv[:, :3] = np.asarray(tpos)[:, :3], np.asarray(tvel)[:, :3]
        nobody = np.full(m, -1)
        Session = HermiteBlock if order == 4 else Hermite6Block
        self.bodies = Session(posm, vel, dt_max, levels, eta=eta, eta_start=eta_start, level_in=level_in, evaluate=self._evaluate_bodies)
        self._at = self._stored()                                  # the tracers' start: in the stored bodies' field
        if order == 4:
            ev = lambda p, v: self.field(self._at[0], self._at[1], None, p, v, None, nobody)
        else:
            ev = lambda p, v, a: self._field6(self._at, p, v, a, nobody)
        self.tracers = Session(tp, tv, dt_max, levels, eta=eta, eta_start=eta_start, level_in=tracer_level_in, evaluate=ev)
        self.ticks = self.block_steps = self.tracer_only_steps = 0
        self.sizes = []

    def _stored(self):
        b = self.bodies
        return (b.posm, b.vel, b.a0 if self.order == 6 else None)

    def _field6(self, at, p, v, a, own):
        bp, bv, ba = at
        if a is None:                                              # a start: the points' own accelerations first, then the snap with them
            a = self.field(bp, bv, None, p, v, None, own)[0]
        return self.field(bp, bv, ba, p, v, a, own)

    def _evaluate_bodies(self, p, v, a=None):
        own = np.arange(len(p))
        if self.order == 4:
            return self.field(p, v, None, p, v, None, own)
        if a is None:
            a = self.field(p, v, None, p, v, None, own)[0]
        return self.field(p, v, a, p, v, a, own)

    def _due(self, s):
        return s.T + (np.int64(1) << (self.L - s.level).astype(np.int64))

    def block_step(self):
        b, t = self.bodies, self.tracers
        due_b, due_t = self._due(b), self._due(t)
        t_next = int(min(due_b.min(), due_t.min()))
        m_b, m_t = int((due_b == t_next).sum()), int((due_t == t_next).sum())
        assert m_b + m_t >= 1
        dt = ((t_next - b.T).astype(np.float64) * b.tick)[:, None]
        dt = dt[0, 0] if dt.size == 1 else dt
        if self.order == 4:                                        # the bodies at T_next, before their corrector writes the stored state
            self._at = H.predict(b.posm, b.vel, b.a0, b.j0, dt) + (None,)
        else:
            self._at = H6.predict(b.posm, b.vel, b.a0, b.j0, b.s0, b.a3, dt)
        if m_b:
            assert len(b.block_step()) == m_b and b.ticks == t_next
        if m_t:
            assert len(t.block_step()) == m_t and t.ticks == t_next
        self.ticks = t_next
        self.block_steps += 1
        self.tracer_only_steps += m_b == 0
        self.sizes.append((m_b, m_t))
        return m_b, m_t

    def advance(self, frames=1, max_block_steps=2 ** 62):
        frame = 1 << self.L
        target = self.ticks if frames == 0 else (self.ticks // frame + frames) * frame
        taken = 0
        while self.ticks < target and taken < max_block_steps:
            self.block_step()
            taken += 1
        return self.block_steps
