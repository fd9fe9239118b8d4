"""tests/block_tracers_ref.py — the numpy reference of a block session that carries tracers — against the references it is built on,
with the strictly sequential evaluator (seq_field), where a body of mass 0 adds exactly nothing to any sum:
  1. N bodies with M tracers equal, in every byte after every block step, hermite[6]_block_ref's own session of the AUGMENTED system:
     the tracers appended as bodies of mass 0, level_in = the bodies' levels followed by the tracers';
  2. every tracer lands on every frame end;
  3. the bodies' trajectory ignores the tracers."""
import numpy as np
import pytest

from block_tracers_ref import BlockTracers, seq_field
from hermite6_block_ref import Hermite6Block
from hermite_block_ref import HermiteBlock

N, M, LEVELS, DT_MAX = 9, 6, 5, 2.0 ** -3
ETA = {4: 0.02, 6: 0.5}
BODY_FIELDS = {4: ("posm", "vel", "a0", "j0", "a2", "a3", "T", "level"), 6: ("posm", "vel", "a0", "j0", "s0", "a3", "a4", "a5", "T", "level")}


def scene():
    rng = np.random.default_rng(20)
    posm, vel = np.zeros((N, 4)), np.zeros((N, 4))
    posm[:, :3] = rng.normal(0.0, 1.0, (N, 3)); posm[:, 3] = rng.uniform(0.5, 1.5, N) / N
    vel[:, :3] = rng.normal(0.0, 0.3, (N, 3))
    posm[1, :3] = posm[0, :3] + (0.05, 0.0, 0.0)                   # a close pair: deep levels for two bodies and whatever passes by
    return posm, vel, rng.normal(0.0, 1.0, (M, 3)), rng.normal(0.0, 0.3, (M, 3))


def given_levels():
    """The deepest level holds ONLY tracers: the first block step is tracer-only."""
    rng = np.random.default_rng(21)
    lb, lt = rng.integers(0, LEVELS, N), rng.integers(0, LEVELS + 1, M)
    lt[M // 2] = LEVELS
    return lb.astype(np.int32), lt.astype(np.int32)


def augmented_session(order, posm, vel, tpos, tvel, levels):
    m = len(tpos)
    tp, tv = np.zeros((m, 4)), np.zeros((m, 4))
    tp[:, :3], tv[:, :3] = tpos, tvel
    p, v = np.concatenate([posm, tp]), np.concatenate([vel, tv])
    own = np.arange(len(p))
    g = 1.0
    if order == 4:
        return HermiteBlock(p, v, DT_MAX, LEVELS, eta=ETA[4], level_in=levels,
                            evaluate=lambda x, w: seq_field(x, w, None, x, w, None, own, g=g))

    def ev(x, w, a):
        if a is None:
            a = seq_field(x, w, None, x, w, None, own, g=g)[0]
        return seq_field(x, w, a, x, w, a, own, g=g)
    return Hermite6Block(p, v, DT_MAX, LEVELS, eta=ETA[6], level_in=levels, evaluate=ev)


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("order", [4, 6])
@pytest.mark.parametrize("given", [True, False])
def test_the_reference_with_tracers_is_the_reference_of_the_augmented_system(order, given):
    posm, vel, tpos, tvel = scene()
    lb, lt = given_levels() if given else (None, None)
    s = BlockTracers(order, posm, vel, tpos, tvel, DT_MAX, LEVELS, ETA[order], level_in=lb, tracer_level_in=lt, g=1.0)
    aug = augmented_session(order, posm, vel, tpos, tvel, np.concatenate([lb, lt]) if given else None)
    frame = 1 << LEVELS
    while s.ticks < 2 * frame:
        m_b, m_t = s.block_step()
        act = aug.block_step()
        assert (int((act < N).sum()), int((act >= N).sum())) == (m_b, m_t) and aug.ticks == s.ticks
        for f in BODY_FIELDS[order]:
            same(getattr(s.bodies, f), getattr(aug, f)[:N], f"bodies' {f} at tick {s.ticks}")
            same(getattr(s.tracers, f), getattr(aug, f)[N:], f"tracers' {f} at tick {s.ticks}")
    assert s.block_steps == aug.block_steps and s.bodies.body_steps + s.tracers.body_steps == aug.body_steps
    assert s.bodies.floor_hits + s.tracers.floor_hits == aug.floor_hits
    sizes = np.array(s.sizes)
    assert s.tracer_only_steps == int((sizes[:, 0] == 0).sum())
    if given:                                                      # the deepest level holds only tracers; all three kinds of step occur
        assert s.sizes[0][0] == 0 and s.tracer_only_steps >= 1
        assert ((sizes[:, 0] > 0) & (sizes[:, 1] > 0)).any() and (sizes[:, 1] == 0).any()


@pytest.mark.parametrize("order", [4, 6])
def test_every_tracer_lands_on_every_frame_end(order):
    posm, vel, tpos, tvel = scene()
    lb, lt = given_levels()
    s = BlockTracers(order, posm, vel, tpos, tvel, DT_MAX, LEVELS, ETA[order], level_in=lb, tracer_level_in=lt, g=1.0)
    for frame in (1, 2, 3):
        s.advance(1)
        assert s.ticks == frame << LEVELS
        assert (s.tracers.T == s.ticks).all() and (s.bodies.T == s.ticks).all()
    assert s.advance(0) == s.block_steps                           # frames == 0: nothing


@pytest.mark.parametrize("order", [4, 6])
def test_the_bodies_ignore_the_tracers(order):
    posm, vel, tpos, tvel = scene()
    lb, lt = given_levels()
    s = BlockTracers(order, posm, vel, tpos, tvel, DT_MAX, LEVELS, ETA[order], level_in=lb, tracer_level_in=lt, g=1.0)
    alone = augmented_session(order, posm, vel, tpos[:0], tvel[:0], lb)
    s.advance(2); alone.advance(2)
    for f in BODY_FIELDS[order]:
        same(getattr(s.bodies, f), getattr(alone, f), f)
    for f in ("block_steps", "body_steps", "pairs", "floor_hits"):
        assert getattr(s.bodies, f) == getattr(alone, f), f
    assert s.block_steps == alone.block_steps + s.tracer_only_steps
