"""Hermite block time steps — nbody_hermite_block_begin, nbody_hermite_block_advance, nbody_hermite_block_get — against
tests/hermite_block_ref.py, the scheme restated in numpy (tests/test_hermite_block_ref.py pins that yardstick and the level rule on the
CPU).

The evaluation of a block step is, for every active body, what nbody_get_jerk_f64 returns for that body on a context holding the
predicted state, and everything around it is correctly rounded fp64 arithmetic in a documented order.  So EVERY comparison here is byte
for byte, after every block step (max_block_steps = 1): a second fp64 context is loaded with numpy's predicted state, its
jerk(np.float64) supplies all rows, numpy takes those of the active bodies and its corrector and level rule give every bit the stepping
context must hold — positions, velocities, stored accelerations, a0, j0, a2, a3, the bodies' times and levels, the totals.

Scenes: the Plummer spheres of tests/test_hermite_gpu.py with bodies 0 and 1 made a hard binary (hermite_block_ref.binary_in_cluster).
N = 257 is a full tile and a ragged one; N = 1025 is five j-chunks of 256 bodies, and an active set of 1025 is three workgroups of two
bodies per lane, the last one body deep, one of 513 three workgroups of one body per lane, the last one body deep."""
import ctypes

import numpy as np
import pytest

import hermite_block_ref as B
import hermite_ref as H
import test_hermite_gpu as T
from test_hermite_gpu import evaluator, f64, fake_rccl, raises, scene  # noqa: F401  (fake_rccl is a fixture)

pytestmark = pytest.mark.gpu

DT_MAX, LEVELS, ETA = 0.01, 12, 0.02
NAMES = T.NAMES + ("times", "levels")
_scenes = {}


def binary_scene(nb, n):
    if n not in _scenes:
        p, v, _ = B.binary_in_cluster(*scene(nb, n))
        p.setflags(write=False); v.setflags(write=False)
        _scenes[n] = (p, v)
    return _scenes[n]


def snapshot(e):
    """Everything a block step writes, as bytes: the state, the cache, the bodies' times and levels."""
    return T.snapshot(e) + tuple(x.tobytes() for x in e.hermite_block_state())


class Yardstick:
    """hermite_block_ref.HermiteBlock beside a context in session, with the stored accelerations carried along: NBODY_BUF_ACC is (a1, 0)
    for a body that has stepped and what the context held at begin for one that has not."""

    def __init__(self, e, other, posm, vel, dt_max, levels, **kw):
        self.ref = B.HermiteBlock(posm, vel, dt_max, levels, evaluate=evaluator(other), **kw)
        self.acc = e.state(np.float64)[2].copy()

    def block_step(self):
        act = self.ref.block_step()
        self.acc[act, :3] = self.ref.a0[act]
        self.acc[act, 3] = 0.0
        return act

    def expected(self):
        r = self.ref
        return (r.posm.tobytes(), r.vel.tobytes(), self.acc.tobytes(), r.a0.tobytes(), r.j0.tobytes(), r.a2.tobytes(), r.a3.tobytes(),
                r.T.tobytes(), r.level.tobytes())


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g == w, f"{what}: {name} differ"


def step_and_compare(e, y, what):
    stats = e.hermite_block_advance(1, max_block_steps=1)
    act = y.block_step()
    same(snapshot(e), y.expected(), what)
    assert stats == y.ref.stats(), what
    return act


# ---- 1: a criterion-driven run, every block step ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,eps,steps", [(257, 0.0, None), (257, 0.05, None), (1025, 0.0, 24)])
def test_every_block_step_in_every_bit(nb, n, eps, steps):
    posm, vel = binary_scene(nb, n)
    with f64(nb, n, eps=eps) as a, f64(nb, n, eps=eps) as b, f64(nb, n, eps=eps) as whole:
        a.set_state(posm, vel)
        a.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
        y = Yardstick(a, b, posm, vel, DT_MAX, LEVELS, eta=ETA)
        same(snapshot(a), y.expected(), f"N={n} eps={eps} begin")
        assert len(np.unique(y.ref.level)) >= 4 and y.ref.floor_hits == 0
        taken = 0
        while (taken < steps) if steps else (y.ref.ticks < 1 << LEVELS):
            step_and_compare(a, y, f"N={n} eps={eps} block step {taken + 1}")
            taken += 1
            assert a.steps_done() == taken
        sizes = y.ref.sizes
        print(f"N={n} eps={eps}: {taken} block steps, active sets {min(sizes)} .. {max(sizes)}, levels {np.bincount(y.ref.level)}")
        assert min(sizes) <= 2 and y.ref.evaluations == taken + 1
        if steps is None:                                          # the whole frame: in one call on a third context, the same bytes
            assert max(sizes) == n and y.ref.stats()["synchronised"] and y.ref.floor_hits == 0
            whole.set_state(posm, vel)
            whole.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
            stats = whole.hermite_block_advance(1)
            same(snapshot(whole), y.expected(), f"N={n} eps={eps} one frame in one call")
            assert stats == y.ref.stats() and whole.steps_done() == taken
            assert whole.hermite_block_advance(0) == stats         # frames == 0: nothing moves
            same(snapshot(whole), y.expected(), "frames == 0")


# ---- 2: the shapes the gather can get wrong ---------------------------------------------------------------------------------------------------

SETS = {"last": lambda n: [n - 1], "first257": lambda n: range(257), "every_other": lambda n: range(0, n, 2), "all": lambda n: range(n)}


@pytest.mark.parametrize("lanes", [None, "1", "2"])
@pytest.mark.parametrize("which", list(SETS))
def test_one_block_step_of_a_given_active_set(nb, monkeypatch, which, lanes):
    n = 1025
    if lanes is None:
        monkeypatch.delenv("NBODY_HERMITE_BLOCK_LANES", raising=False)
    else:
        monkeypatch.setenv("NBODY_HERMITE_BLOCK_LANES", lanes)     # bodies per lane of the evaluation, either way for every set
    posm, vel = binary_scene(nb, n)
    members = np.array(list(SETS[which](n)))
    level_in = np.zeros(n, np.int32)
    level_in[members] = 1                                          # everything at level 0 except the set: it alone is due at tick 1
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite_block_begin(DT_MAX, 1, eta=ETA, level_in=level_in)
        y = Yardstick(a, b, posm, vel, DT_MAX, 1, eta=ETA, level_in=level_in)
        same(snapshot(a), y.expected(), f"{which} begin")
        act = step_and_compare(a, y, f"{which} lanes={lanes}")
        assert act.tolist() == members.tolist() and a.hermite_block_advance(0)["body_steps"] == len(members)
        others = np.setdiff1d(np.arange(n), members)
        p, v, _ = a.state(np.float64)
        assert p[others].tobytes() == posm[others].tobytes() and v[others].tobytes() == vel[others].tobytes()
        if which == "all":                                         # m = N: the shared step of dt_max / 2
            b.set_state(posm, vel)
            b.hermite_step(DT_MAX / 2, 1)
            same(snapshot(a)[:7], T.snapshot(b), "m = N against nbody_hermite_step")


# ---- 3: the degenerate case ---------------------------------------------------------------------------------------------------------------

def test_levels_zero_is_the_shared_step(nb):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite_block_begin(DT_MAX, 0, eta=ETA)
        stats = a.hermite_block_advance(3)
        b.set_state(posm, vel)
        b.hermite_step(DT_MAX, 3)
        same(snapshot(a)[:7], T.snapshot(b), "three block steps at levels = 0 against nbody_hermite_step(dt_max, 3)")
        assert (stats["block_steps"], stats["frames_done"], stats["body_steps"], stats["ticks"]) == (3, 3, 3 * n, 3)
        assert a.steps_done() == b.steps_done() == 3


# ---- 4: floor hits ----------------------------------------------------------------------------------------------------------------------------

def test_floor_hits_are_clamped_and_counted(nb):
    n, levels = 257, 2                                             # the binary wants level 5 and deeper
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite_block_begin(DT_MAX, levels, eta=ETA)
        y = Yardstick(a, b, posm, vel, DT_MAX, levels, eta=ETA)
        at_begin = y.ref.floor_hits
        assert at_begin >= 2 and a.hermite_block_advance(0)["floor_hits"] == at_begin
        while y.ref.ticks < 1 << levels:
            step_and_compare(a, y, f"levels = {levels}, block step {y.ref.block_steps + 1}")
        stats = a.hermite_block_advance(0)
        print(f"floor hits {stats['floor_hits']} ({at_begin} at begin) in {stats['block_steps']} block steps")
        assert stats["floor_hits"] == y.ref.floor_hits > at_begin and stats["level_max"] == levels


# ---- 5: accounting ----------------------------------------------------------------------------------------------------------------------------

def test_one_forces_pass_and_one_update_pass_per_block_step(nb):
    n = 257
    posm, vel = binary_scene(nb, n)
    F, U = nb._lib.KERNEL_FORCES, nb._lib.KERNEL_UPDATE
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0, u0 = e.kernel_time(F)[1], e.kernel_time(U)[1]
        e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
        assert (e.kernel_time(F)[1] - f0, e.kernel_time(U)[1] - u0) == (1, 0)      # begin evaluates (a0, j0): the cache was not valid
        stats = e.hermite_block_advance(1, max_block_steps=7)
        f1, u1 = e.kernel_time(F)[1], e.kernel_time(U)[1]
        assert stats["block_steps"] == 7 and (f1 - f0, u1 - u0) == (8, 7)
        stats = e.hermite_block_advance(1)
        k = stats["block_steps"]
        assert stats["synchronised"] and (e.kernel_time(F)[1] - f0, e.kernel_time(U)[1] - u0) == (k + 1, k)
        assert stats["pairs"] == stats["body_steps"] * n and stats["body_steps"] < k * n and e.steps_done() == k
        assert e.kernel_time(F)[0] > 0 and e.kernel_time(U)[0] > 0
        e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)             # a new session on the valid cache: no pass
        assert e.kernel_time(F)[1] - f0 == k + 1
        assert e.hermite_block_advance(0)["block_steps"] == 0 and e.steps_done() == k


# ---- 6: session rules ---------------------------------------------------------------------------------------------------------------------------

def three_calls(e):
    return (lambda: e.hermite_block_begin(DT_MAX, LEVELS)), (lambda: e.hermite_block_advance(1)), e.hermite_block_state


def test_errors(nb, fake_rccl, monkeypatch):  # noqa: F811
    monkeypatch.setenv("NBODY_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("NBODY_MULTI_SHARE_DEVICE", "1")
    E = nb._lib
    big = 2000
    p32, v32 = nb.ic_reference_box(big, 1000.0, seed=1)
    for kw, why in (({}, "fp32"), ({"precision": "f32_kahan"}, "fp32"), ({"precision": "f64", "i_begin": 0, "i_count": 1000}, "slice"),
                    ({"devices": [0]}, "multi-device")):
        with nb.NBodyEngine(big, **kw) as e:
            if kw.get("precision") == "f64":
                e.set_state(p32.astype(np.float64), v32.astype(np.float64))
            else:
                e.set_state(p32, v32)
            for call in three_calls(e):
                assert why in raises(nb, E.ERR_UNSUPPORTED, call), kw
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as e:
        for call in three_calls(e):                                # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(posm, vel)
        for call in three_calls(e)[1:]:                            # no session
            assert "nbody_hermite_block_begin" in raises(nb, E.ERR_STATE, call)
        before = T.snapshot_state(e)
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            raises(nb, E.ERR_INVALID, lambda: e.hermite_block_begin(bad, LEVELS))
            raises(nb, E.ERR_INVALID, lambda: e.hermite_block_begin(DT_MAX, LEVELS, eta=bad))
            raises(nb, E.ERR_INVALID, lambda: e.hermite_block_begin(DT_MAX, LEVELS, eta_start=bad))
        for levels in (-1, 41):
            raises(nb, E.ERR_INVALID, lambda: e.hermite_block_begin(DT_MAX, levels))
        assert "normal" in raises(nb, E.ERR_INVALID, lambda: e.hermite_block_begin(1e-300, 40))
        for lv in (np.full(n, LEVELS + 1), np.r_[np.zeros(n - 1), -1]):
            assert "level_in" in raises(nb, E.ERR_INVALID, lambda: e.hermite_block_begin(DT_MAX, LEVELS, level_in=lv))
        for call in three_calls(e)[1:]:                            # none of those began a session
            raises(nb, E.ERR_STATE, call)
        e.hermite_block_begin(DT_MAX, LEVELS)
        raises(nb, E.ERR_INVALID, lambda: e.hermite_block_advance(-1))
        raises(nb, E.ERR_INVALID, lambda: e.hermite_block_advance(1, max_block_steps=-1))
        raises(nb, E.ERR_INVALID, lambda: e.hermite_block_advance(2 ** 62))
        st = E.HermiteBlockStats()
        st.struct_size = ctypes.sizeof(st) - 8
        assert e._L.nbody_hermite_block_advance(e._h, 1, 1, ctypes.byref(st)) == E.ERR_INVALID
        assert e._L.nbody_hermite_block_advance(e._h, 0, 0, None) == 0 and ctypes.sizeof(st) == 64
        assert T.snapshot_state(e) == before                       # nothing above moved a body
        ticks, level = e.hermite_block_state()
        only = np.empty(n, np.int32)
        assert e._L.nbody_hermite_block_get(e._h, None, only.ctypes.data) == 0 and only.tobytes() == level.tobytes()
        assert e._L.nbody_hermite_block_get(e._h, None, None) == 0 and not ticks.any()


@pytest.mark.parametrize("how", ["set_state", "step", "device_ptr_posm", "hermite_restart", "load_checkpoint"])
def test_what_ends_a_session(nb, how, tmp_path):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        e.save_checkpoint(str(tmp_path / "start.ckpt"))
        e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
        e.hermite_block_advance(1, max_block_steps=3)
        if how == "set_state":
            e.set_state(posm, vel)
        elif how == "step":
            e.step(1e-3, 1)
        elif how == "device_ptr_posm":
            assert e.device_ptr(nb._lib.BUF_POSM)[0]
        elif how == "hermite_restart":
            e.hermite_restart()
        else:
            e.load_checkpoint(str(tmp_path / "start.ckpt"))
        for call in three_calls(e)[1:]:
            raises(nb, nb._lib.ERR_STATE, call)
        e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)             # and a new one begins at tick 0
        assert e.hermite_block_advance(0)["ticks"] == 0


def test_shared_steps_and_a_session(nb):
    n, dt = 257, 1e-3
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
        y = Yardstick(a, b, posm, vel, DT_MAX, LEVELS, eta=ETA)
        for s in range(3):
            step_and_compare(a, y, f"block step {s + 1}")
        held = snapshot(a)
        for call in ((lambda: a.hermite_step(dt, 1)), a.hermite_timescale, (lambda: a.hermite_advance(dt))):
            assert "mid-frame" in raises(nb, nb._lib.ERR_STATE, call)   # ragged: the bodies are at times of their own
        assert "mid-frame" in raises(nb, nb._lib.ERR_STATE, lambda: a.hermite_block_begin(DT_MAX, LEVELS))
        same(snapshot(a), held, "refused calls")
        a.hermite_step(0.0, 1)                                     # a no-op stays one
        stats = a.hermite_block_advance(1)
        y.ref.advance(1)
        assert stats["synchronised"] and stats == y.ref.stats()
        # synchronised: a shared step works from the session's cache — Aarseth's criterion at once, no fresh evaluation — and ends it
        r = y.ref
        shared = H.Hermite(r.posm, r.vel, evaluate=evaluator(b))
        shared.a0, shared.j0, shared.a2, shared.a3 = r.a0.copy(), r.j0.copy(), r.a2.copy(), r.a3.copy()
        t, body, kind = a.hermite_timescale()
        t_ref, body_ref, _ = H.timescale(r.a0, r.j0, r.a2, r.a3)
        assert kind == 1 and body == body_ref and abs(t - t_ref) <= 1e-14 * t_ref
        raises(nb, nb._lib.ERR_STATE, a.hermite_block_state)       # the session has ended
        a.hermite_step(dt, 2)
        shared.step(dt, 2)
        T.same(T.snapshot(a), T.expected(shared), "two shared steps behind a frame of block steps")
        assert shared.evaluations == 2


def test_resume_from_a_checkpoint_with_the_saved_levels(nb, tmp_path):
    n = 257
    posm, vel = binary_scene(nb, n)
    ckpt, again = str(tmp_path / "block.ckpt"), str(tmp_path / "plain.ckpt")
    with f64(nb, n) as e, f64(nb, n) as resumed, f64(nb, n) as plain:
        e.set_state(posm, vel)
        e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA)
        first = e.hermite_block_advance(1)
        e.save_checkpoint(ckpt)
        levels = e.hermite_block_state()[1]
        e.hermite_restart()
        e.hermite_block_begin(DT_MAX, LEVELS, eta=ETA, level_in=levels)
        e.hermite_block_advance(1)
        assert resumed.load_checkpoint(ckpt) == first["block_steps"]
        resumed.hermite_block_begin(DT_MAX, LEVELS, eta=ETA, level_in=levels)
        again_stats = resumed.hermite_block_advance(1)
        same(snapshot(e), snapshot(resumed), "save, restart, begin with the levels, a frame against load, begin with the levels, a frame")
        assert e.steps_done() == resumed.steps_done() == first["block_steps"] + again_stats["block_steps"]
        assert plain.load_checkpoint(ckpt) == first["block_steps"]
        plain.save_checkpoint(again)
    data = open(ckpt, "rb").read()
    assert data[:8] == b"NBDYCKP2" and data == open(again, "rb").read()
    header = int.from_bytes(data[8:12], "little")
    assert len(data) == header + 3 * n * 32                       # the header and three double4 arrays: no levels, no times, no cache
