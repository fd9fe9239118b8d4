"""Sixth-order Hermite block time steps — nbody_hermite6_block_begin, nbody_hermite6_block_advance, nbody_hermite6_block_get — against
tests/hermite6_block_ref.py, the scheme restated in numpy (tests/test_hermite6_block_ref.py pins that yardstick and the level rule on
the CPU).

The evaluation of a block step is, for every active body, what nbody_get_snap_f64(acc_in = ap) returns for that body on a context
holding the predicted state, and everything around it — the level rule included, which has no cube root — is correctly rounded fp64
arithmetic in a documented order.  So EVERY comparison here is byte for byte, after every block step (max_block_steps = 1): a second fp64
context is loaded with numpy's predicted state, its snap(ap) supplies all rows, numpy takes those of the active bodies and its corrector
and level rule give every bit the stepping context must hold — positions, velocities, stored accelerations, a0, j0, s0, a3, a4, a5, the
bodies' times and levels, the totals.

Scenes: tests/test_hermite_block_gpu.py's — Plummer spheres with bodies 0 and 1 a hard binary.  N = 257 is a full tile and a ragged one;
N = 1025 is five j-chunks of 256 bodies, and an active set of 1025 is three workgroups of two bodies per lane, the last one body deep,
or five of one body per lane; N = 65536 is the size at which an active set of all bodies passes through three slabs of partial rows."""
import ctypes

import numpy as np
import pytest

import hermite6_block_ref as B6
import hermite6_ref as H6
import hermite_block_ref as B
import test_hermite6_gpu as T
from test_hermite6_gpu import DeviceBuffer, evaluator, f64, fake_rccl, passes, raises, scene  # noqa: F401  (fake_rccl is a fixture)

pytestmark = pytest.mark.gpu

DT_MAX, LEVELS, ETA = 0.01, 12, 0.5
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
    return T.snapshot(e) + tuple(x.tobytes() for x in e.hermite6_block_state())


class Yardstick:
    """hermite6_block_ref.Hermite6Block beside a context in session, with the stored accelerations carried along: NBODY_BUF_ACC is
    (a1, 0) for a body that has stepped and what the context held at begin for one that has not."""

    def __init__(self, e, other, posm, vel, dt_max, levels, **kw):
        self.ref = B6.Hermite6Block(posm, vel, dt_max, levels, evaluate=evaluator(other), **kw)
        self.acc = e.state(np.float64)[2].copy()

    def block_step(self):
        act = self.ref.block_step()
        self.acc[act, :3] = self.ref.a0[act]
        self.acc[act, 3] = 0.0
        return act

    def expected(self):
        r = self.ref
        return (r.posm.tobytes(), r.vel.tobytes(), self.acc.tobytes()) + tuple(x.tobytes() for x in (r.a0, r.j0, r.s0, r.a3, r.a4, r.a5)) + (
            r.T.tobytes(), r.level.tobytes())


def same(got, want, what):
    assert len(got) == len(want) == len(NAMES)
    for name, g, w in zip(NAMES, got, want):
        assert g == w, f"{what}: {name} differ"


def step_and_compare(e, y, what):
    stats = e.hermite6_block_advance(1, max_block_steps=1)
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
        a.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
        y = Yardstick(a, b, posm, vel, DT_MAX, LEVELS, eta=ETA, eps=eps)
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
            whole.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
            stats = whole.hermite6_block_advance(1)
            same(snapshot(whole), y.expected(), f"N={n} eps={eps} one frame in one call")
            assert stats == y.ref.stats() and whole.steps_done() == taken
            assert whole.hermite6_block_advance(0) == stats        # frames == 0: nothing moves
            same(snapshot(whole), y.expected(), "frames == 0")


# ---- 2: the shapes the gather can get wrong ---------------------------------------------------------------------------------------------------

SETS = {"last": lambda n: [n - 1], "first257": lambda n: range(257), "every_other": lambda n: range(0, n, 2), "all": lambda n: range(n)}


@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("which", list(SETS))
def test_one_block_step_of_a_given_active_set(nb, monkeypatch, which, lanes):
    n = 1025
    monkeypatch.setenv("NBODY_HERMITE6_BLOCK_LANES", lanes)        # bodies per lane of the evaluation, either way for every set
    posm, vel = binary_scene(nb, n)
    members = np.array(list(SETS[which](n)))
    level_in = np.zeros(n, np.int32)
    level_in[members] = 1                                          # everything at level 0 except the set: it alone is due at tick 1
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite6_block_begin(DT_MAX, 1, eta=ETA, level_in=level_in)
        y = Yardstick(a, b, posm, vel, DT_MAX, 1, eta=ETA, level_in=level_in)
        same(snapshot(a), y.expected(), f"{which} begin")
        act = step_and_compare(a, y, f"{which} lanes={lanes}")
        assert act.tolist() == members.tolist() and a.hermite6_block_advance(0)["body_steps"] == len(members)
        others = np.setdiff1d(np.arange(n), members)
        p, v, _ = a.state(np.float64)
        assert p[others].tobytes() == posm[others].tobytes() and v[others].tobytes() == vel[others].tobytes()
        if which == "all":                                         # m = N: the shared step of dt_max / 2
            b.set_state(posm, vel)
            b.hermite6_step(DT_MAX / 2, 1)
            T.same(snapshot(a)[:9], T.snapshot(b), "m = N against nbody_hermite6_step")


# ---- 3: the degenerate case, and the slabs ----------------------------------------------------------------------------------------------------

def test_levels_zero_is_the_shared_step(nb):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite6_block_begin(DT_MAX, 0, eta=ETA)
        stats = a.hermite6_block_advance(3)
        b.set_state(posm, vel)
        b.hermite6_step(DT_MAX, 3)
        T.same(snapshot(a)[:9], T.snapshot(b), "three block steps at levels = 0 against nbody_hermite6_step(dt_max, 3)")
        assert (stats["block_steps"], stats["frames_done"], stats["body_steps"], stats["ticks"]) == (3, 3, 3 * n, 3)
        assert a.steps_done() == b.steps_done() == 3


def test_an_active_set_of_three_slabs(nb):
    """N = 65536, every body at level 0: one block step of m = N, two bodies per lane, through three slabs of partial rows (25600
    bodies each) — evaluation and corrector slab by slab — against the shared step's one launch per slab and its own corrector."""
    n = 65536
    posm, vel = scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite6_block_begin(DT_MAX, 2, eta=ETA, level_in=np.zeros(n, np.int32))
        stats = a.hermite6_block_advance(1, max_block_steps=1)
        assert (stats["block_steps"], stats["body_steps"], stats["pairs"], stats["ticks"]) == (1, n, n * n, 4) and stats["synchronised"]
        b.set_state(posm, vel)
        b.hermite6_step(DT_MAX, 1)
        T.same(snapshot(a)[:9], T.snapshot(b), "m = N = 65536 against nbody_hermite6_step(dt_max, 1)")
        ticks, _ = a.hermite6_block_state()
        assert (ticks == 4).all()


# ---- 4: floor hits ----------------------------------------------------------------------------------------------------------------------------

def test_floor_hits_are_clamped_and_counted(nb):
    n, levels = 257, 2                                             # the binary wants deeper levels than 2 at begin (eta_start) and after
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite6_block_begin(DT_MAX, levels, eta=0.1)            # (eta 0.1: the criterion itself asks for less than dt_max / 4)
        y = Yardstick(a, b, posm, vel, DT_MAX, levels, eta=0.1)
        at_begin = y.ref.floor_hits
        assert at_begin >= 2 and a.hermite6_block_advance(0)["floor_hits"] == at_begin
        while y.ref.ticks < 1 << levels:
            step_and_compare(a, y, f"levels = {levels}, block step {y.ref.block_steps + 1}")
        stats = a.hermite6_block_advance(0)
        print(f"floor hits {stats['floor_hits']} ({at_begin} at begin) in {stats['block_steps']} block steps")
        assert stats == y.ref.stats()
        assert stats["floor_hits"] == y.ref.floor_hits > at_begin and stats["level_max"] == levels


# ---- 5: accounting ----------------------------------------------------------------------------------------------------------------------------

def test_pass_counts(nb):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0, u0 = passes(nb, e)
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
        assert tuple(np.subtract(passes(nb, e), (f0, u0))) == (2, 0)   # a fresh context's begin: the jerk pass and the snap pass
        stats = e.hermite6_block_advance(1, max_block_steps=7)
        assert stats["block_steps"] == 7 and tuple(np.subtract(passes(nb, e), (f0, u0))) == (9, 7) and e.steps_done() == 7
        stats = e.hermite6_block_advance(1)
        k = stats["block_steps"]
        assert stats["synchronised"] and tuple(np.subtract(passes(nb, e), (f0, u0))) == (k + 2, k)
        assert stats["pairs"] == stats["body_steps"] * n and stats["body_steps"] < k * n and e.steps_done() == k
        assert e.kernel_time(nb._lib.KERNEL_FORCES)[0] > 0 and e.kernel_time(nb._lib.KERNEL_UPDATE)[0] > 0
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)            # a new session on the valid cache: no pass
        assert passes(nb, e)[0] - f0 == k + 2
        assert e.hermite6_block_advance(0)["block_steps"] == 0 and e.steps_done() == k
        e.hermite6_step(DT_MAX, 1)                                 # ... and a begin behind a shared step: none either
        f1 = passes(nb, e)[0]
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
        assert passes(nb, e)[0] == f1


def test_begin_on_the_cache_a_shared_step_left(nb):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as a, f64(nb, n) as b:
        a.set_state(posm, vel)
        a.hermite6_step(1e-3, 2)
        p, v, _ = a.state(np.float64)
        cache = a.hermite6_state()
        a.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
        y = Yardstick(a, b, p, v, DT_MAX, LEVELS, eta=ETA, cache=cache)
        same(snapshot(a), y.expected(), "begin on a cache with derivatives")
        for s in range(4):
            step_and_compare(a, y, f"block step {s + 1} from a shared step's cache")
        assert y.ref.evaluations == 4


# ---- 6: errors and session rules ------------------------------------------------------------------------------------------------------------------

def three_calls(e):
    return (lambda: e.hermite6_block_begin(DT_MAX, LEVELS)), (lambda: e.hermite6_block_advance(1)), e.hermite6_block_state


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
            assert "nbody_hermite6_block_begin" in raises(nb, E.ERR_STATE, call)
        before = T.snapshot_state(e)
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(bad, LEVELS))
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(DT_MAX, LEVELS, eta=bad))
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(DT_MAX, LEVELS, eta_start=bad))
        for levels in (-1, 41):
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(DT_MAX, levels))
        assert "normal" in raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(1e-300, 40))   # the tick itself
        assert "cube" in raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(1e-100, 10))     # a normal tick, 1e-309 cubed
        for lv in (np.full(n, LEVELS + 1), np.r_[np.zeros(n - 1), -1]):
            assert "level_in" in raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_begin(DT_MAX, LEVELS, level_in=lv))
        for call in three_calls(e)[1:]:                            # none of those began a session
            raises(nb, E.ERR_STATE, call)
        e.hermite6_block_begin(DT_MAX, LEVELS)
        raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_advance(-1))
        raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_advance(1, max_block_steps=-1))
        raises(nb, E.ERR_INVALID, lambda: e.hermite6_block_advance(2 ** 62))
        st = E.HermiteBlockStats()
        st.struct_size = ctypes.sizeof(st) - 8
        assert e._L.nbody_hermite6_block_advance(e._h, 1, 1, ctypes.byref(st)) == E.ERR_INVALID
        assert e._L.nbody_hermite6_block_advance(e._h, 0, 0, None) == 0
        assert T.snapshot_state(e) == before                       # nothing above moved a body
        ticks, level = e.hermite6_block_state()
        only = np.empty(n, np.int32)
        assert e._L.nbody_hermite6_block_get(e._h, None, only.ctypes.data) == 0 and only.tobytes() == level.tobytes()
        assert e._L.nbody_hermite6_block_get(e._h, None, None) == 0 and not ticks.any()
        raises(nb, E.ERR_STATE, e.hermite_block_state)             # the fourth-order session is another one


def mid_frame_session(e, posm, vel):
    """A sixth-order session stopped in mid-frame: one body on half steps, one block step taken."""
    n = len(posm)
    e.set_state(posm, vel)
    level_in = np.zeros(n, np.int32)
    level_in[n // 2] = 1
    e.hermite6_block_begin(DT_MAX, 1, eta=ETA, level_in=level_in)
    st = e.hermite6_block_advance(1, max_block_steps=1)
    assert not st["synchronised"] and st["ticks"] == 1


CALLS = {"hermite6_step": lambda e: e.hermite6_step(1e-3, 1), "hermite6_timescale": lambda e: e.hermite6_timescale(),
         "hermite6_advance": lambda e: e.hermite6_advance(1e-3), "hermite_step": lambda e: e.hermite_step(1e-3, 1),
         "hermite_timescale": lambda e: e.hermite_timescale(), "hermite_advance": lambda e: e.hermite_advance(1e-3),
         "hermite_block_begin": lambda e: e.hermite_block_begin(DT_MAX, 1), "hermite6_block_begin": lambda e: e.hermite6_block_begin(DT_MAX, 1)}


@pytest.mark.parametrize("which", list(CALLS))
def test_a_call_on_a_session_in_mid_frame_and_at_a_frame_end(nb, which):
    n = 257
    posm, vel = binary_scene(nb, n)
    call = CALLS[which]
    with f64(nb, n) as e, f64(nb, n) as fresh:
        mid_frame_session(e, posm, vel)
        held = snapshot(e)
        text = raises(nb, nb._lib.ERR_STATE, lambda: call(e))
        assert "mid-frame" in text and "sixth-order" in text
        same(snapshot(e), held, f"{which} refused")
        assert len(e.hermite6_state()) == 6                        # the cache reads during a session: a row belongs to its own T_i
        a0 = e.snap()[0]                                           # the getters answer on the stored state and end nothing
        assert a0.tobytes() == e.jerk(np.float64)[0].tobytes()
        same(snapshot(e), held, "getters")
        stats = e.hermite6_block_advance(1)
        assert stats["synchronised"]
        p, v, _ = e.state(np.float64)
        cache = e.hermite6_state()
        call(e)                                                    # at a frame end: the session ends, the call proceeds
        if which == "hermite6_block_begin":
            assert e.hermite6_block_advance(0)["ticks"] == 0 and e.hermite6_block_advance(0)["block_steps"] == 0
            return
        raises(nb, nb._lib.ERR_STATE, e.hermite6_block_state)
        assert "nbody_hermite6_block_begin" in raises(nb, nb._lib.ERR_STATE, lambda: e.hermite6_block_advance(1))
        if which == "hermite6_step":                               # ... from the session's cache: every body has stepped, a3, a4, a5 are in
            ref = H6.Hermite6(p, v, evaluate=evaluator(fresh))
            ref.a0, ref.j0, ref.s0, ref.a3, ref.a4, ref.a5 = (x.copy() for x in cache)
            ref.step(1e-3, 1)
            T.same(T.snapshot(e), T.expected(ref), "hermite6_step at a frame end")
            assert ref.evaluations == 1
        elif which == "hermite6_timescale":
            assert e.hermite6_timescale()[2] == 1
            T.same(T.snapshot(e)[3:], tuple(x.tobytes() for x in cache), "the cache behind hermite6_timescale")
        elif which == "hermite_step":                              # the fourth-order calls start from the stored state and forget the cache
            fresh.set_state(p, v)
            fresh.hermite_step(1e-3, 1)
            assert T.snapshot4(e) == T.snapshot4(fresh)
            raises(nb, nb._lib.ERR_STATE, e.hermite6_state)
        elif which in ("hermite_advance", "hermite_block_begin"):
            raises(nb, nb._lib.ERR_STATE, e.hermite6_state)


def test_begin_against_a_fourth_order_session(nb):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        level_in = np.zeros(n, np.int32)
        level_in[n // 2] = 1
        e.hermite_block_begin(DT_MAX, 1, level_in=level_in)
        assert not e.hermite_block_advance(1, max_block_steps=1)["synchronised"]
        assert "mid-frame" in raises(nb, nb._lib.ERR_STATE, lambda: e.hermite6_block_begin(DT_MAX, LEVELS))
        raises(nb, nb._lib.ERR_STATE, e.hermite6_block_state)
        assert e.hermite_block_advance(1)["synchronised"]
        e.hermite6_block_begin(DT_MAX, LEVELS)                     # at a frame end: that session ends, this one begins
        raises(nb, nb._lib.ERR_STATE, e.hermite_block_state)
        assert e.hermite6_block_advance(0)["ticks"] == 0


@pytest.mark.parametrize("how", ["set_state", "step", "device_ptr_posm", "bind_device_state", "hermite_restart", "load_checkpoint"])
def test_what_ends_a_session(nb, how, tmp_path):
    n = 257
    posm, vel = binary_scene(nb, n)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        e.save_checkpoint(str(tmp_path / "start.ckpt"))
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
        e.hermite6_block_advance(1, max_block_steps=3)
        if how == "set_state":
            e.set_state(posm, vel)
        elif how == "step":
            e.step(1e-3, 1)
        elif how == "device_ptr_posm":
            assert e.device_ptr(nb._lib.BUF_POSM)[0]
        elif how == "bind_device_state":
            e.bind_device_state(acc=DeviceBuffer(n * 32))
        elif how == "hermite_restart":
            e.hermite_restart()
        else:
            e.load_checkpoint(str(tmp_path / "start.ckpt"))
        for call in three_calls(e)[1:]:
            raises(nb, nb._lib.ERR_STATE, call)
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)            # and a new one begins at tick 0
        assert e.hermite6_block_advance(0)["ticks"] == 0


def test_resume_from_a_checkpoint_with_the_saved_levels(nb, tmp_path):
    n = 257
    posm, vel = binary_scene(nb, n)
    ckpt, again = str(tmp_path / "block6.ckpt"), str(tmp_path / "plain.ckpt")
    with f64(nb, n) as e, f64(nb, n) as resumed, f64(nb, n) as plain:
        e.set_state(posm, vel)
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA)
        first = e.hermite6_block_advance(1)
        e.save_checkpoint(ckpt)
        levels = e.hermite6_block_state()[1]
        e.hermite_restart()
        e.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA, level_in=levels)
        e.hermite6_block_advance(1)
        assert resumed.load_checkpoint(ckpt) == first["block_steps"]
        resumed.hermite6_block_begin(DT_MAX, LEVELS, eta=ETA, level_in=levels)
        again_stats = resumed.hermite6_block_advance(1)
        same(snapshot(e), snapshot(resumed), "save, restart, begin with the levels, a frame against load, begin with the levels, a frame")
        assert e.steps_done() == resumed.steps_done() == first["block_steps"] + again_stats["block_steps"]
        assert plain.load_checkpoint(ckpt) == first["block_steps"]
        plain.save_checkpoint(again)
    data = open(ckpt, "rb").read()
    assert data[:8] == b"NBDYCKP2" and data == open(again, "rb").read()
    header = int.from_bytes(data[8:12], "little")
    assert len(data) == header + 3 * n * 32                       # the header and three double4 arrays: no levels, no times, no cache


def test_the_command_line(nb, tmp_path, capsys):
    import json
    from parallelnbody_amd.__main__ import main
    n, frames = 257, 2
    out = str(tmp_path / "block6.npy")
    main(["--plummer", "--n", str(n), "--precision", "f64", "--integrator", "hermite6-block", "--levels", "6", "--dt", "0.01", "--steps",
          str(frames), "--dump-positions", out])
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    posm, vel = nb.ic_plummer(n, seed=1)
    with f64(nb, n) as e:                                          # defaults: eta = 0.5; one session for the run
        e.set_state(posm, vel)
        e.hermite6_block_begin(0.01, 6, eta=0.5)
        stats = e.hermite6_block_advance(frames)
        assert np.load(out).tobytes() == e.positions().tobytes()
    assert lines[-1]["steps_done"] == stats["block_steps"] >= frames
