"""Hermite block sessions that carry the fp64 tracers — nbody_hermite_block_begin_tracers, nbody_hermite6_block_begin_tracers,
nbody_hermite_block_tracers_get, nbody_hermite6_block_tracers_get — on the device, both orders.

THE ORACLE is the one of tests/test_tracers_f64_gpu.py, here for block steps: a second fp64 context that holds the N bodies and,
appended behind them, the M tracers as bodies of mass 0 (N + M <= 32768: both contexts have 256-body chunks), run through the EXISTING
nbody_hermite[6]_block_begin with level_in = the bodies' levels followed by the tracers'.  A body of mass 0 adds exactly nothing, the
joint schedule of the carrying session is the augmented context's own schedule, and the point forms of the jerk and snap passes give the
body forms' bits: every comparison is BYTE FOR BYTE, after every block step.  tests/block_tracers_ref.py restates the joint schedule in
numpy (tests/test_block_tracers_ref.py).

The frame of the whole-frame tests: the Plummer spheres of test_tracers_f64_gpu.py with bodies 0 and 1 a hard binary of period 0.0225,
dt_max = 1.25e-3, four levels.  The binary starts at level 3 and stays there, everything else starts at levels 0 .. 2, and an eighth of
the tracers start at level 4, ALONE there: the first block step is tracer-only, the second has both sets, and once those tracers have
climbed to the levels their criterion asks for the binary steps alone."""
import ctypes

import numpy as np
import pytest

import hermite_block_ref as B
import hermite_ref as H
from jerk_ref import probe_geometry
from test_hermite6_gpu import fake_rccl  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DT_MAX, LEVELS = 1.25e-3, 4
_scenes = {}


def scene(nb, n, m=0):
    """(posm, vel, tpos, tvel) in fp64, read-only: test_tracers_f64_gpu.py's scene() — a Plummer sphere with masses that all differ and
    coordinates that are no fp32 numbers, m random moving points inside it — with bodies 0 and 1 made a hard binary."""
    if (n, m) not in _scenes:
        p32, v32 = nb.ic_plummer(n, seed=n)
        posm, vel = p32.astype(np.float64), v32.astype(np.float64)
        posm[:, :3] += 1e-7 * posm[:, :3] ** 2 + 1e-9
        vel[:, :3] += 1e-7 * vel[:, :3] ** 2 + 1e-9
        posm[:, 3] *= 1.0 + 0.5 * np.arange(n) / n + 1e-9 * np.arange(n)
        vel[:, 3] = 0.0
        rng = np.random.default_rng(7000 + n + m)
        tpos = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
        tvel = rng.normal(0.0, float(np.abs(vel[:, :3]).std()) + 1e-3, (m, 3))
        posm, vel, _ = B.binary_in_cluster(posm, vel)
        for a in (posm, vel, tpos, tvel):
            a.setflags(write=False)
        _scenes[(n, m)] = (posm, vel, tpos, tvel)
    return _scenes[(n, m)]


def augmented(posm, vel, tpos, tvel):
    """(posm, vel) of the oracle: the tracers appended as bodies of mass 0."""
    m = tpos.shape[0]
    tp = np.zeros((m, 4)); tv = np.zeros((m, 4))
    tp[:, :3] = tpos; tv[:, :3] = tvel
    return np.concatenate([posm, tp]), np.concatenate([vel, tv])


def given_levels(n, m, levels=LEVELS):
    """The deepest level holds ONLY tracers (an eighth of them); the binary one above it; everything else 0 .. 2."""
    rng = np.random.default_rng(n + m)
    lb = rng.integers(0, 2, n).astype(np.int32); lb[:2] = levels - 1
    lt = rng.integers(0, 3, m).astype(np.int32); lt[rng.choice(m, max(1, m // 8), replace=False)] = levels
    return lb, lt


class Order:
    """The calls of one order, by name."""

    def __init__(self, order):
        self.order, self.p = order, "hermite" if order == 4 else "hermite6"
        self.eta = 0.02 if order == 4 else 0.5
        self.env = "NBODY_HERMITE_BLOCK_LANES" if order == 4 else "NBODY_HERMITE6_BLOCK_LANES"
        self.width = 3 if order == 4 else 5                        # float4 per partial row
        self.start_passes = 1 if order == 4 else 2

    def __repr__(self):
        return f"order{self.order}"

    def call(self, e, name, *a, **kw):
        return getattr(e, f"{self.p}_{name}")(*a, **kw)

    def begin(self, e, levels=LEVELS, dt_max=DT_MAX, **kw):
        return self.call(e, "block_begin", dt_max, levels, eta=self.eta, **kw)

    def begin_tracers(self, e, levels=LEVELS, dt_max=DT_MAX, **kw):
        return self.call(e, "block_begin_tracers", dt_max, levels, eta=self.eta, **kw)

    def advance(self, e, frames=1, **kw):
        return self.call(e, "block_advance", frames, **kw)

    def bodies(self, e, n=None, session=True):
        """What a block step writes of the first n bodies: state, acc, cache and — in a session — T, level."""
        p, v, a = e.state(np.float64)
        out = (p, v, a) + tuple(self.call(e, "state")) + (tuple(self.call(e, "block_state")) if session else ())
        return tuple(np.ascontiguousarray(x[:n]) for x in out)

    def tracers(self, e, session=True):
        """What a block step writes of the carried tracers: pos, vel, cache and — in a session — T, level."""
        return tuple(e.tracers_f64()) + tuple(self.call(e, "tracers_state")) + (tuple(self.call(e, "block_tracers_state")[:2]) if session else ())

    def tracers_of(self, aug, n, session=True):
        """The same of the bodies behind the first n of the augmented context."""
        p, v, _ = aug.state(np.float64)
        out = (p[:, :3], v[:, :3]) + tuple(self.call(aug, "state")) + (tuple(self.call(aug, "block_state")) if session else ())
        return tuple(np.ascontiguousarray(x[n:]) for x in out)


ORDERS = [Order(4), Order(6)]


def f64(nb, n, **kw):
    return nb.NBodyEngine(n, precision="f64", **kw)


def raises(nb, code, call):
    with pytest.raises(nb.NBodyError) as er:
        call()
    assert er.value.code == code, (er.value.code, str(er.value))
    return str(er.value)


def passes(nb, e):
    return np.array([e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]])


def same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: array {k}: {g.dtype}{g.shape} against {w.dtype}{w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what}: array {k}: {int((g != w).reshape(len(g), -1).any(axis=1).sum())} of {len(g)} rows differ"


def probe_slab_points(n_total, width):
    """kernels_probe.hip's: the points whose partial rows (width float4 per point and chunk) fit 256 MiB, a multiple of 1024."""
    return max(1024, (256 << 20) // (probe_geometry(n_total)[0] * 16 * width) // 1024 * 1024)


def carrying(nb, o, n, m, eps=0.0, levels=True, **kw):
    """(e, aug, lb, lt): a context in a session that carries its m tracers, and the oracle in a plain session, both at tick 0."""
    posm, vel, tpos, tvel = scene(nb, n, m)
    lb, lt = given_levels(n, m) if levels else (None, None)
    e, aug = f64(nb, n, eps=eps, **kw), f64(nb, n + m, eps=eps)
    e.set_state(posm, vel); e.set_tracers_f64(tpos, tvel)
    aug.set_state(*augmented(posm, vel, tpos, tvel))
    o.begin_tracers(e, level_in=lb, tracer_level_in=lt)
    o.begin(aug, level_in=None if lb is None else np.concatenate([lb, lt]))
    return e, aug, lb, lt


def frame_against_the_oracle(nb, o, n, m, eps, levels):
    """One frame, a block step at a time; returns the (m_b, m_t) of every block step."""
    e, aug, lb, lt = carrying(nb, o, n, m, eps, levels)
    with e, aug:
        what = f"{o} N={n} M={m} eps={eps}"
        same(o.bodies(e), o.bodies(aug, n), f"{what} begin, bodies"); same(o.tracers(e), o.tracers_of(aug, n), f"{what} begin, tracers")
        sizes, st, ts = [], o.advance(e, 0), o.call(e, "block_tracers_state")[2]
        assert ts["carried"] == m and st["floor_hits"] + ts["floor_hits"] == o.advance(aug, 0)["floor_hits"]
        while not sizes or not st["synchronised"]:
            before = (st["body_steps"], ts["tracer_steps"])
            st, sa = o.advance(e, 1, max_block_steps=1), o.advance(aug, 1, max_block_steps=1)
            ts = o.call(e, "block_tracers_state")[2]
            sizes.append((st["body_steps"] - before[0], ts["tracer_steps"] - before[1]))
            step = f"{what} block step {len(sizes)} {sizes[-1]}"
            same(o.bodies(e), o.bodies(aug, n), f"{step}, bodies"); same(o.tracers(e), o.tracers_of(aug, n), f"{step}, tracers")
            assert st["block_steps"] == sa["block_steps"] == len(sizes) == e.steps_done() and st["ticks"] == sa["ticks"], step
            assert st["body_steps"] + ts["tracer_steps"] == sa["body_steps"] and st["floor_hits"] + ts["floor_hits"] == sa["floor_hits"], step
            assert st["pairs"] == st["body_steps"] * n and ts["pairs"] == ts["tracer_steps"] * n, step
        assert st["ticks"] == 1 << LEVELS and ts["tracer_only_steps"] == sum(1 for b, _ in sizes if b == 0)
        ticks, level, _ = o.call(e, "block_tracers_state")
        assert (ticks == st["ticks"]).all() and (ts["level_min"], ts["level_max"]) == (level.min(), level.max())
        print(f"{what}: {len(sizes)} block steps {sizes}")
        return sizes


# ---- 1: a whole frame, every block step -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(257, 300), (1000, 25)])
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_a_whole_frame_against_the_augmented_context(nb, o, eps, n, m):
    sizes = frame_against_the_oracle(nb, o, n, m, eps, levels=True)
    assert sizes[0][0] == 0 and sizes[0][1] == max(1, m // 8)      # the deepest level holds only tracers
    assert any(b > 0 and t > 0 for b, t in sizes) and any(t == 0 for _, t in sizes)
    assert sizes[-1] == (n, m)                                     # the frame end: everybody


@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_a_whole_frame_with_begins_own_start_rule(nb, o):
    frame_against_the_oracle(nb, o, 257, 300, 0.0, levels=False)


# ---- 2: the bodies do not see the tracers ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_the_bodies_are_untouched(nb, o):
    n, m = 257, 300
    posm, vel, tpos, tvel = scene(nb, n, m)
    lb, lt = given_levels(n, m)
    with f64(nb, n) as e, f64(nb, n) as plain:
        e.set_state(posm, vel); e.set_tracers_f64(tpos, tvel); plain.set_state(posm, vel)
        o.begin_tracers(e, level_in=lb, tracer_level_in=lt); o.begin(plain, level_in=lb)
        st, sp = o.advance(e, 1), o.advance(plain, 1)
        same(o.bodies(e), o.bodies(plain), f"{o} a frame with and without tracers")
        assert all(st[k] == sp[k] for k in ("body_steps", "pairs", "floor_hits", "level_min", "level_max", "ticks"))
        ts = o.call(e, "block_tracers_state")[2]
        assert st["block_steps"] == sp["block_steps"] + ts["tracer_only_steps"] and ts["tracer_only_steps"] >= 1


# ---- 3: levels = 0 is the shared step -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_levels_zero_is_the_shared_step(nb, o):
    n, m = 257, 300
    posm, vel, tpos, tvel = scene(nb, n, m)
    with f64(nb, n) as e, f64(nb, n) as shared:
        for c in (e, shared):
            c.set_state(posm, vel); c.set_tracers_f64(tpos, tvel)
        o.begin_tracers(e, levels=0)
        st = o.advance(e, 3)
        o.call(shared, "step", DT_MAX, 3)
        same(o.bodies(e)[:-2], o.bodies(shared, session=False), f"{o} bodies")
        same(o.tracers(e)[:-2], o.tracers(shared, session=False), f"{o} tracers")
        ts = o.call(e, "block_tracers_state")[2]
        assert (st["block_steps"], st["body_steps"], ts["tracer_steps"], ts["tracer_only_steps"]) == (3, 3 * n, 3 * m, 0)
        assert e.steps_done() == shared.steps_done() == 3


# ---- 4: the points per lane enter no sum ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_lane_shapes(nb, o, monkeypatch):
    n, m = 257, 300
    got = []
    for lanes in ("1", "2"):
        monkeypatch.setenv(o.env, lanes)                           # read at begin
        e, aug, _, _ = carrying(nb, o, n, m)
        with e, aug:
            o.advance(e, 1)
            got.append(o.bodies(e) + o.tracers(e))
    same(got[0], got[1], f"{o} one and two points per lane")


# ---- 5: an active set of tracers beyond a slab of partial rows --------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_tracers_beyond_a_slab(nb, o):
    n = 33000
    slab = probe_slab_points(n, o.width)
    m = slab + 600
    posm, vel, tpos, tvel = scene(nb, n, m)
    pick = np.r_[0:50, slab - 200:slab + 200, m - 50:m]            # both sides of the slab boundary, and both ends
    with f64(nb, n) as e, f64(nb, n) as few:
        e.set_state(posm, vel); e.set_tracers_f64(tpos, tvel)
        few.set_state(posm, vel); few.set_tracers_f64(tpos[pick], tvel[pick])
        for c in (e, few):
            o.begin_tracers(c, levels=0)
            st = o.advance(c, 1, max_block_steps=1)
            assert st["synchronised"] and st["block_steps"] == 1
        ts = o.call(e, "block_tracers_state")[2]
        assert (ts["carried"], ts["tracer_steps"], ts["pairs"]) == (m, m, m * n)
        same(tuple(x[pick] for x in o.tracers(e)), o.tracers(few), f"{o} {len(pick)} of {m} tracers, slab {slab}")
        same(o.bodies(e), o.bodies(few), f"{o} the bodies")


# ---- 6: small ends --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_one_tracer(nb, o):
    sizes = frame_against_the_oracle(nb, o, 257, 1, 0.0, levels=True)
    assert sizes[0] == (0, 1)


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_two_bodies_and_one_tracer(nb, o, given):
    """A circular pair at level 0 — or where the start rule puts it —, the tracer deeper."""
    posm, vel, period = H.kepler(0.0)
    tpos, tvel = np.array([[30.0, 40.0, 5.0]]), np.array([[1.0, -2.0, 0.5]])
    dt_max, levels = period / 64, 3
    kw = dict(level_in=np.zeros(2, np.int32), tracer_level_in=np.array([2], np.int32)) if given else {}
    with f64(nb, 2) as e, f64(nb, 3) as aug:
        e.set_state(posm, vel); e.set_tracers_f64(tpos, tvel)
        aug.set_state(*augmented(posm, vel, tpos, tvel))
        o.begin_tracers(e, levels, dt_max, **kw)
        o.begin(aug, levels, dt_max, level_in=np.array([0, 0, 2], np.int32) if given else None)
        steps = 0
        while steps == 0 or not st["synchronised"]:
            st, sa = o.advance(e, 1, max_block_steps=1), o.advance(aug, 1, max_block_steps=1)
            steps += 1
            same(o.bodies(e), o.bodies(aug, 2), f"{o} block step {steps}, bodies"); same(o.tracers(e), o.tracers_of(aug, 2), f"{o} block step {steps}, tracer")
            assert st["ticks"] == sa["ticks"]
        ts = o.call(e, "block_tracers_state")[2]
        assert st["body_steps"] + ts["tracer_steps"] == sa["body_steps"]
        if given:                                                  # the pair steps once, at the frame end; the tracer steps before it, alone
            assert st["body_steps"] == 2 and ts["tracer_only_steps"] == steps - 1 >= 1 and ts["tracer_steps"] == steps


# ---- 7: hand-over ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_mid_frame_and_frame_end(nb, o):
    n, m = 257, 25
    e, aug, lb, lt = carrying(nb, o, n, m)
    E = nb._lib
    with e, aug:
        st = o.advance(e, 1, max_block_steps=2); o.advance(aug, 1, max_block_steps=2)
        assert not st["synchronised"]
        before = o.bodies(e) + o.tracers(e)
        for other in ORDERS:                                       # in mid-frame nothing but block_advance moves the state on
            for call in ((lambda: other.call(e, "step", DT_MAX, 1)), (lambda: other.call(e, "timescale")),
                         (lambda: other.call(e, "tracers_timescale")), (lambda: other.begin(e)), (lambda: other.begin_tracers(e))):
                assert "mid-frame" in raises(nb, E.ERR_STATE, call)
        for n_set in (m, 0):                                       # the session's lists index the tracers it began with
            pos = scene(nb, n, m)[2][:n_set]
            assert "block session" in raises(nb, E.ERR_STATE, lambda: e.set_tracers_f64(pos))
        same(o.bodies(e) + o.tracers(e), before, f"{o} refused calls change nothing")   # (the getters work in mid-frame: a ragged state)
        o.advance(e, 1); o.advance(aug, 1)
        assert o.call(e, "tracers_timescale")[2] == 1              # a whole frame: the tracers' derivatives are a step's
        raises(nb, E.ERR_STATE, lambda: o.call(e, "block_tracers_state"))   # ... and the call ended the session, at a frame end
        o.call(e, "step", DT_MAX, 1); o.call(aug, "step", DT_MAX, 1)
        same(o.bodies(e, session=False), o.bodies(aug, n, session=False), f"{o} a shared step, bodies")
        same(o.tracers(e, session=False), o.tracers_of(aug, n, session=False), f"{o} a shared step, tracers")
        e.set_tracers_f64(np.zeros((0, 3)))                        # no session: the tracers can go


@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_resume_from_a_checkpoint_with_the_saved_levels(nb, o, tmp_path):
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    lb, lt = given_levels(n, m)
    ckpt, again = str(tmp_path / "carried.ckpt"), str(tmp_path / "plain.ckpt")
    with f64(nb, n) as e, f64(nb, n) as resumed, f64(nb, n) as plain:
        e.set_state(posm, vel); e.set_tracers_f64(tpos, tvel)
        o.begin_tracers(e, level_in=lb, tracer_level_in=lt)
        first = o.advance(e, 1)
        e.save_checkpoint(ckpt)
        levels, tracer_levels = o.call(e, "block_state")[1], o.call(e, "block_tracers_state")[1]
        saved = e.tracers_f64()
        e.hermite_restart()
        o.begin_tracers(e, level_in=levels, tracer_level_in=tracer_levels)
        o.advance(e, 1)
        assert resumed.load_checkpoint(ckpt) == first["block_steps"]
        resumed.set_tracers_f64(*saved)
        o.begin_tracers(resumed, level_in=levels, tracer_level_in=tracer_levels)
        o.advance(resumed, 1)
        same(o.bodies(e) + o.tracers(e), o.bodies(resumed) + o.tracers(resumed), f"{o} resumed on the writer against a fresh context")
        assert e.steps_done() == resumed.steps_done()
        assert plain.load_checkpoint(ckpt) == first["block_steps"]
        plain.save_checkpoint(again)
    data = open(ckpt, "rb").read()
    assert data[:8] == b"NBDYCKP2" and data == open(again, "rb").read()
    assert len(data) == int.from_bytes(data[8:12], "little") + 3 * n * 32   # no tracers, no levels, no times, no cache


# ---- 8: accounting --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_pass_counts(nb, o):
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    lb, lt = given_levels(n, m)
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel); e.set_tracers_f64(tpos, tvel)
        p0 = passes(nb, e)
        o.begin_tracers(e, level_in=lb, tracer_level_in=lt)
        assert tuple(passes(nb, e) - p0) == (2 * o.start_passes, 0)    # the bodies' start, and as many passes again for the tracers
        kinds = set()
        st, ts = o.advance(e, 0), o.call(e, "block_tracers_state")[2]
        while not kinds or not st["synchronised"]:
            p1, before = passes(nb, e), (st["body_steps"], ts["tracer_steps"])
            st, ts = o.advance(e, 1, max_block_steps=1), o.call(e, "block_tracers_state")[2]
            both = st["body_steps"] > before[0] and ts["tracer_steps"] > before[1]
            assert tuple(passes(nb, e) - p1) == (2 if both else 1, 1)
            kinds.add("both" if both else "bodies" if st["body_steps"] > before[0] else "tracers")
        assert kinds == {"both", "bodies", "tracers"} and e.steps_done() == st["block_steps"]
        p2 = passes(nb, e)
        o.begin_tracers(e, level_in=lb, tracer_level_in=lt)        # a new session on valid caches: no pass
        assert tuple(passes(nb, e) - p2) == (0, 0)


# ---- 9: errors ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o", ORDERS, ids=repr)
def test_errors(nb, o):
    E = nb._lib
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    get = getattr(nb._lib.lib(), f"nbody_{o.p}_block_tracers_get")
    big = 2000
    p32, v32 = nb.ic_reference_box(big, 1000.0, seed=1)
    for kw in ({}, {"precision": "f32_kahan"}, {"precision": "f64", "i_begin": 0, "i_count": 1000}):
        with nb.NBodyEngine(big, **kw) as e:
            e.set_state(*((p32.astype(np.float64), v32.astype(np.float64)) if kw.get("precision") == "f64" else (p32, v32)))
            raises(nb, E.ERR_UNSUPPORTED, lambda: o.begin_tracers(e))
            raises(nb, E.ERR_UNSUPPORTED, lambda: o.call(e, "block_tracers_state"))
    with f64(nb, n) as e:
        raises(nb, E.ERR_STATE, lambda: o.begin_tracers(e))        # no particles set
        e.set_state(posm, vel)
        raises(nb, E.ERR_STATE, lambda: o.call(e, "block_tracers_state"))   # no session
        assert "tracer_level_in" in raises(nb, E.ERR_INVALID, lambda: o.begin_tracers(e, tracer_level_in=np.zeros(3, np.int32)))
        raises(nb, E.ERR_STATE, lambda: o.call(e, "block_tracers_state"))
        o.begin_tracers(e)                                         # without tracers: the plain begin
        ticks, level, ts = o.call(e, "block_tracers_state")
        assert ticks.size == level.size == 0 and set(ts.values()) == {0}
        e.set_tracers_f64(np.zeros((0, 3)))                        # (a session that carries none: removing none is fine)
        assert "block session" in raises(nb, E.ERR_STATE, lambda: e.set_tracers_f64(tpos, tvel))
        e.hermite_restart()
        e.set_tracers_f64(tpos, tvel)
        for begin in (o.begin, lambda c: o.begin(c, level_in=np.zeros(n, np.int32))):   # the plain begins still refuse, and say what carries them
            msg = raises(nb, E.ERR_UNSUPPORTED, lambda: begin(e))
            assert "nbody_set_tracers_f64(ctx, NULL, 0, NULL, 0, 0)" in msg and f"nbody_{o.p}_block_begin_tracers" in msg
        for bad in (float("nan"), 0.0, -1.0):
            raises(nb, E.ERR_INVALID, lambda: o.begin_tracers(e, dt_max=bad))
        raises(nb, E.ERR_INVALID, lambda: o.begin_tracers(e, levels=41))
        assert "level_in[256]" in raises(nb, E.ERR_INVALID, lambda: o.begin_tracers(e, level_in=np.r_[np.zeros(n - 1), LEVELS + 1]))
        for k, v in ((0, -1), (m - 1, LEVELS + 1)):
            lt = np.zeros(m, np.int32); lt[k] = v
            assert f"tracer_level_in[{k}]" in raises(nb, E.ERR_INVALID, lambda: o.begin_tracers(e, tracer_level_in=lt))
        raises(nb, E.ERR_STATE, lambda: o.call(e, "block_tracers_state"))   # none of those began a session
        o.begin_tracers(e)
        st = E.HermiteBlockTracerStats()
        assert ctypes.sizeof(st) == 48
        st.struct_size = 40
        assert get(e._h, None, None, ctypes.byref(st)) == E.ERR_INVALID
        assert get(e._h, None, None, None) == E.ERR_INVALID
        only = np.empty(m, np.int32)
        assert get(e._h, None, only.ctypes.data, None) == 0 and only.tobytes() == o.call(e, "block_tracers_state")[1].tobytes()
        other = ORDERS[o.order == 4]
        raises(nb, E.ERR_STATE, lambda: other.call(e, "block_tracers_state"))   # the other order's session is another one
        for n_set in (m, 0):
            assert "block session" in raises(nb, E.ERR_STATE, lambda: e.set_tracers_f64(tpos[:n_set]))
        e.hermite_restart()
        e.set_tracers_f64(np.zeros((0, 3)))
        assert e.tracer_count_f64 == 0


def test_errors_on_a_multi_device_context(nb, fake_rccl, monkeypatch):  # noqa: F811
    monkeypatch.setenv("NBODY_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("NBODY_MULTI_SHARE_DEVICE", "1")
    p32, v32 = nb.ic_reference_box(2000, 1000.0, seed=1)
    with nb.NBodyEngine(2000, devices=[0]) as e:
        e.set_state(p32, v32)
        for o in ORDERS:
            assert "multi-device" in raises(nb, nb._lib.ERR_UNSUPPORTED, lambda: o.begin_tracers(e))
            assert "multi-device" in raises(nb, nb._lib.ERR_UNSUPPORTED, lambda: o.call(e, "block_tracers_state"))
