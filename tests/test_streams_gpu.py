"""The stream contract (include/nbody.h): a context works on its own non-blocking stream or on the caller's, never on
the null stream's implicit ordering; nbody_step returns with its steps in flight, and whatever is called next — an upload, a getter, a
query — is ordered behind them.

Part A: two contexts with the same parameters and the same state.  The SETTLED twin waits (synchronize()) before every call under test;
the BUSY twin is given the call immediately behind a load — step(dt, K), on fp64 contexts also hermite_step(dt, K) — that is still
running.  Both run the same load, so when ordering is right they agree in every byte: every comparison here is byte equality.  K is
sized per shape (Rig.size_k) so that the load outlasts the slowest call under test ten times over and by 50 ms at least.

Part B (tests/helpers/stream_worker.py, a child process: torch brings its HIP runtime up first there): a caller's stream — torch work
queued ahead of the engine and behind it with no host wait in between, nbody_set_stream there and back, the launch counts.

Measured on an MI355X (K, t_wait, t_idle per shape): see DESIGN.md, "Ordering on the stream"."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1e-4
K_FIRST, K_CAP = 64, 65536
WAIT_FACTOR, WAIT_MIN = 10.0, 0.050                                # t_wait >= 10 t_idle (host timing jitters by milliseconds) and >= 50 ms

# the smallest shapes that still reach each stepping path; grow: what n is raised to, for that shape only, if the host cannot get ahead
# of the device at it (seen at f32 n = 2000) — never past where the shape's kernel changes (the one-launch step: 16384 bodies; the
# generic block kernel of the Kahan and fp64 contexts: 6656), which the rigs fixture checks by the kernel's name
SHAPES = {
    "f32-2000": dict(precision="f32", n=2000, load="step", grow=(4096, 8192)),              # the one-launch step with buffer swapping
    "f32-20000": dict(precision="f32", n=20000, load="step", grow=()),                      # the symmetric pass with fused update
    "kahan-2000": dict(precision="f32_kahan", n=2000, load="step", grow=(4096,)),           # the generic block kernel
    "f64-2000": dict(precision="f64", n=2000, load="step", grow=(4096,)),                   # the generic block kernel, fp64
    "f64-1025-hermite": dict(precision="f64", n=1025, load="hermite", grow=(4096,)),        # fp64 under a Hermite load
}


def flat(x):
    """Every byte of a result: arrays, numbers, tuples (named ones too), dicts."""
    if isinstance(x, dict):
        return b"{" + b",".join(str(k).encode() + b":" + flat(v) for k, v in sorted(x.items())) + b"}"
    if isinstance(x, (tuple, list)):
        return b"(" + b"|".join(flat(v) for v in x) + b")"
    if x is None:
        return b"None"
    a = np.asarray(x)
    return repr(x).encode() if a.dtype == object else a.tobytes()


def four(a3, dtype):
    out = np.zeros((a3.shape[0], 4), dtype)
    out[:, :3] = a3
    return out


def new_state(nb, n, seed):
    """(posm, vel) in fp64 with coordinates that are no fp32 numbers and masses that all differ; velocity w = 0."""
    p32, v32 = nb.ic_plummer(n, seed=seed)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    posm[:, :3] += 1e-7 * posm[:, :3] ** 2 + 1e-9
    vel[:, :3] += 1e-7 * vel[:, :3] ** 2 + 1e-9
    posm[:, 3] *= 1.0 + 0.5 * np.arange(n) / n
    vel[:, 3] = 0.0
    assert (posm[:, :3].astype(np.float32) != posm[:, :3]).all()
    return posm, vel


class DeviceBuffer:
    """Caller-owned device memory for nbody_bind_device_state (the pattern of tests/test_hermite6_gpu.py), filled from a host array."""

    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), host.nbytes) == 0
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0 and self.hip.hipDeviceSynchronize() == 0

    def data_ptr(self):
        return self.ptr.value

    def __del__(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = ctypes.c_void_p()


class Rig:
    """The twins of one shape, a third context for the measurements, and K."""

    def __init__(self, nb, key, n, tmp):
        spec = SHAPES[key]
        self.nb, self.key, self.n, self.precision, self.hermite = nb, key, n, spec["precision"], spec["load"] == "hermite"
        self.f64 = self.precision == "f64"
        self.plain32 = self.precision == "f32"
        self.own = np.float64 if self.f64 else np.float32
        self.other = np.float32 if self.f64 else np.float64
        self.tmp = tmp
        p, v = new_state(nb, n, n)
        # the start: ic_plummer's equal masses (the equal-mass kernels), as the context's own type
        p[:, 3] = p[:, 3].mean()
        self.posm0, self.vel0 = p.astype(self.own), v.astype(self.own)
        self.new64 = new_state(nb, n, n + 1)
        rng = np.random.default_rng(n)
        self.acc_in = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
        self.points = rng.normal(0.0, 100.0, (3000, 3))
        self.settled, self.busy, self.third = (self.fresh() for _ in range(3))
        self.kernel = self.settled.launch_config()["kernel"]
        self.mirror = {}
        for e in (self.settled, self.busy):
            self.mirror[id(e)] = np.zeros(n, nb.PARTICLE_DTYPE)
            e.pin(self.mirror[id(e)])
        # a file saved earlier: another state, five steps on, accelerations stored
        self.third.set_state(*(x.astype(self.own) for x in new_state(nb, n, n + 2)))
        self.third.step(DT, 5)
        self.ckpt = os.path.join(tmp, key + ".ckpt")
        self.third.save_checkpoint(self.ckpt)
        self.ckpt_state = self.third.state(self.own)
        self.third.set_state(self.posm0, self.vel0)
        self.K = self.t_wait = self.t_idle = None
        self.failure = None

    def fresh(self, **kw):
        e = self.nb.NBodyEngine(self.n, precision=self.precision, **kw)
        e.set_state(self.posm0, self.vel0)
        return e

    def close(self):
        for e in (self.settled, self.busy, self.third):
            e.close()

    @property
    def tag(self):
        return (f"{self.key}: n = {self.n}, K = {self.K}, t_wait = {1e3 * (self.t_wait or 0):.2f} ms, "
                f"t_idle = {1e3 * (self.t_idle or 0):.3f} ms")

    def load(self, e, k=None):
        (e.hermite_step if self.hermite else e.step)(DT, self.K if k is None else k)

    def reset(self):
        for e in (self.settled, self.busy):
            e.synchronize()
            if self.plain32 and e.tracer_count:
                e.set_tracers(np.zeros((0, 3), np.float32))
            if self.f64 and e.tracer_count_f64:
                e.set_tracers_f64(None)
            e.set_state(self.posm0, self.vel0)

    def size_k(self, ops):
        """t_idle: the slowest call under test, idle, on the settled twin (its second run: the first one allocates).  K: doubled from 64
        until synchronize() right behind the load takes 10 t_idle and 50 ms; the cap is a failure."""
        t_idle = 0.0
        for name, op in ops:
            for _ in range(2):
                self.load(self.settled, 1)                         # (what every call under test follows; hermite_state needs its cache)
                self.settled.synchronize()
                t0 = time.perf_counter()
                op(self, self.settled)
                t = time.perf_counter() - t0
            t_idle = max(t_idle, t)
        self.t_idle = t_idle
        self.reset()
        k = K_FIRST
        while True:
            self.load(self.third, k)
            t0 = time.perf_counter()
            self.third.synchronize()
            self.t_wait = time.perf_counter() - t0
            self.K = k
            if self.t_wait >= max(WAIT_FACTOR * t_idle, WAIT_MIN):
                return True
            if k >= K_CAP:
                self.failure = "the host does not get far enough ahead of the device: " + self.tag
                return False
            k *= 2

    def pair(self, op, prepare=None):
        """op on the settled twin (load, wait, call) and on the busy one (load, call): their results."""
        self.reset()
        out = []
        for e, settle in ((self.settled, True), (self.busy, False)):
            if prepare:
                prepare(self, e)
            self.load(e)
            if settle:
                e.synchronize()
            out.append(op(self, e))
        return out

    def everything(self, e):
        """the state a context holds, in its own type, and what it counts"""
        out = {"state": e.state(self.own), "steps_done": e.steps_done()}
        if self.plain32 and e.tracer_count:
            out["tracers"] = e.tracers()
        if self.f64 and e.tracer_count_f64:
            out["tracers_f64"] = e.tracers_f64()
        return out

    def assert_twins_equal(self, settled, busy, what):
        a, b = self.everything(settled), self.everything(busy)
        assert a["steps_done"] == b["steps_done"], f"{what}: steps_done {b['steps_done']} != {a['steps_done']} ({self.tag})"
        for name, x, y in zip(("posm", "vel", "acc"), a["state"], b["state"]):
            differ = int((x.view(np.uint8) != y.view(np.uint8)).reshape(x.shape[0], -1).any(axis=1).sum())
            assert differ == 0, f"{what}: {name} of the busy twin differs from the settled twin's in {differ} of {x.shape[0]} rows ({self.tag})"
        assert flat(a) == flat(b), f"{what}: the twins' tracers differ ({self.tag})"


# ---- the calls under test ------------------------------------------------------------------------------------------------------------
# readers: fn(rig, e) -> what the call returned

def r_tick(pinned):
    def fn(rig, e):
        out = rig.mirror[id(e)] if pinned else np.zeros(rig.n, rig.nb.PARTICLE_DTYPE)
        size, rec = e.tick(DT, out)
        return size, rec.copy()
    return fn


def r_save(rig, e):
    path = os.path.join(rig.tmp, f"{rig.key}-{id(e)}.out.ckpt")
    e.save_checkpoint(path)
    with open(path, "rb") as f:
        return f.read()


EVERY, PLAIN32, F64, HERMITE = "every", "plain32", "f64", "hermite"
READERS = {
    "state": (EVERY, lambda rig, e: e.state(rig.own)),
    "state_other_type": (EVERY, lambda rig, e: e.state(rig.other)),
    "positions": (EVERY, lambda rig, e: e.positions()),
    "particles": (EVERY, lambda rig, e: e.particles()),
    "tick_pinned": (EVERY, r_tick(True)),
    "tick_unpinned": (EVERY, r_tick(False)),
    "bounds": (EVERY, lambda rig, e: e.bounds()),
    "energy": (EVERY, lambda rig, e: e.energy()),
    "moments": (EVERY, lambda rig, e: e.moments()),
    "mass_within": (EVERY, lambda rig, e: e.mass_within((1.5, -2.5, 0.25), np.linspace(0.0, 500.0, 9))),
    "jerk": (EVERY, lambda rig, e: e.jerk()),
    "save_checkpoint": (EVERY, r_save),
    "energy_fast": (PLAIN32, lambda rig, e: e.energy_fast()),
    "potentials": (PLAIN32, lambda rig, e: e.potentials()),
    "tidal": (PLAIN32, lambda rig, e: e.tidal()),
    "field_at": (PLAIN32, lambda rig, e: e.field_at(rig.points[:700].astype(np.float32))),
    "potential_at": (PLAIN32, lambda rig, e: e.potential_at(rig.points[:700].astype(np.float32))),
    "tracers": (PLAIN32, lambda rig, e: e.tracers()),
    "potentials_f64": (F64, lambda rig, e: e.potentials_f64()),
    "nearest_f64": (F64, lambda rig, e: e.nearest_f64()),
    "neighbours_f64": (F64, lambda rig, e: e.neighbours_f64(6)),
    "radial_order_f64": (F64, lambda rig, e: e.radial_order_f64((0.5, -0.25, 0.125))),
    "groups_f64": (F64, lambda rig, e: e.groups_f64(8.0)),
    "jerk_f64": (F64, lambda rig, e: e.jerk(np.float64)),
    "snap": (F64, lambda rig, e: e.snap()),
    "tracers_f64": (F64, lambda rig, e: e.tracers_f64()),
    "hermite_state": (HERMITE, lambda rig, e: e.hermite_state()),     # (a step() load leaves no Hermite cache to read)
}


def set_some_tracers(rig, e):
    pts = rig.points[:300]
    if rig.f64:
        e.set_tracers_f64(pts, 0.01 * pts[::-1])
    else:
        e.set_tracers(pts.astype(np.float32), (0.01 * pts[::-1]).astype(np.float32))


PREPARE = {"tracers": set_some_tracers, "tracers_f64": set_some_tracers}


# writers: fn(rig, e) -> what the context must hold afterwards: p, v, a as [n, 4] of the context's type (None: whatever the settled
# twin holds), steps (None: as before the call)

def w_set_state(other):
    def fn(rig, e):
        t = rig.other if other else rig.own
        p, v = (x.astype(t) for x in rig.new64)
        if other:
            v[:, 3] = 7.25 + np.arange(rig.n)                      # a converting upload clears the unused fourth component (one of the caller's
        e.set_state(p, v)                                          # own type is taken as it is: nbody.h calls that component unused)
        want_v = v.astype(rig.own)
        want_v[:, 3] = 0.0
        return dict(p=p.astype(rig.own), v=want_v, a=np.zeros((rig.n, 4), rig.own), steps=0)
    return fn


def w_particles(push):
    def fn(rig, e):
        q = np.zeros(rig.n, rig.nb.PARTICLE_DTYPE)
        p, v = (x.astype(np.float32) for x in rig.new64)
        q["Mass"], q["Position"], q["Velocity"], q["Acceleration"] = p[:, 3], p[:, :3], v[:, :3], rig.acc_in
        (e.push_particles if push else e.set_particles)(q)
        return dict(p=p.astype(rig.own), v=four(v[:, :3], np.float32).astype(rig.own), a=four(rig.acc_in, np.float32).astype(rig.own),
                    steps=None if push else 0)
    return fn


def w_load_checkpoint(rig, e):
    assert e.load_checkpoint(rig.ckpt) == 5
    p, v, a = rig.ckpt_state
    return dict(p=p, v=v, a=a, steps=5)


def w_set_tracers(rig, e):
    set_some_tracers(rig, e)
    pts = rig.points[:300]
    if rig.f64:
        p, v = e.tracers_f64()
        assert p.tobytes() == pts.tobytes() and v.tobytes() == (0.01 * pts[::-1]).tobytes(), rig.tag
    else:
        p, v, a = e.tracers()
        assert p.tobytes() == four(pts, np.float32).tobytes() and v.tobytes() == four(0.01 * pts[::-1], np.float32).tobytes(), rig.tag
        assert not a.any(), rig.tag
    return dict(p=None, v=None, a=None, steps=None)


def w_hermite_restart(rig, e):
    e.hermite_restart()
    return dict(p=None, v=None, a=None, steps=None)


def w_theta(rig, e):
    e.set_theta(1.0)
    e.set_theta(0.0)
    return dict(p=None, v=None, a=None, steps=None)


WRITERS = {
    "set_state_own_type": (EVERY, w_set_state(False)),
    "set_state_other_type": (EVERY, w_set_state(True)),
    "set_particles": (EVERY, w_particles(False)),
    "push_particles": (EVERY, w_particles(True)),
    "load_checkpoint": (EVERY, w_load_checkpoint),
    "set_tracers": (PLAIN32, w_set_tracers),
    "set_tracers_f64": (F64, w_set_tracers),
    "hermite_restart": (F64, w_hermite_restart),
    "set_theta_and_back": (PLAIN32, w_theta),
}


def applies(key, where):
    spec = SHAPES[key]
    return {EVERY: True, PLAIN32: spec["precision"] == "f32", F64: spec["precision"] == "f64",
            HERMITE: spec["load"] == "hermite"}[where]


def cases(table):
    return [(key, name) for key in SHAPES for name, (where, _) in table.items() if applies(key, where)]


# ---- the rigs: one per shape for the module ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rigs(nb, tmp_path_factory):
    made = {}
    tmp = str(tmp_path_factory.mktemp("streams"))

    def get(key):
        if key not in made:
            ns = [SHAPES[key]["n"]] + list(SHAPES[key]["grow"])
            kernel = None
            for n in ns:
                rig = Rig(nb, key, n, tmp)
                kernel = kernel or rig.kernel
                assert rig.kernel == kernel, f"{key}: at n = {n} the force kernel is {rig.kernel}, at n = {ns[0]} it is {kernel}"
                ops = [(name, fn) for table in (READERS, WRITERS) for name, (where, fn) in table.items()
                       if applies(key, where) and name not in PREPARE]
                if rig.size_k(ops) or n == ns[-1]:
                    break
                rig.close()                                        # the host cannot get ahead at this n: the next one, for this shape only
            made[key] = rig
            print(f"\n[streams] {rig.tag}")
        if made[key].failure:
            pytest.fail(made[key].failure)
        return made[key]

    yield get
    for rig in made.values():
        rig.close()


# ---- part A ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,name", cases(READERS))
def test_a_reader_behind_a_load_returns_what_the_settled_twin_returns(rigs, key, name):
    rig = rigs(key)
    settled, busy = rig.pair(READERS[name][1], PREPARE.get(name))
    assert flat(settled) == flat(busy), f"{name}: the busy twin's result differs from the settled twin's ({rig.tag})"
    rig.assert_twins_equal(rig.settled, rig.busy, name)


def check_written(rig, e, want, steps_before, what):
    p, v, a = e.state(rig.own)
    for name, got, exp in (("posm", p, want["p"]), ("vel", v, want["v"]), ("acc", a, want["a"])):
        if exp is None:
            continue
        wrong = int((got.view(np.uint8) != np.ascontiguousarray(exp).view(np.uint8)).reshape(rig.n, -1).any(axis=1).sum())
        assert wrong == 0, f"{what}: {name} is not what was uploaded in {wrong} of {rig.n} rows ({rig.tag})"
    steps = steps_before if want["steps"] is None else want["steps"]
    assert e.steps_done() == steps, f"{what}: steps_done = {e.steps_done()}, expected {steps} ({rig.tag})"


def writer_on_twins(rig, settled, busy, fn, what):
    for e, settle in ((settled, True), (busy, False)):
        rig.load(e)
        before = e.steps_done()                                    # (the host's count: no wait)
        if settle:
            e.synchronize()
        want = fn(rig, e)
        check_written(rig, e, want, before, f"{what} ({'settled' if settle else 'busy'} twin)")
    rig.assert_twins_equal(settled, busy, what)
    for e in (settled, busy):
        e.step(DT, 3)
        if rig.f64:
            e.hermite_step(DT, 2)
    rig.assert_twins_equal(settled, busy, what + ", then three more steps")


@pytest.mark.parametrize("key,name", cases(WRITERS))
def test_a_writer_behind_a_load_leaves_what_it_was_given(rigs, key, name):
    rig = rigs(key)
    rig.reset()
    writer_on_twins(rig, rig.settled, rig.busy, WRITERS[name][1], name)


@pytest.mark.parametrize("key", list(SHAPES))
def test_bind_device_state_behind_a_load(rigs, key):
    """nbody_bind_device_state onto pre-filled caller buffers: the steps in flight end in the context's own buffers, the bound ones hold
    what the caller put there.  (Fresh twins: a bound position buffer ends the buffer-swapping and the fused step for good.)"""
    rig = rigs(key)
    settled, busy = rig.fresh(), rig.fresh()
    p, v = (x.astype(rig.own) for x in rig.new64)
    a = four(rig.acc_in, rig.own)
    # made and filled BEFORE the load, a set per twin: DeviceBuffer waits for the whole device, and nothing between the busy twin's load
    # and its bind may
    buffers = {id(e): [DeviceBuffer(x) for x in (p, v, a)] for e in (settled, busy)}

    def bind(rig, e):
        e.bind_device_state(*buffers[id(e)])
        return dict(p=p, v=v, a=a, steps=None)

    try:
        writer_on_twins(rig, settled, busy, bind, "bind_device_state")
    finally:
        settled.close(); busy.close()


@pytest.mark.parametrize("variant", ["f32", "f32-tracers", "f64"])
def test_staging_that_grows_behind_a_load(rigs, variant):
    """A query behind the load that needs larger partial rows (ensure_probe_part) and a larger staging pair (ensure_stage: the points
    and results of every point query, the records of particles()) than any call before it — also with fp32 tracers, whose pass in the
    load reads the partial rows.  By the code both wait for the stream before they free, and the staging pair is moreover only used by
    calls that wait for their own work before they return; this confirms the order, on contexts that have made only small calls."""
    rig = rigs("f64-2000" if variant == "f64" else "f32-2000")
    twins = [rig.fresh(), rig.fresh()]
    small, big = rig.points[:8], rig.points
    got = []
    try:
        for e, settle in zip(twins, (True, False)):
            if variant == "f32-tracers":
                set_some_tracers(rig, e)
            out = [e.positions(count=1)]
            out.append(e.neighbours_at_f64(small, 6) if rig.f64 else e.potential_at(small.astype(np.float32)))
            rig.load(e)
            if settle:
                e.synchronize()
            out.append(e.neighbours_at_f64(big, 6) if rig.f64 else e.potential_at(big.astype(np.float32)))
            if variant != "f32-tracers":                           # (the staging pair has nothing to do with tracers, whose loads take twice as long)
                rig.load(e)
                if settle:
                    e.synchronize()
                out.append(e.particles())
            got.append(out)
        assert flat(got[0]) == flat(got[1]), f"{variant}: the busy twin's results differ from the settled twin's ({rig.tag})"
        rig.assert_twins_equal(twins[0], twins[1], variant)
    finally:
        for e in twins:
            e.close()


# ---- part B ------------------------------------------------------------------------------------------------------------------------------

def test_a_callers_stream_in_a_child_process():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "stream_worker.py")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    for precision in ("f32", "f64"):
        for check in ("torch to engine", "engine to torch", "switching back", "timers"):
            assert f"ok: {precision}: {check}" in out.stdout, out.stdout[-3000:]
