"""Fourth-order Hermite stepping of fp64 contexts — nbody_hermite_step, nbody_hermite_timescale, nbody_hermite_advance, nbody_hermite_get,
nbody_hermite_restart — against tests/hermite_ref.py, the scheme restated in numpy (tests/test_hermite_ref.py pins that yardstick on the
CPU).

A step evaluates exactly what nbody_get_jerk_f64 evaluates, and everything around the evaluation is a handful of correctly rounded fp64
operations in a documented order.  So the steps are checked BYTE FOR BYTE: a second fp64 context is loaded with numpy's predicted state,
its jerk(np.float64) supplies (a1, j1), and numpy's corrector gives every bit the stepping context must hold.  The scenes are Plummer
spheres with distinct masses whose coordinates are not fp32 numbers; N = 1025 is five j-chunks of 256 bodies and three workgroups of the
jerk kernel, the last one one body deep, N = 257 a full tile and a ragged one.  Trajectories (order, adaptive steps) run on kepler(e) of
hermite_ref.py, whose errors sit orders of magnitude above fp64 rounding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hermite_ref as H
from jerk_ref import direct_jerk, rel

pytestmark = pytest.mark.gpu

DT = 1e-3
_scenes = {}


def scene(nb, n):
    """(posm, vel) in fp64, read-only: ic_plummer's sphere with masses that all differ and coordinates that are no fp32 numbers."""
    if n not in _scenes:
        p32, v32 = nb.ic_plummer(n, seed=n)
        posm, vel = p32.astype(np.float64), v32.astype(np.float64)
        posm[:, :3] += 1e-7 * posm[:, :3] ** 2 + 1e-9
        vel[:, :3] += 1e-7 * vel[:, :3] ** 2 + 1e-9
        posm[:, 3] *= 1.0 + 0.5 * np.arange(n) / n + 1e-9 * np.arange(n)
        vel[:, 3] = 0.0
        assert (posm[:, :3].astype(np.float32) != posm[:, :3]).all() and len(np.unique(posm[:, 3])) == n
        posm.setflags(write=False); vel.setflags(write=False)
        _scenes[n] = (posm, vel)
    return _scenes[n]


def f64(nb, n, **kw):
    return nb.NBodyEngine(n, precision="f64", **kw)


def evaluator(b):
    """hermite_ref's `evaluate` on a second context: upload, then nbody_get_jerk_f64."""
    def evaluate(posm, vel):
        b.set_state(posm, vel)
        return b.jerk(np.float64)
    return evaluate


def snapshot(e):
    """Everything a Hermite step writes, as bytes: positions, velocities, accelerations, the cache."""
    p, v, a = e.state(np.float64)
    return (p.tobytes(), v.tobytes(), a.tobytes()) + tuple(x.tobytes() for x in e.hermite_state())


def expected(ref):
    acc = np.zeros_like(ref.posm)
    acc[:, :3] = ref.a0
    return (ref.posm.tobytes(), ref.vel.tobytes(), acc.tobytes(), ref.a0.tobytes(), ref.j0.tobytes(), ref.a2.tobytes(), ref.a3.tobytes())


NAMES = ("positions", "velocities", "accelerations", "a0", "j0", "a2", "a3")


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g == w, f"{what}: {name} differ"


def raises(nb, code, call):
    with pytest.raises(nb.NBodyError) as er:
        call()
    assert er.value.code == code, (er.value.code, str(er.value))
    return str(er.value)


# ---- 1: every bit of three chained steps ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,eps", [(1025, 0.0), (1025, 0.05), (257, 0.0), (257, 0.05)])
def test_three_chained_steps_in_every_bit(nb, n, eps):
    posm, vel = scene(nb, n)
    with f64(nb, n, eps=eps) as a, f64(nb, n, eps=eps) as b, f64(nb, n, eps=eps) as a3:
        a.set_state(posm, vel)
        ref = H.Hermite(posm, vel, evaluate=evaluator(b))
        for s in range(3):
            a.hermite_step(DT, 1)
            ref.step(DT)
            same(snapshot(a), expected(ref), f"N={n} eps={eps} step {s + 1}")
            assert a.steps_done() == s + 1
        assert ref.evaluations == 4
        assert (ref.posm[:, :3] != posm[:, :3]).all() and ref.a2.any() and ref.a3.any()
        a3.set_state(posm, vel)
        a3.hermite_step(DT, 3)
        same(snapshot(a3), expected(ref), f"N={n} eps={eps} three steps in one call")
        assert a3.steps_done() == 3
        a3.hermite_step(0.0, 5); a3.hermite_step(-1.0, 5); a3.hermite_step(DT, 0)        # no-ops, like nbody_step's
        same(snapshot(a3), expected(ref), "no-op calls")
        assert a3.steps_done() == 3


# ---- 2: one pass per step --------------------------------------------------------------------------------------------------------------

def test_one_jerk_pass_per_step(nb):
    n = 257
    posm, vel = scene(nb, n)
    F, U = nb._lib.KERNEL_FORCES, nb._lib.KERNEL_UPDATE
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0, u0 = e.kernel_time(F)[1], e.kernel_time(U)[1]
        e.hermite_step(DT, 3)
        f1, u1 = e.kernel_time(F)[1], e.kernel_time(U)[1]
        assert (f1 - f0, u1 - u0) == (4, 3)                        # the first step evaluates (a0, j0) as well
        e.hermite_step(DT, 2)
        f2, u2 = e.kernel_time(F)[1], e.kernel_time(U)[1]
        assert (f2 - f1, u2 - u1) == (2, 2)
        assert e.hermite_timescale()[2] == 1                       # from the cache: no pass
        assert e.kernel_time(F)[1] == f2
        assert e.kernel_time(F)[0] > 0 and e.kernel_time(U)[0] > 0


# ---- 3: order four -----------------------------------------------------------------------------------------------------------------------

def closing_error(e, start, a=100.0):
    return float(np.abs(e.state(np.float64)[0][:, :3] - start[:, :3]).max() / a)


def test_order_four_on_the_circular_orbit(nb):
    posm, vel, period = H.kepler(0.0)
    err = {}
    for steps in (64, 128, 256, 512):
        with f64(nb, 2) as e:
            e.set_state(posm, vel)
            e.hermite_step(period / steps, steps)
            err[steps] = closing_error(e, posm)
    ratios = [err[s] / err[2 * s] for s in (64, 128, 256)]
    print("errors", err, "ratios", ratios)
    assert all(15.0 <= r <= 17.5 for r in ratios), (err, ratios)
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        e.step(period / 256, 256)
        kick_drift = closing_error(e, posm)
    print(f"256 steps: hermite {err[256]:.3e}, kick-drift {kick_drift:.3e}")
    assert err[256] < kick_drift / 1000


# ---- 4: adaptive steps -------------------------------------------------------------------------------------------------------------------

def test_adaptive_steps_on_an_eccentric_orbit(nb):
    posm, vel, period = H.kepler(0.9)
    ref = H.Hermite(posm, vel)
    _, ref_steps, _ = ref.advance(period, eta=0.01, eta_start=0.01, dt_max=period / 16)
    assert ref_steps == 242
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        t_done, steps = e.hermite_advance(period, eta=0.01, eta_start=0.01, dt_max=period / 16)
        err = closing_error(e, posm)
        assert e.steps_done() == steps
    assert t_done == period and abs(steps - ref_steps) <= 3
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        e.hermite_step(period / steps, steps)
        fixed = closing_error(e, posm)
    print(f"{steps} steps: adaptive {err:.3e}, fixed {fixed:.3e}")
    assert err < fixed / 100
    with f64(nb, 2) as e:                                          # one step per call: the cache carries from call to call
        e.set_state(posm, vel)
        t, dts = 0.0, []
        while t < period:
            got, one = e.hermite_advance(period - t, eta=0.01, eta_start=0.01, dt_max=period / 16, max_steps=1)
            assert one == 1 and got > 0
            dts.append(got)
            t = period if got == period - t else t + got
            assert len(dts) < 1000
        assert abs(len(dts) - ref_steps) <= 3 and e.steps_done() == len(dts)
        assert e.hermite_advance(0.0) == (0.0, 0) and e.hermite_advance(1.0, max_steps=0) == (0.0, 0)
    assert max(dts) > 100 * dts[1], (max(dts), dts[1])


# ---- 5: the time scale -------------------------------------------------------------------------------------------------------------------

def test_timescale(nb):
    n = 1025
    posm, vel = scene(nb, n)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        before = snapshot_state(e)
        t, body, kind = e.hermite_timescale()
        assert kind == 0 and (t, body) == e.jerk_time()            # bitwise: the same reduction over the same vectors
        a0, j0, a2, a3 = e.hermite_state()
        assert a0.tobytes() == e.jerk(np.float64)[0].tobytes() and not a2.any() and not a3.any()
        assert snapshot_state(e) == before                         # nothing a getter shows has changed
        e.hermite_step(DT, 1)
        t, body, kind = e.hermite_timescale()
        assert (t, body, kind) == e.hermite_timescale()
        state = e.hermite_state()
        only_t, only_body, only_kind = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        f = e._L.nbody_hermite_timescale
        assert f(e._h, ctypes.byref(only_t), None, None) == 0 and only_t.value == t
        assert f(e._h, None, ctypes.byref(only_body), None) == 0 and only_body.value == body
        assert f(e._h, None, None, ctypes.byref(only_kind)) == 0 and only_kind.value == kind
    k = np.sort(H.aarseth_k(*state))
    assert k[-2] < k[-1] * (1 - 1e-12)                             # the runner-up is not within rounding of the maximum
    t_ref, body_ref, _ = H.timescale(*state)
    print(f"hermite_timescale N={n}: t {t:.17g} body {body} (numpy {t_ref:.17g} body {body_ref})")
    assert kind == 1 and body == body_ref
    assert abs(t - t_ref) <= 1e-14 * t_ref
    with f64(nb, 1) as e:
        e.set_state(np.array([[1.0, 2.0, 3.0, 4.0]]), np.array([[0.1, 0.2, 0.3, 0.0]]))
        assert e.hermite_timescale() == (float("inf"), 0, 0)
        e.hermite_step(DT, 1)
        assert e.hermite_timescale() == (float("inf"), 0, 1)


def snapshot_state(e):
    p, v, a = e.state(np.float64)
    return p.tobytes(), v.tobytes(), a.tobytes(), e.steps_done()


# ---- 6: invalidation and resume ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["set_state", "step", "device_ptr_posm", "device_ptr_vel", "hermite_restart"])
def test_a_step_behind_an_invalidation_starts_from_a_fresh_evaluation(nb, how):
    n = 257
    posm, vel = scene(nb, n)
    with f64(nb, n) as e, f64(nb, n) as fresh:
        e.set_state(posm, vel)
        e.hermite_step(DT, 2)
        assert e.hermite_timescale()[2] == 1
        if how == "set_state":
            p, v, _ = e.state(np.float64)
            e.set_state(p, v)
        elif how == "step":
            e.step(DT, 1)
        elif how == "device_ptr_posm":
            assert e.device_ptr(nb._lib.BUF_POSM)[0]
        elif how == "device_ptr_vel":
            assert e.device_ptr(nb._lib.BUF_VEL)[0]
        else:
            e.hermite_restart()
        assert "nbody_hermite_get" in raises(nb, nb._lib.ERR_STATE, e.hermite_state)
        p, v, _ = e.state(np.float64)
        fresh.set_state(p, v)
        assert e.hermite_timescale()[2] == 0 and e.hermite_timescale() == fresh.hermite_timescale()
        e.hermite_step(DT, 1)
        fresh.hermite_step(DT, 1)
        same(snapshot(e), snapshot(fresh), how)
        # once a pointer is out every CALL evaluates anew — not every step of a call
        e.hermite_step(DT, 2)
        if how.startswith("device_ptr"):
            fresh.hermite_restart()
        fresh.hermite_step(DT, 2)
        same(snapshot(e), snapshot(fresh), how + ", the call after")


def test_a_handed_out_pointer_costs_one_pass_per_call(nb):
    n = 257
    posm, vel = scene(nb, n)
    F = nb._lib.KERNEL_FORCES
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        e.device_ptr(nb._lib.BUF_ACC)
        f0 = e.kernel_time(F)[1]
        e.hermite_step(DT, 3)
        f1 = e.kernel_time(F)[1]
        e.hermite_step(DT, 2)
        f2 = e.kernel_time(F)[1]
        assert (f1 - f0, f2 - f1) == (4, 3)
        assert e.hermite_timescale()[2] == 0                       # the call evaluated anew: no derivatives
        assert e.kernel_time(F)[1] == f2 + 1


def test_compute_forces_leaves_the_cache_alone(nb):
    n = 257
    posm, vel = scene(nb, n)
    with f64(nb, n) as e, f64(nb, n) as other:
        for x in (e, other):
            x.set_state(posm, vel)
            x.hermite_step(DT, 2)
        cache = tuple(x.tobytes() for x in e.hermite_state())
        e.compute_forces()
        assert tuple(x.tobytes() for x in e.hermite_state()) == cache and e.hermite_timescale()[2] == 1
        e.hermite_step(DT, 1)
        other.hermite_step(DT, 1)
        same(snapshot(e), snapshot(other), "a step behind compute_forces")


def test_checkpoints_hold_no_cache_and_resume_the_trajectory(nb, tmp_path):
    n = 257
    posm, vel = scene(nb, n)
    ckpt, again = str(tmp_path / "hermite.ckpt"), str(tmp_path / "plain.ckpt")
    with f64(nb, n) as e, f64(nb, n) as resumed, f64(nb, n) as plain:
        e.set_state(posm, vel)
        e.hermite_step(DT, 3)
        e.save_checkpoint(ckpt)
        e.hermite_restart()
        e.hermite_step(DT, 3)
        assert resumed.load_checkpoint(ckpt) == 3
        resumed.hermite_step(DT, 3)
        same(snapshot(e), snapshot(resumed), "save, restart, three steps against load, three steps")
        assert e.steps_done() == resumed.steps_done() == 6
        # the file is the one a context that never stepped this way writes for that state
        assert plain.load_checkpoint(ckpt) == 3
        plain.save_checkpoint(again)
    data = open(ckpt, "rb").read()
    assert data[:8] == b"NBDYCKP2" and data == open(again, "rb").read()
    header = int.from_bytes(data[8:12], "little")
    assert len(data) == header + 3 * n * 32                       # the header and three double4 arrays: nothing else


# ---- 7: nothing else moves -----------------------------------------------------------------------------------------------------------------

def test_the_jerk_and_the_energy_after_hermite_steps(nb):
    n, eps = 257, 0.05
    posm, vel = scene(nb, n)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        e0 = sum(e.energy())
        e.hermite_step(DT, 50)
        drift = abs(sum(e.energy()) - e0)
        got = e.jerk(np.float64)
        p, v, a = e.state(np.float64)
        assert a[:, :3].tobytes() != got[0].tobytes()              # (the stored a1 is the predicted state's, the jerk() the live one's)
        cache = e.hermite_state()
        e.set_state(posm, vel)
        e.step(DT, 50)
        kick_drift = abs(sum(e.energy()) - e0)
    ra, rj = direct_jerk(p[:, :3], p[:, 3], v, p[:, :3], v, eps=eps, skip_self=True, dtype=np.longdouble)
    ea, ej = rel(got[0], ra.astype(np.float64)).max(), rel(got[1], rj.astype(np.float64)).max()
    print(f"after 50 steps: jerk() err acc {ea:.3e} jerk {ej:.3e}; |dE| hermite {drift:.3e} kick-drift {kick_drift:.3e} of {abs(e0):.3e}")
    assert ea < 1e-12 and ej < 1e-12
    assert rel(cache[0], a[:, :3]).max() == 0.0                    # NBODY_BUF_ACC is the cached a0
    assert drift < kick_drift


def test_a_single_body_moves_by_dt_v(nb):
    posm = np.array([[1.5, -2.25, 3.0000001, 7.0]]); vel = np.array([[0.1, 0.7, -0.3, 0.0]])
    dt = 0.37
    with f64(nb, 1) as e:
        e.set_state(posm, vel)
        e.hermite_step(dt, 1)
        p, v, a = e.state(np.float64)
    want = posm.copy()
    want[:, :3] = posm[:, :3] + np.float64(dt) * vel[:, :3]
    assert p.tobytes() == want.tobytes() and v.tobytes() == vel.tobytes() and not a.any()


# ---- 8: errors -------------------------------------------------------------------------------------------------------------------------------

def five_calls(e):
    return (lambda: e.hermite_step(DT, 1)), e.hermite_timescale, (lambda: e.hermite_advance(DT)), e.hermite_state, e.hermite_restart


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    """tests/cpp/fake_rccl.c, the suite's stand-in for the communication library, as tests/test_jerk_gpu.py builds it: a multi-device
    context over device 0 alone needs no real communicator to refuse a call."""
    so = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "fake_rccl.c"), "-o", so, "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return so


def test_errors(nb, fake_rccl, monkeypatch):
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
            for call in five_calls(e):
                assert why in raises(nb, E.ERR_UNSUPPORTED, call), kw
    n = 257
    posm, vel = scene(nb, n)
    with f64(nb, n) as e:
        for call in five_calls(e):                                 # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(posm, vel)
        e.step_begin()
        for call in five_calls(e):                                 # a step is open
            raises(nb, E.ERR_STATE, call)
        e.step_end(0.0)
        before = snapshot_state(e)
        for dt in (float("nan"), float("inf"), -float("inf")):
            raises(nb, E.ERR_INVALID, lambda: e.hermite_step(dt, 1))
        raises(nb, E.ERR_INVALID, lambda: e.hermite_step(DT, -1))
        for kw in ({"eta": 0.0}, {"eta": -1.0}, {"eta": float("nan")}, {"eta_start": 0.0}, {"dt_max": 0.0}, {"max_steps": -1}):
            raises(nb, E.ERR_INVALID, lambda: e.hermite_advance(DT, **kw))
        for span in (-1.0, float("inf"), float("nan")):
            raises(nb, E.ERR_INVALID, lambda: e.hermite_advance(span))
        assert e._L.nbody_hermite_timescale(e._h, None, None, None) == E.ERR_INVALID
        e.hermite_timescale()
        out = np.zeros((n, 12))
        assert e._L.nbody_hermite_get(e._h, out.ctypes.data, 95) == E.ERR_INVALID
        assert e._L.nbody_hermite_get(e._h, None, 96) == E.ERR_INVALID
        assert not out.any() and snapshot_state(e) == before
        wide = np.full((n, 13), 5.0)                               # a stride of its own
        assert e._L.nbody_hermite_get(e._h, wide.ctypes.data, 104) == 0
        assert np.ascontiguousarray(wide[:, :3]).tobytes() == e.hermite_state()[0].tobytes() and (wide[:, 12] == 5.0).all()
