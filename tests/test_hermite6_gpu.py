"""The snap pass and sixth-order Hermite stepping of fp64 contexts — nbody_get_snap_f64, nbody_hermite6_step, nbody_hermite6_timescale,
nbody_hermite6_advance, nbody_hermite6_get — against tests/hermite6_ref.py (tests/test_hermite6_ref.py pins that yardstick on the CPU).

The a and j of a snap pass are nbody_get_jerk_f64's in every bit, and everything around the evaluation is a handful of correctly rounded
fp64 operations in a documented order.  So the steps are checked BYTE FOR BYTE: a second fp64 context is loaded with numpy's predicted
state, its snap(acc_in=ap) supplies (a1, j1, s1), and numpy's corrector gives every bit the stepping context must hold.  The snap itself is
held to the project's fp64 parity bound against the long-double pair sum.  The scenes are test_hermite_gpu.py's: Plummer spheres with
distinct masses whose coordinates are not fp32 numbers; N = 1025 is five j-chunks of 256 bodies and three workgroups of the snap kernel,
the last one one body deep, N = 257 a full tile and a ragged one.  Trajectories run on kepler(e) of hermite_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hermite6_ref as H6
import hermite_ref as H
from jerk_ref import rel

pytestmark = pytest.mark.gpu

DT = 1e-3
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
LD = np.longdouble
_scenes, _refs = {}, {}


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


def given_acc(nb, n):
    """An input acceleration array that is nobody's acceleration: normal, of the scale of the scene's own."""
    posm, vel = scene(nb, n)
    a = H6.direct_snap(posm, vel, np.zeros((n, 3)))[0]
    return np.random.default_rng(1000 + n).normal(0.0, float(np.abs(a).std()), (n, 3))


def long_double_snap(nb, n, eps, given):
    """(a, j, s) of the scene as float64 roundings of the long-double pair sum, computed once per case."""
    key = (n, eps, given)
    if key not in _refs:
        posm, vel = scene(nb, n)
        _refs[key] = tuple(x.astype(np.float64) for x in H6.direct_snap(posm, vel, given_acc(nb, n) if given else None, eps=eps, dtype=LD))
    return _refs[key]


def f64(nb, n, **kw):
    return nb.NBodyEngine(n, precision="f64", **kw)


def evaluator(b):
    """hermite6_ref's `evaluate` on a second context: upload, then nbody_get_snap_f64."""
    def evaluate(posm, vel, acc_in):
        b.set_state(posm, vel)
        return b.snap(acc_in)
    return evaluate


def snapshot(e):
    """Everything a sixth-order step writes, as bytes: positions, velocities, accelerations, the cache."""
    p, v, a = e.state(np.float64)
    return (p.tobytes(), v.tobytes(), a.tobytes()) + tuple(x.tobytes() for x in e.hermite6_state())


def snapshot4(e):
    p, v, a = e.state(np.float64)
    return (p.tobytes(), v.tobytes(), a.tobytes()) + tuple(x.tobytes() for x in e.hermite_state())


def snapshot_state(e):
    p, v, a = e.state(np.float64)
    return p.tobytes(), v.tobytes(), a.tobytes(), e.steps_done()


def expected(ref):
    acc = np.zeros_like(ref.posm)
    acc[:, :3] = ref.a0
    return (ref.posm.tobytes(), ref.vel.tobytes(), acc.tobytes()) + tuple(x.tobytes() for x in (ref.a0, ref.j0, ref.s0, ref.a3, ref.a4, ref.a5))


NAMES = ("positions", "velocities", "accelerations", "a0", "j0", "s0", "a3", "a4", "a5")


def same(got, want, what):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert g == w, f"{what}: {name} differ"


def raises(nb, code, call):
    with pytest.raises(nb.NBodyError) as er:
        call()
    assert er.value.code == code, (er.value.code, str(er.value))
    return str(er.value)


class DeviceBuffer:
    """Caller-owned device memory for nbody_bind_device_state, zeroed; lives as long as the object (the engine keeps it)."""

    def __init__(self, nbytes):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), nbytes) == 0
        assert self.hip.hipMemset(self.ptr, 0, nbytes) == 0 and self.hip.hipDeviceSynchronize() == 0

    def data_ptr(self):
        return self.ptr.value

    def __del__(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = ctypes.c_void_p()


def passes(nb, e):
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]


CASES = [(1025, 0.0), (1025, 0.05), (257, 0.0), (257, 0.05)]


# ---- 1: the snap pass ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,eps", CASES)
def test_the_snap_pass(nb, n, eps):
    posm, vel = scene(nb, n)
    ain = given_acc(nb, n)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        before = snapshot_state(e)
        ja, jj = e.jerk(np.float64)
        a, j, s = e.snap()
        assert a.tobytes() == ja.tobytes() and j.tobytes() == jj.tobytes(), "a, j of the snap pass are not nbody_get_jerk_f64's bits"
        ga, gj, gs = e.snap(ain)
        assert ga.tobytes() == ja.tobytes() and gj.tobytes() == jj.tobytes(), "a, j depend on the input accelerations"
        assert gs.tobytes() != s.tobytes()
        own = e.snap(ja)
        assert own[2].tobytes() == s.tobytes() and own[0].tobytes() == ja.tobytes(), "acc_in = NULL is not the context's own jerk(np.float64)[0]"
        for given, got in ((False, (a, j, s)), (True, (ga, gj, gs))):
            ref = long_double_snap(nb, n, eps, given)
            errs = [float(rel(g, r).max()) for g, r in zip(got, ref)]
            print(f"snap N={n} eps={eps} acc_in {'given' if given else 'NULL'}: a {errs[0]:.2e} j {errs[1]:.2e} s {errs[2]:.2e}")
            assert max(errs) < TOL_F64, errs
            # (the first and the last body by name — a smoke check of the ends of the index range: a self pair has d = w = b = 0 and
            # adds nothing even at eps > 0, so what this can catch is a NEIGHBOUR dropped in a body's place, which the bound above sees too)
            ends = [float(rel(g[[0, n - 1]], r[[0, n - 1]]).max()) for g, r in zip(got, ref)]
            assert max(ends) < TOL_F64, ends
        # strides of their own, and each output NULL in turn: the same bytes
        f = e._L.nbody_get_snap_f64
        wide_in = np.full((n, 5), 9.0); wide_in[:, :3] = ain
        wide = [np.full((n, 5), 7.0) for _ in range(3)]
        assert f(e._h, wide_in.ctypes.data, 40, wide[0].ctypes.data, 40, wide[1].ctypes.data, 40, wide[2].ctypes.data, 40) == 0
        for w, g in zip(wide, (ga, gj, gs)):
            assert np.ascontiguousarray(w[:, :3]).tobytes() == g.tobytes() and (w[:, 3:] == 7.0).all()
        for skip in range(3):
            out = [np.full((n, 3), 7.0) for _ in range(3)]
            ptr = [None if k == skip else out[k].ctypes.data for k in range(3)]
            assert f(e._h, ain.ctypes.data, 24, ptr[0], 24, ptr[1], 24, ptr[2], 24) == 0
            for k, g in enumerate((ga, gj, gs)):
                assert (out[k] == 7.0).all() if k == skip else out[k].tobytes() == g.tobytes()
        assert snapshot_state(e) == before                         # nothing a getter shows has changed


# ---- 1b: a fresh context above the slab sizes ------------------------------------------------------------------------------------------

def test_a_fresh_context_whose_passes_run_in_slabs(nb):
    """N = 65536 is 128 chunks: the snap pass's partial rows go in three slabs of 25600 bodies, and the jerk pass's rows (slabs of 43008
    bodies, three float4 each) need MORE staging than the snap pass's (five float4 each) — 16 515 072 against 16 384 000 float4.  The
    stepping context's FIRST call is a sixth-order one: its start must size the staging area for both passes."""
    n = 65536
    p32, v32 = nb.ic_reference_box(n, 1000.0, seed=n)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    posm[:, :3] += 1e-7 * posm[:, :3] ** 2 + 1e-9
    vel[:, 3] = 0.0
    with f64(nb, n) as e, f64(nb, n) as other:
        e.set_state(posm, vel)
        assert e.hermite6_timescale()[2] == 0                      # nothing before it: no jerk(), no fourth-order call
        a0, j0, s0, a3, a4, a5 = e.hermite6_state()
        other.set_state(posm, vel)
        ja, jj = other.jerk(np.float64)
        assert a0.tobytes() == ja.tobytes() and j0.tobytes() == jj.tobytes(), "the slabs' a, j are not nbody_get_jerk_f64's bits"
        oa, oj, osnap = other.snap()
        assert oa.tobytes() == ja.tobytes() and oj.tobytes() == jj.tobytes() and osnap.tobytes() == s0.tobytes()
        rows = np.array([0, 1023, 25599, 25600, 25601, 43007, 43008, 51199, 51200, 65535])   # both sides of every slab boundary
        ref = H6.direct_snap(posm, vel, a0, dtype=LD, rows=rows)
        errs = [float(rel(g[rows], r.astype(np.float64)).max()) for g, r in zip((a0, j0, s0), ref)]
        print(f"snap N={n} at {len(rows)} bodies around the slab boundaries: a {errs[0]:.2e} j {errs[1]:.2e} s {errs[2]:.2e}")
        assert max(errs) < TOL_F64, errs
        e.hermite6_step(1e-4, 1)                                   # a step in slabs: the same bytes on a context that grew its staging
        other.hermite6_step(1e-4, 1)                               # area the other way round (jerk first)
        same(snapshot(e), snapshot(other), "a step at N = 65536")


# ---- 2: small cases --------------------------------------------------------------------------------------------------------------------

def test_one_body_and_coincident_bodies(nb):
    with f64(nb, 1) as e:
        e.set_state(np.array([[1.0, 2.0, 3.0, 4.0]]), np.array([[0.1, 0.2, 0.3, 0.0]]))
        assert not any(x.any() for x in e.snap()) and not any(x.any() for x in e.snap(np.array([[5.0, 6.0, 7.0]])))
    posm = np.array([[1.0, 2.0, 3.0, 5.0], [1.0, 2.0, 3.0, 7.0], [4.0, -1.0, 0.5, 11.0]])
    vel = np.array([[0.1, 0.2, 0.3, 0.0], [-0.3, 0.1, 0.0, 0.0], [0.0, 0.5, -0.2, 0.0]])
    ain = np.array([[1.0, -2.0, 0.5], [0.25, 0.0, -1.0], [3.0, 1.0, 1.0]])
    for eps in (0.0, 0.5):
        with f64(nb, 3, eps=eps) as e, f64(nb, 2, eps=eps) as lone:
            e.set_state(posm, vel)
            got = e.snap(ain)
            for k, other in ((0, 1), (1, 0)):
                lone.set_state(np.delete(posm, other, 0), np.delete(vel, other, 0))
                want = lone.snap(np.delete(ain, other, 0))
                assert got[0][k].tobytes() == want[0][0].tobytes()   # d == 0: nothing in a, at either eps
                if eps == 0.0:                                      # the pair is dropped from all nine sums: exactly 0 is added
                    assert got[1][k].tobytes() == want[1][0].tobytes() and got[2][k].tobytes() == want[2][0].tobytes()
                else:                                               # the twin is felt: q w in the jerk, q b in the snap
                    q = H6.G * posm[other, 3] / eps ** 3
                    assert np.allclose(got[1][k] - want[1][0], q * (vel[other, :3] - vel[k, :3]), rtol=1e-12, atol=0)
                    assert np.allclose(got[2][k] - want[2][0], q * (ain[other] - ain[k]), rtol=1e-12, atol=0)
            ref = H6.direct_snap(posm, vel, ain, eps=eps, dtype=LD)
            assert max(float(rel(g, r.astype(np.float64)).max()) for g, r in zip(got, ref)) < TOL_F64


# ---- 3: every bit of three chained steps -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,eps", CASES)
def test_three_chained_steps_in_every_bit(nb, n, eps):
    posm, vel = scene(nb, n)
    with f64(nb, n, eps=eps) as a, f64(nb, n, eps=eps) as b, f64(nb, n, eps=eps) as a3:
        a.set_state(posm, vel)
        ref = H6.Hermite6(posm, vel, evaluate=evaluator(b))
        for s in range(3):
            a.hermite6_step(DT, 1)
            ref.step(DT)
            same(snapshot(a), expected(ref), f"N={n} eps={eps} step {s + 1}")
            assert a.steps_done() == s + 1
        assert ref.evaluations == 4
        assert (ref.posm[:, :3] != posm[:, :3]).all() and ref.a3.any() and ref.a4.any() and ref.a5.any()
        a3.set_state(posm, vel)
        a3.hermite6_step(DT, 3)
        same(snapshot(a3), expected(ref), f"N={n} eps={eps} three steps in one call")
        assert a3.steps_done() == 3
        a3.hermite6_step(0.0, 5); a3.hermite6_step(-1.0, 5); a3.hermite6_step(DT, 0)     # no-ops, like nbody_step's
        same(snapshot(a3), expected(ref), "no-op calls")
        assert a3.steps_done() == 3


# ---- 4: one snap pass per step -----------------------------------------------------------------------------------------------------------

def test_one_snap_pass_per_step(nb):
    n = 257
    posm, vel = scene(nb, n)
    F, U = nb._lib.KERNEL_FORCES, nb._lib.KERNEL_UPDATE
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0, u0 = passes(nb, e)
        e.hermite6_step(DT, 3)
        f1, u1 = passes(nb, e)
        assert (f1 - f0, u1 - u0) == (2 + 3, 3)                    # the start: one jerk pass for a, one snap pass for (a0, j0, s0)
        e.hermite6_step(DT, 2)
        f2, u2 = passes(nb, e)
        assert (f2 - f1, u2 - u1) == (2, 2)
        assert e.hermite6_timescale()[2] == 1                      # from the cache: no pass
        assert passes(nb, e) == (f2, u2)
        assert e.kernel_time(F)[0] > 0 and e.kernel_time(U)[0] > 0
        e.snap()                                                   # acc_in = NULL: the jerk pass and the snap pass
        assert passes(nb, e) == (f2 + 2, u2)
        e.snap(np.zeros((n, 3)))
        assert passes(nb, e) == (f2 + 3, u2)


# ---- 5: order six ------------------------------------------------------------------------------------------------------------------------

def closing_error(e, start, a=100.0):
    return float(np.abs(e.state(np.float64)[0][:, :3] - start[:, :3]).max() / a)


def test_order_six_on_the_circular_orbit(nb):
    posm, vel, period = H.kepler(0.0)
    err = {}
    for steps in (16, 32, 64, 128):                                # 256 steps and beyond approach rounding: left out on purpose
        with f64(nb, 2) as e:
            e.set_state(posm, vel)
            e.hermite6_step(period / steps, steps)
            err[steps] = closing_error(e, posm)
    ratios = [err[s] / err[2 * s] for s in (16, 32, 64)]
    print("errors", err, "ratios", ratios)
    assert all(60.0 <= r <= 68.0 for r in ratios), (err, ratios)
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        e.hermite_step(period / 256, 256)
        four = closing_error(e, posm)
    print(f"sixth order at 64 steps {err[64]:.3e}, fourth order at 256 steps {four:.3e}")
    assert err[64] < four


# ---- 6: the time scale and the adaptive driver ---------------------------------------------------------------------------------------------

def test_timescale(nb):
    n = 1025
    posm, vel = scene(nb, n)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        before = snapshot_state(e)
        t, body, kind = e.hermite6_timescale()
        assert kind == 0 and (t, body) == e.jerk_time()            # bitwise: the same reduction over the same vectors
        a0, j0, s0, a3, a4, a5 = e.hermite6_state()
        got = e.snap()
        assert all(x.tobytes() == y.tobytes() for x, y in zip((a0, j0, s0), got)) and not a3.any() and not a4.any() and not a5.any()
        assert snapshot_state(e) == before                         # nothing a getter shows has changed
        e.hermite6_step(DT, 1)
        t, body, kind = e.hermite6_timescale()
        assert (t, body, kind) == e.hermite6_timescale()
        state = e.hermite6_state()
        only_t, only_body, only_kind = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        f = e._L.nbody_hermite6_timescale
        assert f(e._h, ctypes.byref(only_t), None, None) == 0 and only_t.value == t
        assert f(e._h, None, ctypes.byref(only_body), None) == 0 and only_body.value == body
        assert f(e._h, None, None, ctypes.byref(only_kind)) == 0 and only_kind.value == kind
    k = H6.hermite6_k(*state)
    ranked = np.sort(k)
    assert ranked[-2] < ranked[-1] * (1 - 1e-12)                   # the runner-up is not within rounding of the maximum
    t_ref, body_ref, _ = H6.timescale(*state)
    print(f"hermite6_timescale N={n}: t {t:.17g} body {body} (numpy {t_ref:.17g} body {body_ref})")
    assert kind == 1 and body == body_ref == int(np.argmax(k))
    assert abs(t - t_ref) <= 4 * np.spacing(t_ref)                 # cbrt is not correctly rounded: 4 ulp
    with f64(nb, 1) as e:
        e.set_state(np.array([[1.0, 2.0, 3.0, 4.0]]), np.array([[0.1, 0.2, 0.3, 0.0]]))
        assert e.hermite6_timescale() == (float("inf"), 0, 0)
        e.hermite6_step(DT, 1)
        assert e.hermite6_timescale() == (float("inf"), 0, 1)


REF_STEPS = 70                                                     # hermite6_ref on kepler(0.9), eta = 0.5 (test_hermite6_ref.py pins it)


def test_adaptive_steps_on_an_eccentric_orbit(nb):
    posm, vel, period = H.kepler(0.9)
    kw = dict(eta=0.5, eta_start=0.01, dt_max=period / 16)
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        t_done, steps = e.hermite6_advance(period, **kw)
        err = closing_error(e, posm)
        assert e.steps_done() == steps
    assert t_done == period and abs(steps - REF_STEPS) <= 3
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        _, steps4 = e.hermite_advance(period, eta=0.01, eta_start=0.01, dt_max=period / 16)
        err4 = closing_error(e, posm)
    print(f"sixth order: {steps} steps, {err:.3e}; fourth order: {steps4} steps, {err4:.3e}")
    assert 2 * steps < steps4 and err <= err4
    with f64(nb, 2) as e:                                          # one step per call: the cache carries from call to call
        e.set_state(posm, vel)
        t, dts = 0.0, []
        while t < period:
            got, one = e.hermite6_advance(period - t, max_steps=1, **kw)
            assert one == 1 and got > 0
            dts.append(got)
            t = period if got == period - t else t + got
            assert len(dts) < 1000
        assert abs(len(dts) - REF_STEPS) <= 3 and e.steps_done() == len(dts)
        assert e.hermite6_advance(0.0) == (0.0, 0) and e.hermite6_advance(1.0, max_steps=0) == (0.0, 0)
    assert max(dts) > 50 * dts[1], (max(dts), dts[1])


# ---- 7: living with the other integrators --------------------------------------------------------------------------------------------------

INVALIDATIONS = ["nothing", "set_state", "set_particles", "push_particles", "step", "step_end", "tick", "device_ptr_posm", "device_ptr_acc",
                 "bind_device_state", "hermite_restart", "load_checkpoint", "hermite_step", "hermite_advance", "hermite_block_begin"]
EXTERNAL = ("device_ptr_posm", "device_ptr_acc", "bind_device_state")   # somebody else may write the state from then on


@pytest.mark.parametrize("how", INVALIDATIONS)
def test_a_step_behind_an_invalidation_evaluates_anew(nb, how, tmp_path):
    n = 257
    posm, vel = scene(nb, n)
    with f64(nb, n, time_kernels=True) as e, f64(nb, n) as fresh:
        e.set_state(posm, vel)
        e.hermite6_step(DT, 2)
        assert e.hermite6_timescale()[2] == 1
        if how == "set_state":
            p, v, _ = e.state(np.float64)
            e.set_state(p, v)
        elif how == "set_particles":
            e.set_particles(e.particles())
        elif how == "push_particles":
            e.push_particles(e.particles())
        elif how == "step":
            e.step(DT, 1)
        elif how == "tick":
            e.tick(DT)
        elif how == "bind_device_state":
            e.bind_device_state(acc=DeviceBuffer(n * 32))
        elif how == "step_end":
            e.step_begin()
            e.step_end(DT)
        elif how.startswith("device_ptr"):
            assert e.device_ptr(nb._lib.BUF_POSM if how.endswith("posm") else nb._lib.BUF_ACC)[0]
        elif how == "hermite_restart":
            e.hermite_restart()
        elif how == "load_checkpoint":
            e.save_checkpoint(str(tmp_path / "s.ckpt"))
            e.load_checkpoint(str(tmp_path / "s.ckpt"))
        elif how == "hermite_step":
            e.hermite_step(DT, 1)
        elif how == "hermite_advance":
            e.hermite_advance(DT, max_steps=1)
        elif how == "hermite_block_begin":
            e.hermite_block_begin(DT, 0)
        if how != "nothing":
            assert "nbody_hermite6_get" in raises(nb, nb._lib.ERR_STATE, e.hermite6_state)
        p, v, _ = e.state(np.float64)
        f0 = passes(nb, e)[0]
        e.hermite6_step(DT, 1)
        f1 = passes(nb, e)[0]
        assert f1 - f0 == (1 if how == "nothing" else 3), how      # the start's two passes and the step's one
        if how != "nothing":                                       # ... from the stored state alone
            fresh.set_state(p, v)
            fresh.hermite6_step(DT, 1)
            same(snapshot(e), snapshot(fresh), how)
        # once a pointer is out every CALL evaluates anew — not every step of a call
        e.hermite6_step(DT, 2)
        assert passes(nb, e)[0] - f1 == (4 if how in EXTERNAL else 2), how


def test_the_two_schemes_forget_each_others_cache(nb):
    n = 257
    posm, vel = scene(nb, n)
    with f64(nb, n) as e, f64(nb, n) as fresh:
        e.set_state(posm, vel)
        e.hermite_step(DT, 2)
        e.hermite6_step(DT, 2)                                     # starts from the stored state
        fresh.set_state(posm, vel)
        fresh.hermite_step(DT, 2)
        p, v, _ = fresh.state(np.float64)
        fresh.set_state(p, v)
        fresh.hermite6_step(DT, 2)
        same(snapshot(e), snapshot(fresh), "hermite6_step behind hermite_step")
        assert "nbody_hermite_get" in raises(nb, nb._lib.ERR_STATE, e.hermite_state)   # the fourth-order cache is gone
        p, v, _ = e.state(np.float64)
        e.hermite_step(DT, 2)                                      # and back
        fresh.set_state(p, v)
        fresh.hermite_step(DT, 2)
        assert snapshot4(e) == snapshot4(fresh), "hermite_step behind hermite6_step"
        assert "nbody_hermite6_get" in raises(nb, nb._lib.ERR_STATE, e.hermite6_state)


def test_a_block_session(nb):
    n = 257
    posm, vel = scene(nb, n)
    E = nb._lib
    with f64(nb, n) as e, f64(nb, n) as fresh:
        e.set_state(posm, vel)
        level_in = np.zeros(n, np.int32)
        level_in[n // 2] = 1                                       # one body on half steps: the first block step ends in mid-frame
        e.hermite_block_begin(0.01, 1, level_in=level_in)
        st = e.hermite_block_advance(1, max_block_steps=1)
        assert not st["synchronised"] and st["ticks"] == 1
        before = snapshot_state(e)
        for call in ((lambda: e.hermite6_step(DT, 1)), e.hermite6_timescale, (lambda: e.hermite6_advance(DT))):
            assert "mid-frame" in raises(nb, E.ERR_STATE, call)
        assert snapshot_state(e) == before
        assert e.snap()[0].tobytes() == e.jerk(np.float64)[0].tobytes()   # the getter answers on the stored state and ends nothing
        st = e.hermite_block_advance(1)
        assert st["synchronised"]
        p, v, _ = e.state(np.float64)
        e.hermite6_step(DT, 1)                                     # at a frame end: from the stored state, and the session ends
        fresh.set_state(p, v)
        fresh.hermite6_step(DT, 1)
        same(snapshot(e), snapshot(fresh), "hermite6_step at a frame end")
        assert "no block session" in raises(nb, E.ERR_STATE, lambda: e.hermite_block_advance(1))


def test_checkpoints_hold_no_cache_and_resume_the_trajectory(nb, tmp_path):
    n = 257
    posm, vel = scene(nb, n)
    ckpt, again = str(tmp_path / "hermite6.ckpt"), str(tmp_path / "plain.ckpt")
    with f64(nb, n) as e, f64(nb, n) as resumed, f64(nb, n) as plain:
        e.set_state(posm, vel)
        e.hermite6_step(DT, 3)
        e.save_checkpoint(ckpt)
        e.hermite_restart()
        e.hermite6_step(DT, 3)
        assert resumed.load_checkpoint(ckpt) == 3
        resumed.hermite6_step(DT, 3)
        same(snapshot(e), snapshot(resumed), "save, restart, three steps against load, three steps")
        assert e.steps_done() == resumed.steps_done() == 6
        assert plain.load_checkpoint(ckpt) == 3
        plain.save_checkpoint(again)
    data = open(ckpt, "rb").read()
    assert data[:8] == b"NBDYCKP2" and data == open(again, "rb").read()
    header = int.from_bytes(data[8:12], "little")
    assert len(data) == header + 3 * n * 32                       # the header and three double4 arrays: nothing else


def test_the_snap_getter_leaves_both_caches_alone(nb):
    n = 257
    posm, vel = scene(nb, n)
    with f64(nb, n) as e, f64(nb, n) as other:
        for x in (e, other):
            x.set_state(posm, vel)
            x.hermite6_step(DT, 2)
            assert x.hermite_timescale()[2] == 0                   # the fourth-order cache holds (a0, j0) of the same state
        before = snapshot(e), snapshot4(e), e.steps_done()
        e.snap()
        e.snap(given_acc(nb, n))
        assert (snapshot(e), snapshot4(e), e.steps_done()) == before
        assert e.hermite6_timescale()[2] == 1 and e.hermite_timescale()[2] == 0
        e.hermite6_step(DT, 1)
        other.hermite6_step(DT, 1)
        same(snapshot(e), snapshot(other), "a step behind nbody_get_snap_f64")


def test_a_single_body_moves_by_dt_v(nb):
    posm = np.array([[1.5, -2.25, 3.0000001, 7.0]]); vel = np.array([[0.1, 0.7, -0.3, 0.0]])
    dt = 0.37
    with f64(nb, 1) as e:
        e.set_state(posm, vel)
        e.hermite6_step(dt, 1)
        p, v, a = e.state(np.float64)
    want = posm.copy()
    want[:, :3] = posm[:, :3] + np.float64(dt) * vel[:, :3]
    assert p.tobytes() == want.tobytes() and v.tobytes() == vel.tobytes() and not a.any()


# ---- 7b: the command line ------------------------------------------------------------------------------------------------------------------

def test_the_command_line_runs_both_forms(nb, tmp_path, capsys):
    import json
    from parallelnbody_amd.__main__ import main
    n, dt, frames = 257, 1e-3, 4
    base = ["--plummer", "--n", str(n), "--precision", "f64", "--integrator", "hermite6", "--energy-every", "2"]
    out = str(tmp_path / "fixed.npy")
    main(base + ["--dt", str(dt), "--steps", str(frames), "--dump-positions", out])
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x.get("frame") for x in lines[:-1]] == [2, 4] and lines[-1]["steps_done"] == frames
    posm, vel = nb.ic_plummer(n, seed=1)
    with f64(nb, n) as e:                                          # without --eta: one step of --dt per frame
        e.set_state(posm, vel)
        e.hermite6_step(dt, frames)
        assert np.load(out).tobytes() == e.positions().tobytes()
    e2, e4 = lines[0]["total"], lines[1]["total"]
    print(f"command line, fixed steps: total energy {e2!r} at frame 2, {e4!r} at frame 4")
    assert abs(e4 - e2) < 1e-6 * abs(e2), (e2, e4)             # (a frame is 1/300 of a crossing time: six orders below that)
    out = str(tmp_path / "adaptive.npy")
    main(base + ["--dt", "0.01", "--steps", "2", "--eta", "0.5", "--dump-positions", out])
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    with f64(nb, n) as e:                                          # with --eta: adaptive steps that cover --dt per frame
        e.set_state(posm, vel)
        steps = sum(e.hermite6_advance(0.01, eta=0.5)[1] for _ in range(2))
        assert np.load(out).tobytes() == e.positions().tobytes()
    assert lines[-1]["steps_done"] == steps > 2 and lines[0]["frame"] == 2


# ---- 8: errors -----------------------------------------------------------------------------------------------------------------------------

def five_calls(e):
    return e.snap, (lambda: e.hermite6_step(DT, 1)), e.hermite6_timescale, (lambda: e.hermite6_advance(DT)), e.hermite6_state


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
        for call in five_calls(e)[1:]:                             # a step is open (the getter answers like nbody_get_jerk_f64)
            raises(nb, E.ERR_STATE, call)
        e.step_end(0.0)
        before = snapshot_state(e)
        for dt in (float("nan"), float("inf"), -float("inf")):
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_step(dt, 1))
        raises(nb, E.ERR_INVALID, lambda: e.hermite6_step(DT, -1))
        for kw in ({"eta": 0.0}, {"eta": -1.0}, {"eta": float("nan")}, {"eta_start": 0.0}, {"dt_max": 0.0}, {"max_steps": -1}):
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_advance(DT, **kw))
        for span in (-1.0, float("inf"), float("nan")):
            raises(nb, E.ERR_INVALID, lambda: e.hermite6_advance(span))
        assert e._L.nbody_hermite6_timescale(e._h, None, None, None) == E.ERR_INVALID
        raises(nb, E.ERR_STATE, e.hermite6_state)                  # nothing cached yet
        e.hermite6_timescale()
        out = np.zeros((n, 18))
        assert e._L.nbody_hermite6_get(e._h, out.ctypes.data, 143) == E.ERR_INVALID
        assert e._L.nbody_hermite6_get(e._h, None, 144) == E.ERR_INVALID
        f = e._L.nbody_get_snap_f64
        o = out.ctypes.data
        assert f(e._h, None, 24, None, 24, None, 24, None, 24) == E.ERR_INVALID
        assert f(e._h, o, 23, o, 24, None, 24, None, 24) == E.ERR_INVALID
        for bad in range(3):
            strides = [23 if k == bad else 24 for k in range(3)]
            assert f(e._h, None, 24, o, strides[0], o, strides[1], o, strides[2]) == E.ERR_INVALID
        assert f(e._h, None, 0, None, 0, None, 0, o, 144) == 0     # the strides of NULL arrays are not looked at
        assert out[:, :3].tobytes() == e.snap()[2].tobytes()
        out[:] = 0.0
        assert snapshot_state(e) == before
        wide = np.full((n, 19), 5.0)                               # a stride of its own
        assert e._L.nbody_hermite6_get(e._h, wide.ctypes.data, 152) == 0
        assert np.ascontiguousarray(wide[:, :3]).tobytes() == e.hermite6_state()[0].tobytes() and (wide[:, 18] == 5.0).all()
