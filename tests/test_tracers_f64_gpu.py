"""fp64 point queries and fp64 tracers on the shared-step Hermite calls — nbody_jerk_at_f64, nbody_set_tracers_f64, nbody_get_tracers_f64,
nbody_tracer_count_f64, nbody_hermite[6]_tracers_get, nbody_hermite[6]_tracers_timescale — on the device.

THE ORACLE is a second fp64 context that holds the N bodies and, appended behind them, the M tracers as bodies of mass 0, N + M <= 32768:
up to 32768 bodies probe_geometry gives 256-body chunks to both contexts, so the real bodies fall into the same chunks in the same
order; a body of mass 0 adds fma(0, d, A) == A to every chain and the extra chunks add rows of +0; a massless body's own pair is
dropped by index there and never met here.  Every comparison called "augmented" below is therefore BYTE FOR BYTE, against kernels
tested since the jerk and snap passes exist.  The scenes are random (no massless body comes closer to anything than a normal-range
s^2); points exactly on bodies are tested separately and directly.  The long-double pair sum of tests/jerk_ref.py holds the values to
the project's fp64 parity bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hermite6_ref as H6
import hermite_ref as H
from jerk_ref import G, direct_jerk, probe_geometry, rel

pytestmark = pytest.mark.gpu

DT = 1e-3
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
LD = np.longdouble
_scenes = {}


def scene(nb, n, m=0):
    """(posm, vel, tpos, tvel) in fp64, read-only: test_hermite6_gpu.py's Plummer sphere — masses that all differ, coordinates that are
    no fp32 numbers — and m random moving points inside it."""
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


def f64(nb, n, **kw):
    return nb.NBodyEngine(n, precision="f64", **kw)


def raises(nb, code, call):
    with pytest.raises(nb.NBodyError) as er:
        call()
    assert er.value.code == code, (er.value.code, str(er.value))
    return str(er.value)


def passes(nb, e):
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]


def eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int((a != b).any(axis=-1).sum())} of {a.shape[0]} rows differ"


def probe_slab_points(n_total, width):
    """kernels_probe.hip's: the points whose partial rows (width float4 per point and chunk) fit 256 MiB, a multiple of 1024."""
    return max(1024, (256 << 20) // (probe_geometry(n_total)[0] * 16 * width) // 1024 * 1024)


CASES = [(1000, 25), (257, 300)]
EPS = [0.0, 0.05]


# ---- 1: a body asked about as a point gets its own row ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("eps", EPS)
def test_jerk_at_f64_at_the_bodies_own_state_is_get_jerk_f64(nb, n, eps):
    posm, vel, _, _ = scene(nb, n)
    rng = np.random.default_rng(n)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        acc, jerk = e.jerk(np.float64)
        # all of them; 300 in a shuffled order (N = 1025: a subset; N = 257: every body, 43 of them twice); the last body alone; counts
        # round the 256 lanes of a workgroup and its two points per lane — beyond n the bodies are asked about again: a point's sums
        # do not depend on the other points
        subset = rng.permutation(np.arange(max(n, 300)) % n)[:300]
        assert subset.size == 300
        forms = [np.arange(n), subset, np.array([n - 1])] + [np.arange(m) % n for m in (255, 256, 257, 512, 513)]
        for idx in forms:
            a, j = e.jerk_at_f64(posm[idx, :3], vel[idx, :3])
            eq(a, acc[idx], f"acc of {idx.size} points"); eq(j, jerk[idx], f"jerk of {idx.size} points")
        p, v, a0 = e.state(np.float64)                             # nothing a getter shows has changed
        eq(p, posm, "positions"); eq(v, vel, "velocities")


# ---- 2: random moving points -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("eps", EPS)
def test_jerk_at_f64_at_moving_points_against_the_augmented_context(nb, n, m, eps):
    posm, vel, tpos, tvel = scene(nb, n, m)
    ap, av = augmented(posm, vel, tpos, tvel)
    with f64(nb, n, eps=eps, time_kernels=True) as e, f64(nb, n + m, eps=eps) as aug:
        e.set_state(posm, vel); aug.set_state(ap, av)
        f0 = passes(nb, e)[0]
        a, j = e.jerk_at_f64(tpos, tvel)
        assert passes(nb, e)[0] - f0 == 1                          # one pass under NBODY_KERNEL_FORCES
        ra, rj = aug.jerk(np.float64)
        eq(a, ra[n:], "acc against the augmented rows"); eq(j, rj[n:], "jerk against the augmented rows")
        la, lj = direct_jerk(posm[:, :3], posm[:, 3], vel, tpos, tvel, eps=eps, dtype=LD)
        ea, ej = rel(a, la.astype(np.float64)).max(), rel(j, lj.astype(np.float64)).max()
        print(f"N = {n}, M = {m}, eps = {eps}: acc {ea:.3e}, jerk {ej:.3e} of the long-double sum")
        assert ea < TOL_F64 and ej < TOL_F64
        # at rest: NULL velocities give the bits an array of zeros gives; either output alone
        a0, j0 = e.jerk_at_f64(tpos)
        az, jz = e.jerk_at_f64(tpos, np.zeros_like(tpos))
        eq(a0, az, "acc at rest"); eq(j0, jz, "jerk at rest"); eq(a0, a, "acc does not depend on the velocity")
        only = np.empty((m, 3))
        assert e._L.nbody_jerk_at_f64(e._h, tpos.ctypes.data, 24, tvel.ctypes.data, 24, m, None, 24, only.ctypes.data, 24) == 0
        eq(only, j, "jerk alone")
        wide = np.full((m, 5), -1.0)                               # a stride of its own
        assert e._L.nbody_jerk_at_f64(e._h, tpos.ctypes.data, 24, tvel.ctypes.data, 24, m, wide.ctypes.data, 40, None, 0) == 0
        eq(wide[:, :3], a, "acc into strided rows"); assert (wide[:, 3:] == -1.0).all()


@pytest.mark.parametrize("eps", EPS)
def test_a_point_exactly_on_a_body(nb, eps):
    n, k = 1000, 417
    posm, vel, _, tvel = scene(nb, n, 25)
    pt, pv = posm[k:k + 1, :3].copy(), tvel[:1].copy()
    rest = np.delete(np.arange(n), k)
    la, lj = direct_jerk(posm[rest, :3], posm[rest, 3], vel[rest], pt, pv, eps=eps, dtype=LD)   # the sum without that body
    massless = posm.copy(); massless[k, 3] = 0.0
    with f64(nb, n, eps=eps) as e, f64(nb, n, eps=eps) as without:
        e.set_state(posm, vel); without.set_state(massless, vel)
        a, j = e.jerk_at_f64(pt, pv)
        wa, wj = without.jerk_at_f64(pt, pv)
        eq(a, wa, "acc: the pair adds nothing")
        assert rel(a, la.astype(np.float64)).max() < TOL_F64
        if eps == 0.0:                                             # the pair is dropped from every sum
            eq(j, wj, "jerk: the pair is dropped")
            assert rel(j, lj.astype(np.float64)).max() < TOL_F64
        else:                                                      # the jerk carries G m w / eps^3, a does not
            w = (vel[k:k + 1, :3] - pv).astype(LD)
            want = lj + LD(G) * LD(posm[k, 3]) * w / (LD(eps) * LD(eps) * LD(eps))
            assert rel(j, want.astype(np.float64)).max() < TOL_F64
            assert np.abs(j - wj).max() > 1e3 * np.abs(wj).max()   # (and it dominates: this is no rounding matter)


def test_one_body_and_no_points(nb):
    posm = np.array([[1.5, -2.25, 3.0, 7.0]]); vel = np.array([[0.1, 0.7, -0.3, 0.0]])
    pts = np.array([[4.0, 1.0, -2.0], [1.5, -2.25, 3.0]]); pv = np.array([[0.3, 0.0, 0.1], [0.0, 0.0, 0.0]])
    with f64(nb, 1) as e:
        e.set_state(posm, vel)
        a, j = e.jerk_at_f64(pts, pv)
        la, lj = direct_jerk(posm[:, :3], posm[:, 3], vel, pts, pv, dtype=LD)
        assert rel(a, la.astype(np.float64)).max() < TOL_F64 and rel(j, lj.astype(np.float64)).max() < TOL_F64
        assert not a[1].any() and not j[1].any()                   # on the only body, eps == 0: nothing
        a, j = e.jerk_at_f64(np.zeros((0, 3)))
        assert a.shape == (0, 3) and j.shape == (0, 3)


# ---- 3: slabs of the staging area ------------------------------------------------------------------------------------------------------

def test_points_beyond_one_slab_of_the_staging_area(nb):
    """N = 33000: a 512-body chunk, 65 chunks, so a slab of the fp64 jerk's rows (three float4 per point and chunk) is 86016 points.
    M = 86016 + 450 = 86466 is the smallest count at which the 300 points round the slab boundary and the last 300 do not overlap."""
    n = 33000
    assert probe_geometry(n) == (65, 512)
    slab = probe_slab_points(n, 3)
    m = slab + 450
    assert slab == 86016 and m == 86466
    posm, vel, tpos, tvel = scene(nb, n, m)
    with f64(nb, n, eps=0.05) as e:
        e.set_state(posm, vel)
        a, j = e.jerk_at_f64(tpos, tvel)
        for lo in (0, slab - 150, m - 300):
            sa, sj = e.jerk_at_f64(tpos[lo:lo + 300], tvel[lo:lo + 300])
            eq(a[lo:lo + 300], sa, f"acc of points {lo} .. {lo + 300}"); eq(j[lo:lo + 300], sj, f"jerk of points {lo} .. {lo + 300}")


@pytest.mark.parametrize("order", [4, 6])
def test_tracers_beyond_one_slab_step_as_they_do_alone(nb, order):
    """The same for the tracers' passes: a tracer's step depends on the tracer and the bodies alone, so a tracer among more tracers than
    one slab holds (86016 for the jerk's rows, 51200 for the snap's nine doubles) ends where it ends as one of 300."""
    n = 33000
    slab = probe_slab_points(n, 3 if order == 4 else 5)
    assert slab == (86016 if order == 4 else 51200)
    m = slab + 450
    posm, vel, tpos, tvel = scene(nb, n, 86466)
    tpos, tvel = tpos[:m], tvel[:m]
    step = (lambda x: x.hermite_step(DT, 2)) if order == 4 else (lambda x: x.hermite6_step(DT, 2))
    cache = (lambda x: x.hermite_tracers_state()) if order == 4 else (lambda x: x.hermite6_tracers_state())
    with f64(nb, n, eps=0.05) as e:
        e.set_state(posm, vel)
        e.set_tracers_f64(tpos, tvel)
        step(e)
        p, v = e.tracers_f64()
        c = cache(e)
        bodies = e.state(np.float64)
        for lo in (0, slab - 150, m - 300):
            e.set_state(posm, vel)
            e.set_tracers_f64(tpos[lo:lo + 300], tvel[lo:lo + 300])
            step(e)
            sp, sv = e.tracers_f64()
            eq(p[lo:lo + 300], sp, f"positions of tracers {lo} .. {lo + 300}"); eq(v[lo:lo + 300], sv, f"velocities of tracers {lo} .. {lo + 300}")
            for name, x, y in zip("abcdef", c, cache(e)):
                eq(x[lo:lo + 300], y, f"cache array {name} of tracers {lo} .. {lo + 300}")
            for x, y in zip(bodies, e.state(np.float64)):
                eq(x, y, "the bodies")


# ---- 4, 5: steps against the augmented context -----------------------------------------------------------------------------------------

def compare_with_augmented(e, aug, plain, n, order, what):
    cache = (lambda x: x.hermite_state()) if order == 4 else (lambda x: x.hermite6_state())
    tcache = e.hermite_tracers_state() if order == 4 else e.hermite6_tracers_state()
    tp, tv = e.tracers_f64()
    ap, av, aa = aug.state(np.float64)
    eq(tp, ap[n:, :3], f"{what}: tracer positions"); eq(tv, av[n:, :3], f"{what}: tracer velocities")
    for k, (x, y) in enumerate(zip(tcache, cache(aug))):
        eq(x, y[n:], f"{what}: tracer cache array {k}")
    for name, x, y, z in zip(("positions", "velocities", "accelerations"), e.state(np.float64), (ap, av, aa), plain.state(np.float64)):
        eq(x, y[:n], f"{what}: the bodies' {name} against the augmented context"); eq(x, z, f"{what}: the bodies' {name} against a tracer-free context")
    for k, (x, y, z) in enumerate(zip(cache(e), cache(aug), cache(plain))):
        eq(x, y[:n], f"{what}: the bodies' cache array {k} against the augmented context"); eq(x, z, f"{what}: the bodies' cache array {k}")


@pytest.mark.parametrize("order", [4, 6])
@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("eps", EPS)
def test_three_steps_against_the_augmented_context(nb, order, n, m, eps):
    posm, vel, tpos, tvel = scene(nb, n, m)
    ap, av = augmented(posm, vel, tpos, tvel)
    with f64(nb, n, eps=eps) as e, f64(nb, n + m, eps=eps) as aug, f64(nb, n, eps=eps) as plain:
        e.set_state(posm, vel); aug.set_state(ap, av); plain.set_state(posm, vel)
        e.set_tracers_f64(tpos, tvel)
        assert e.tracer_count_f64 == m and plain.tracer_count_f64 == 0
        if order == 6:                                             # the start's (a0, j0, s0); a3, a4, a5 read as zeros
            assert e.hermite6_tracers_timescale()[2] == 0
            for x in (e, aug, plain):
                assert x.hermite6_timescale()[2] == 0
            compare_with_augmented(e, aug, plain, n, order, "the start")
            assert not any(x.any() for x in e.hermite6_tracers_state()[3:])
        for s in range(3):
            for x in (e, aug, plain):
                x.hermite_step(DT, 1) if order == 4 else x.hermite6_step(DT, 1)
            compare_with_augmented(e, aug, plain, n, order, f"step {s + 1}")
        assert (e.hermite_timescale() if order == 4 else e.hermite6_timescale()) == (plain.hermite_timescale() if order == 4 else plain.hermite6_timescale())


# ---- 6: the adaptive drivers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [4, 6])
def test_advance_carries_the_tracers_and_ignores_them(nb, order):
    n, m = 257, 300
    posm, vel, tpos, tvel = scene(nb, n, m)
    eta, eta_start = (0.02, 0.01) if order == 4 else (0.5, 0.01)
    adv = (lambda x, **kw: x.hermite_advance(**kw)) if order == 4 else (lambda x, **kw: x.hermite6_advance(**kw))
    scale = (lambda x: x.hermite_timescale()) if order == 4 else (lambda x: x.hermite6_timescale())
    tscale = (lambda x: x.hermite_tracers_timescale()) if order == 4 else (lambda x: x.hermite6_tracers_timescale())
    tstate = (lambda x: x.hermite_tracers_state()) if order == 4 else (lambda x: x.hermite6_tracers_state())
    ref = H.timescale if order == 4 else H6.timescale
    n_zero = 2 if order == 4 else 3                                # the arrays a kind-0 time scale is formed from
    with f64(nb, n, eps=0.05) as e, f64(nb, n, eps=0.05) as plain, f64(nb, n, eps=0.05) as replay:
        plain.set_state(posm, vel)
        t10, steps = adv(plain, t_span=1e9, eta=eta, eta_start=eta_start, max_steps=10)
        assert steps == 10
        span, dt_max = 0.97 * t10, 0.2 * t10                      # about ten steps, the last one cut, the cap reached
        plain.set_state(posm, vel)
        for x in (e, replay):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
        # the tracers' own time scale before a step: kind 0, from the (a0, j0) the call evaluates
        got = tscale(e)
        assert got == ref(*tstate(e)[:n_zero]) and got[2] == 0
        kw = dict(t_span=span, eta=eta, eta_start=eta_start, dt_max=dt_max)
        done = adv(e, **kw)
        assert done == adv(plain, **kw) and done[0] == span and 5 <= done[1] <= 40
        for name, x, y in zip(("positions", "velocities", "accelerations"), e.state(np.float64), plain.state(np.float64)):
            eq(x, y, f"the bodies' {name} with and without tracers")
        assert scale(e) == scale(plain)
        # the header's dt rule, step by step
        t_acc, taken = 0.0, 0
        root_eta = float(np.sqrt(np.float64(eta)))
        while t_acc < span:
            t, _, kind = scale(replay)
            dt = min(dt_max, (root_eta * t if order == 4 else eta * t) if kind == 1 else eta_start * t)
            last = dt >= span - t_acc
            if last:
                dt = span - t_acc
            replay.hermite_step(dt, 1) if order == 4 else replay.hermite6_step(dt, 1)
            t_acc = span if last else t_acc + dt
            taken += 1
        assert taken == done[1]
        for name, x, y in zip(("positions", "velocities"), e.tracers_f64(), replay.tracers_f64()):
            eq(x, y, f"the tracers' {name} against the replay")
        for k, (x, y) in enumerate(zip(tstate(e), tstate(replay))):
            eq(x, y, f"the tracers' cache array {k} against the replay")
        got = tscale(e)                                            # after steps: kind 1, from the derivatives
        assert got == ref(*tstate(e)) and got[2] == 1 and 0 <= got[1] < m


# ---- 7: invalidation and accounting ----------------------------------------------------------------------------------------------------

HOW = ["set_state", "step", "device_ptr", "hermite_restart", "set_tracers_f64"]


@pytest.mark.parametrize("order", [4, 6])
@pytest.mark.parametrize("how", HOW)
def test_a_step_behind_an_invalidation_evaluates_the_tracers_anew(nb, how, order):
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    step = (lambda x, k: x.hermite_step(DT, k)) if order == 4 else (lambda x, k: x.hermite6_step(DT, k))
    tstate = (lambda x: x.hermite_tracers_state()) if order == 4 else (lambda x: x.hermite6_tracers_state())
    start = 1 if order == 4 else 2                                 # the passes of a start: the bodies', and as many for the tracers
    with f64(nb, n, time_kernels=True) as e, f64(nb, n, time_kernels=True) as plain, f64(nb, n) as fresh:
        for x in (e, plain):
            x.set_state(posm, vel)
        e.set_tracers_f64(tpos, tvel)
        f0, u0 = passes(nb, e); g0, v0 = passes(nb, plain)
        for x in (e, plain):
            step(x, 2)
        f1, u1 = passes(nb, e); g1, v1 = passes(nb, plain)
        assert (g1 - g0, v1 - v0) == (start + 2, 2)                # without tracers every count is what it was
        assert (f1 - f0, u1 - u0) == (2 * (start + 2), 2)          # a tracer evaluation beside every evaluation of the bodies; one update pass a step
        tp, tv = e.tracers_f64()
        for x in ((e, plain) if how != "set_tracers_f64" else (e,)):
            if how == "set_state":
                p, v, _ = x.state(np.float64)
                x.set_state(p, v)
            elif how == "step":
                x.step(DT, 1)
            elif how == "device_ptr":
                assert x.device_ptr(nb._lib.BUF_POSM)[0]
            elif how == "hermite_restart":
                x.hermite_restart()
            elif how == "set_tracers_f64":
                x.set_tracers_f64(tp, tv)
        assert e.tracer_count_f64 == m                             # uploads (and everything else here) keep the tracers ...
        for name, a, b in zip(("positions", "velocities"), e.tracers_f64(), (tp, tv)):
            eq(a, b, f"{how}: the tracers' {name}")                # ... and nothing but the Hermite steps moves them
        assert "tracers_get" in raises(nb, nb._lib.ERR_STATE, lambda: tstate(e))
        if how == "set_tracers_f64":                               # ... which forgets the tracers' caches and only those
            assert len(e.hermite_state() if order == 4 else e.hermite6_state()) == (4 if order == 4 else 6)
        p, v, _ = e.state(np.float64)
        f1 = passes(nb, e)[0]; g1 = passes(nb, plain)[0]
        step(e, 1); step(plain, 1)
        f2 = passes(nb, e)[0]; g2 = passes(nb, plain)[0]
        if how == "set_tracers_f64":
            assert (f2 - f1, g2 - g1) == (start + 2, 1)            # the tracers' start, the step's two passes; the bodies go on from their cache
        else:
            assert (f2 - f1, g2 - g1) == (2 * (start + 1), start + 1)
            fresh.set_state(p, v); fresh.set_tracers_f64(tp, tv)   # ... from the stored bodies and tracers alone
            step(fresh, 1)
            for name, a, b in zip(("positions", "velocities"), e.tracers_f64(), fresh.tracers_f64()):
                eq(a, b, f"{how}: the tracers' {name} against a fresh context")
            for k, (a, b) in enumerate(zip(tstate(e), tstate(fresh))):
                eq(a, b, f"{how}: the tracers' cache array {k} against a fresh context")
        for a, b in zip(e.state(np.float64), plain.state(np.float64)):
            eq(a, b, f"{how}: the bodies with and without tracers")
        # once a pointer is out every CALL evaluates anew — not every step of a call
        step(e, 2)
        assert passes(nb, e)[0] - f2 == (2 * (start + 2) if how == "device_ptr" else 4), how


def test_what_moves_the_tracers_and_what_does_not(nb, tmp_path):
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    with f64(nb, n) as e, f64(nb, n) as other, f64(nb, n) as plain:
        e.set_state(posm, vel); plain.set_state(posm, vel); other.set_state(posm, vel)
        e.set_tracers_f64(tpos, tvel); other.set_tracers_f64(tpos, tvel)
        p, v = e.tracers_f64()
        eq(p, tpos, "positions as set"); eq(v, tvel, "velocities as set")
        other.step(DT, 2); other.compute_forces(); other.tick(DT)  # the kick-drift calls leave every byte of the tracers
        p, v = other.tracers_f64()
        eq(p, tpos, "positions behind nbody_step"); eq(v, tvel, "velocities behind nbody_step")
        e.hermite_step(DT, 2); e.hermite6_step(DT, 2)              # both orders move them
        p, v = e.tracers_f64()
        assert (p != tpos).all() and (v != tvel).any()
        # a get / set round trip restores them bit for bit: a second context goes on as this one does
        other.set_state(*e.state(np.float64)[:2]); other.set_tracers_f64(p, v)
        q, w = other.tracers_f64()
        eq(q, p, "positions after the round trip"); eq(w, v, "velocities after the round trip")
        e.hermite_restart()
        e.hermite6_step(DT, 1); other.hermite6_step(DT, 1)
        for a, b in zip(e.tracers_f64() + e.hermite6_tracers_state(), other.tracers_f64() + other.hermite6_tracers_state()):
            eq(a, b, "a step behind the round trip")
        # at rest; replaced; removed
        other.set_tracers_f64(p[:7])
        assert other.tracer_count_f64 == 7 and not other.tracers_f64()[1].any()
        other.set_tracers_f64(np.zeros((0, 3)))
        assert other.tracer_count_f64 == 0 and other.tracers_f64()[0].shape == (0, 3) and other.hermite_tracers_state()[0].shape == (0, 3)
        raises(nb, nb._lib.ERR_STATE, other.hermite_tracers_timescale)   # no tracers
        raises(nb, nb._lib.ERR_STATE, other.hermite6_tracers_timescale)
        # checkpoints do not store them: the files are the same bytes with and without
        plain.hermite_step(DT, 2); plain.hermite6_step(DT, 2); plain.hermite_restart(); plain.hermite6_step(DT, 1)
        a, b = str(tmp_path / "with.ckpt"), str(tmp_path / "without.ckpt")
        e.save_checkpoint(a); plain.save_checkpoint(b)
        data = open(a, "rb").read()
        assert data[:8] == b"NBDYCKP2" and data == open(b, "rb").read()
        assert other.load_checkpoint(a) == e.steps_done() and e.load_checkpoint(a) == e.steps_done()
        assert e.tracer_count_f64 == m and other.tracer_count_f64 == 0   # a load keeps the tracers a context has, and brings none


# ---- 8: errors -------------------------------------------------------------------------------------------------------------------------

def eight_calls(e):
    pts = np.zeros((3, 3)) + [[1.0], [2.0], [3.0]]
    return ((lambda: e.jerk_at_f64(pts)), (lambda: e.set_tracers_f64(pts)), e.tracers_f64, (lambda: e.tracer_count_f64), e.hermite_tracers_state,
            e.hermite6_tracers_state, e.hermite_tracers_timescale, e.hermite6_tracers_timescale)


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
    pts32 = np.ones((3, 3), np.float32)
    for kw, why in (({}, "fp32"), ({"precision": "f32_kahan"}, "fp32"), ({"precision": "f64", "i_begin": 0, "i_count": 1000}, "slice"),
                    ({"devices": [0]}, "multi-device")):
        with nb.NBodyEngine(big, **kw) as e:
            if kw.get("precision") == "f64":
                e.set_state(p32.astype(np.float64), v32.astype(np.float64))
            else:
                e.set_state(p32, v32)
            for call in eight_calls(e):
                assert why in raises(nb, E.ERR_UNSUPPORTED, call), kw
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    with f64(nb, n) as e:
        for call in eight_calls(e):                                # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(posm, vel)
        # what the fp32 calls report on an fp64 context is what it was
        assert "fp64" in raises(nb, E.ERR_UNSUPPORTED, lambda: e.jerk_at(pts32))
        raises(nb, E.ERR_UNSUPPORTED, lambda: e.set_tracers(pts32))
        out = np.empty((m, 18))
        P, V, O, L = tpos.ctypes.data, tvel.ctypes.data, out.ctypes.data, e._L
        assert L.nbody_jerk_at_f64(e._h, None, 24, None, 24, m, O, 24, O, 24) == E.ERR_INVALID       # null points
        assert L.nbody_jerk_at_f64(e._h, P, 24, V, 24, -1, O, 24, O, 24) == E.ERR_INVALID            # n < 0
        assert L.nbody_jerk_at_f64(e._h, P, 24, V, 24, m, None, 24, None, 24) == E.ERR_INVALID       # both outputs null
        for strides in ((23, 24, 24, 24), (24, 23, 24, 24), (24, 24, 23, 24), (24, 24, 24, 23)):
            assert L.nbody_jerk_at_f64(e._h, P, strides[0], V, strides[1], m, O, strides[2], O, strides[3]) == E.ERR_INVALID
        assert L.nbody_jerk_at_f64(e._h, P, 24, None, 0, m, O, 24, None, 0) == 0                      # (strides of absent arrays are not looked at)
        assert L.nbody_jerk_at_f64(e._h, None, 0, None, 0, 0, None, 0, None, 0) == E.ERR_INVALID     # null points even with n == 0
        assert L.nbody_jerk_at_f64(e._h, P, 24, None, 0, 0, O, 24, None, 0) == 0                      # n == 0: a no-op
        assert L.nbody_set_tracers_f64(e._h, None, 24, None, 24, 3) == E.ERR_INVALID
        assert L.nbody_set_tracers_f64(e._h, P, 24, V, 24, -1) == E.ERR_INVALID
        assert L.nbody_set_tracers_f64(e._h, P, 23, V, 24, m) == E.ERR_INVALID and L.nbody_set_tracers_f64(e._h, P, 24, V, 23, m) == E.ERR_INVALID
        assert L.nbody_tracer_count_f64(e._h, None) == E.ERR_INVALID
        e.set_tracers_f64(tpos, tvel)
        assert L.nbody_get_tracers_f64(e._h, O, 23, None, 0) == E.ERR_INVALID and L.nbody_get_tracers_f64(e._h, None, 0, O, 23) == E.ERR_INVALID
        assert L.nbody_hermite_tracers_get(e._h, None, 96) == E.ERR_INVALID and L.nbody_hermite_tracers_get(e._h, O, 95) == E.ERR_INVALID
        assert L.nbody_hermite6_tracers_get(e._h, None, 144) == E.ERR_INVALID and L.nbody_hermite6_tracers_get(e._h, O, 143) == E.ERR_INVALID
        assert L.nbody_hermite_tracers_timescale(e._h, None, None, None) == E.ERR_INVALID
        assert L.nbody_hermite6_tracers_timescale(e._h, None, None, None) == E.ERR_INVALID
        raises(nb, E.ERR_STATE, e.hermite_tracers_state)           # nothing cached yet
        raises(nb, E.ERR_STATE, e.hermite6_tracers_state)
        e.step_begin()                                             # a step is open
        raises(nb, E.ERR_STATE, lambda: e.jerk_at_f64(tpos))
        e.step_end(0.0)
        # block sessions carry no tracers, and say how to get rid of them
        for begin in ((lambda: e.hermite_block_begin(DT, 2)), (lambda: e.hermite6_block_begin(DT, 2))):
            assert "nbody_set_tracers_f64(ctx, NULL, 0, NULL, 0, 0)" in raises(nb, E.ERR_UNSUPPORTED, begin)
        e.set_tracers_f64(np.zeros((0, 3)))
        for begin in ((lambda: e.hermite_block_begin(DT, 2)), (lambda: e.hermite6_block_begin(DT, 2))):
            begin()
            assert "block session" in raises(nb, E.ERR_STATE, lambda: e.set_tracers_f64(tpos, tvel))
            e.set_tracers_f64(np.zeros((0, 3)))                    # removing none is fine
            e.hermite_restart()
        e.set_tracers_f64(tpos, tvel)                              # the session is gone
        assert e.tracer_count_f64 == m
