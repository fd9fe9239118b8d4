"""The yardstick of the fp64 tracers pinned on the CPU (tests/tracers_f64_ref.py; tests/test_tracers_f64_gpu.py holds the device to
the same rules): a tracer carried beside the bodies converges with the order of the scheme that carries it, tracers change no byte of
the bodies, the point sums are the bodies' sums where a point is a body of mass 0, and the public surface exists.

The scene of the order tests is circular_tracer(): one body of mass 4000 at rest on the origin — it feels nothing and stays — and a
tracer on the circular orbit of radius 100 round it: the relative orbit of hermite_ref.kepler(0).  The ratio bounds are the ones
tests/test_hermite_ref.py (15 .. 17.5) and tests/test_hermite6_ref.py (60 .. 68) apply to the bodies' own orders."""
import ctypes
import os
import re

import numpy as np

import hermite6_ref as H6
import hermite_ref as H
import tracers_f64_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def closing_error(pos, start, a=100.0):
    return float(np.abs(pos[:, :3] - start[:, :3]).max() / a)


def cloud(n, seed, mass=(1.0, 3.0)):
    rng = np.random.default_rng(seed)
    posm = np.concatenate([rng.normal(0.0, 100.0, (n, 3)), rng.uniform(mass[0], mass[1], (n, 1))], 1)
    vel = np.zeros((n, 4)); vel[:, :3] = rng.normal(0.0, 30.0, (n, 3))
    return posm, vel


def test_a_tracer_orbit_closes_with_order_four():
    posm, vel, tpos, tvel, period = T.circular_tracer()
    err = {}
    for n in (64, 128, 256, 512):
        h = T.Hermite(posm, vel, tpos, tvel)
        h.step(period / n, n)
        err[n] = closing_error(h.tpos, tpos)
        assert h.point_evaluations == n + 1 == h.evaluations      # one point evaluation per step once the cache is filled
        assert h.posm.tobytes() == posm.tobytes() and h.vel.tobytes() == vel.tobytes()   # the lone body never moves
    ratios = [err[n] / err[2 * n] for n in (64, 128, 256)]
    print("errors", err, "ratios", ratios)
    assert all(15.0 <= r <= 17.5 for r in ratios), (err, ratios)


def test_a_tracer_orbit_closes_with_order_six():
    posm, vel, tpos, tvel, period = T.circular_tracer()
    err = {}
    for steps in (16, 32, 64, 128):
        h = T.Hermite6(posm, vel, tpos, tvel)
        h.step(period / steps, steps)
        err[steps] = closing_error(h.tpos, tpos)
        assert h.point_evaluations == steps + 2                    # a start is a point jerk pass and a point snap pass
    ratios = [err[s] / err[2 * s] for s in (16, 32, 64)]
    print("errors", err, "ratios", ratios)
    assert all(60.0 <= r <= 68.0 for r in ratios), (err, ratios)
    four = T.Hermite(posm, vel, tpos, tvel)
    four.step(period / 256, 256)
    assert err[64] < closing_error(four.tpos, tpos)


def test_the_bodies_are_bit_identical_with_and_without_tracers():
    posm, vel = cloud(40, 5, mass=(1000.0, 3000.0))
    tp, tv = cloud(9, 6)
    for Plain, Carrying, state in ((H.Hermite, T.Hermite, ("posm", "vel", "a0", "j0", "a2", "a3")),
                                   (H6.Hermite6, T.Hermite6, ("posm", "vel", "a0", "j0", "s0", "a3", "a4", "a5"))):
        plain, carrying = Plain(posm, vel, eps=0.05), Carrying(posm, vel, tp[:, :3], tv[:, :3], eps=0.05)
        plain.step(1e-3, 3); carrying.step(1e-3, 3)
        for name in state:
            assert getattr(plain, name).tobytes() == getattr(carrying, name).tobytes(), name
        assert plain.timescale() == carrying.timescale()
        a = plain.advance(2e-2, dt_max=4e-3); b = carrying.advance(2e-2, dt_max=4e-3)
        assert a == b and plain.posm.tobytes() == carrying.posm.tobytes() and plain.evaluations == carrying.evaluations
        assert not (carrying.tpos[:, :3] == tp[:, :3]).all() and not carrying.tpos[:, 3].any()
        t, at, kind = carrying.tracers_timescale()
        assert kind == 1 and 0 <= at < 9 and 0 < t < np.inf


def test_a_point_is_a_body_of_mass_zero():
    """The oracle of the GPU tests in the small: the tracers' sums equal the rows of the tracers appended as bodies of mass 0 (here to
    rounding: numpy sums in another order; on the device, where a zero adds exactly nothing to a chain, in every bit)."""
    posm, vel = cloud(30, 7, mass=(1000.0, 3000.0))
    tp, tv = cloud(6, 8)
    tp[:, 3] = 0.0
    both_p, both_v = np.concatenate([posm, tp]), np.concatenate([vel, tv])
    for eps in (0.0, 0.05):
        a, j = T.point_jerk(posm, vel, tp[:, :3], tv[:, :3], eps=eps)
        ra, rj = H.direct(both_p, both_v, eps)
        assert np.allclose(a, ra[30:], rtol=1e-13, atol=0) and np.allclose(j, rj[30:], rtol=1e-12, atol=0)
        ain = H.direct(both_p, both_v, eps)[0]
        a, j, s = T.point_snap(posm, vel, ain[:30], tp, tv, ain[30:], eps=eps)
        ra, rj, rs = H6.direct_snap(both_p, both_v, ain, eps=eps)
        assert np.allclose(a, ra[30:], rtol=1e-13, atol=0) and np.allclose(s, rs[30:], rtol=1e-11, atol=0)
    # a point exactly on a body: eps == 0 drops the pair; eps > 0 adds G m w / eps^3 to the jerk and nothing to a
    on = posm[3:4, :3].copy(); w = vel[3:4, :3] - tv[:1, :3]
    rest = np.delete(np.arange(30), 3)
    a, j = T.point_jerk(posm, vel, on, tv[:1, :3], eps=0.0)
    ra, rj = T.point_jerk(posm[rest], vel[rest], on, tv[:1, :3], eps=0.0)
    assert np.allclose(a, ra, rtol=1e-14) and np.allclose(j, rj, rtol=1e-14)
    a, j = T.point_jerk(posm, vel, on, tv[:1, :3], eps=0.05)
    ra, rj = T.point_jerk(posm[rest], vel[rest], on, tv[:1, :3], eps=0.05)
    assert np.allclose(a, ra, rtol=1e-14) and np.allclose(j - rj, T.G * posm[3, 3] * w / 0.05 ** 3, rtol=1e-9)


SYMBOLS = ("nbody_jerk_at_f64", "nbody_set_tracers_f64", "nbody_get_tracers_f64", "nbody_tracer_count_f64", "nbody_hermite_tracers_get",
           "nbody_hermite6_tracers_get", "nbody_hermite_tracers_timescale", "nbody_hermite6_tracers_timescale")
METHODS = ("jerk_at_f64", "set_tracers_f64", "tracers_f64", "hermite_tracers_state", "hermite6_tracers_state", "hermite_tracers_timescale",
           "hermite6_tracers_timescale")


def test_the_header_the_library_and_the_engine_have_the_new_calls(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = ctypes.CDLL(nb._lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert hasattr(L, s), f"{s} is not exported"
        assert getattr(nb.lib(), s).argtypes is not None
    for m in METHODS:
        assert callable(getattr(nb.NBodyEngine, m, None)), m
    assert isinstance(nb.NBodyEngine.tracer_count_f64, property)
    # the header says which calls advance the fp64 tracers and which leave them alone
    assert "ONLY nbody_hermite_step, nbody_hermite_advance, nbody_hermite6_step and nbody_hermite6_advance advance the fp64 tracers" in text
