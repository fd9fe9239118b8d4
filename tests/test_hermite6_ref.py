"""tests/hermite6_ref.py, the numpy yardstick of the snap pass and of sixth-order Hermite stepping, pinned on the CPU: its snap is the time
derivative of jerk_ref.direct_jerk, its chunk-ordered fp64 sums sit far inside the project's fp64 parity bound, the scheme as restated
there is of order six, its adaptive driver does what nbody_hermite6_advance documents — and the public surface exists.

Measured here (numpy, fp64): circular orbit of hermite_ref.kepler(0.0), one period in 16, 32, 64, 128, 256 steps: closing errors 7.78e-4,
1.18e-5, 1.81e-7, 2.79e-9, 4.33e-11 of the separation, ratios 65.99, 65.15, 64.85, 64.48 (fourth order at 256 steps: 2.86e-7).  e = 0.9
with dt_max = P / 16: eta = 0.5 closes to 2.76e-4 a in 70 steps, eta = 0.3 to 1.59e-5 a in 116; hermite_ref.Hermite.advance(eta = 0.01)
takes 242 steps for 3.51e-4 a."""
import ctypes
import os
import re

import numpy as np
import pytest

import hermite6_ref as H6
import hermite_ref as H
from jerk_ref import direct_jerk, jerk_time_of, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)


def closing_error(posm, start, a=100.0):
    return float(np.abs(posm[:, :3] - start[:, :3]).max() / a)


def cloud(n, seed, mass=(1.0, 3.0)):
    rng = np.random.default_rng(seed)
    posm = np.concatenate([rng.normal(0.0, 100.0, (n, 3)), rng.uniform(mass[0], mass[1], (n, 1))], 1)
    vel = np.zeros((n, 4)); vel[:, :3] = rng.normal(0.0, 30.0, (n, 3))
    return posm, vel


def rel_ld(got, ref):
    return float((np.linalg.norm((got.astype(LD) - ref.astype(LD)), axis=1) / np.linalg.norm(ref.astype(LD), axis=1)).max())


# ---- the pair term ---------------------------------------------------------------------------------------------------------------------

QUOTIENT_H = 1e-6
# The central difference's own error at that step, measured in long double as 4/3 |D(h) - D(h/2)| (its h^2 term by Richardson):
# 4.63e-9 at eps = 0, 4.37e-9 at eps = 3 on the cloud below (64 bodies, masses 1000 .. 3000 — close pairs set the figure).  At h = 1e-5
# it is 4.63e-7, at 1e-4 4.63e-5: pure h^2, rounding (1e-19 / h) plays no part.  The bound is ten times the larger figure.
QUOTIENT_BOUND = 10 * 4.7e-9


def jerk_quotient(posm, vel, eps, h):
    """(j(t + h) - j(t - h)) / (2 h) in long double along the trajectory x(t) = x + t v + t^2/2 a + t^3/6 j, v(t) = v + t a + t^2/2 j."""
    p = posm.astype(LD); v = vel.astype(LD); h = LD(h)
    a, j = direct_jerk(p[:, :3], p[:, 3], v, p[:, :3], v, eps=eps, skip_self=True, dtype=LD)
    side = []
    for t in (h, -h):
        x = p.copy(); w = v.copy()
        x[:, :3] = p[:, :3] + t * v[:, :3] + t * t / 2 * a + t * t * t / 6 * j
        w[:, :3] = v[:, :3] + t * a + t * t / 2 * j
        side.append(direct_jerk(x[:, :3], x[:, 3], w, x[:, :3], w, eps=eps, skip_self=True, dtype=LD)[1])
    return (side[0] - side[1]) / (2 * h)


@pytest.mark.parametrize("eps", [0.0, 3.0])
def test_the_snap_is_the_time_derivative_of_the_jerk(eps):
    posm, vel = cloud(64, 7, mass=(1000.0, 3000.0))
    D, D2 = jerk_quotient(posm, vel, eps, QUOTIENT_H), jerk_quotient(posm, vel, eps, QUOTIENT_H / 2)
    own = 4.0 / 3.0 * rel_ld(D, D2)
    a, j, s = H6.direct_snap(posm, vel, None, eps=eps)
    a_ld, j_ld, s_ld = H6.direct_snap(posm, vel, None, eps=eps, dtype=LD)
    err, err_ld = rel_ld(s, D), rel_ld(s_ld, D)
    print(f"eps={eps}: h={QUOTIENT_H:g} quotient's own error {own:.3e}; snap against it: fp64 {err:.3e}, long double {err_ld:.3e}")
    assert own < QUOTIENT_BOUND / 5                                # the figure the bound was sized from still holds
    assert err < QUOTIENT_BOUND and err_ld < QUOTIENT_BOUND
    # a and j beside it are jerk_ref's own
    ra, rj = direct_jerk(posm[:, :3], posm[:, 3], vel, posm[:, :3], vel, eps=eps, skip_self=True)
    assert rel(a, ra).max() < 1e-14 and rel(j, rj).max() < 1e-14
    # an input acceleration array enters linearly through b alone: S(acc_in + c) == S(acc_in) for a constant shift, and a, j ignore it
    shifted = H6.direct_snap(posm, vel, a_ld + LD(5.0), eps=eps, dtype=LD)
    assert rel_ld(shifted[2], s_ld) < 1e-15 and rel_ld(shifted[0], a_ld) == 0.0 and rel_ld(shifted[1], j_ld) == 0.0


@pytest.mark.parametrize("n,eps", [(257, 0.0), (257, 0.05), (1025, 0.0), (1025, 0.05)])
def test_the_kernels_chunk_order_in_fp64_against_long_double(n, eps):
    posm, vel = cloud(n, n)
    ain = np.random.default_rng(n + 1).normal(0.0, 50.0, (n, 3))
    ref = H6.direct_snap(posm, vel, ain, eps=eps, dtype=LD)
    got = H6.emulate_snap_f64(posm, vel, ain, eps=eps)
    errs = [float(rel(g, r.astype(np.float64)).max()) for g, r in zip(got, ref)]
    print(f"N={n} eps={eps}: chunk-ordered fp64 sums against long double: a {errs[0]:.2e} j {errs[1]:.2e} s {errs[2]:.2e}")
    assert max(errs) < TOL_F64 / 4, errs


def test_coincident_bodies_and_a_single_body():
    posm = np.array([[1.0, 2.0, 3.0, 5.0], [1.0, 2.0, 3.0, 7.0], [4.0, -1.0, 0.5, 11.0]])
    vel = np.array([[0.1, 0.2, 0.3, 0.0], [-0.3, 0.1, 0.0, 0.0], [0.0, 0.5, -0.2, 0.0]])
    ain = np.array([[1.0, -2.0, 0.5], [0.25, 0.0, -1.0], [3.0, 1.0, 1.0]])
    lone = [np.delete(posm, k, 0) for k in (1, 0)], [np.delete(vel, k, 0) for k in (1, 0)], [np.delete(ain, k, 0) for k in (1, 0)]
    for emu in (False, True):
        f = H6.emulate_snap_f64 if emu else H6.direct_snap
        got = f(posm, vel, ain, eps=0.0)
        for k in (0, 1):                                           # eps == 0: the pair is dropped from all nine sums
            want = f(lone[0][k], lone[1][k], lone[2][k], eps=0.0)
            for g, w in zip(got, want):
                assert g[k].tobytes() == w[0].tobytes()
        eps = 0.5
        got = f(posm, vel, ain, eps=eps)
        for k, other in ((0, 1), (1, 0)):                          # eps > 0: the twin adds q w to the jerk, q b to the snap, nothing to a
            want = f(lone[0][k], lone[1][k], lone[2][k], eps=eps)
            q = H6.G * posm[other, 3] / eps ** 3
            assert np.allclose(got[0][k], want[0][0], rtol=1e-14, atol=0)
            assert np.allclose(got[1][k] - want[1][0], q * (vel[other, :3] - vel[k, :3]), rtol=1e-12)
            assert np.allclose(got[2][k] - want[2][0], q * (ain[other] - ain[k]), rtol=1e-12)
        one = f(posm[:1], vel[:1], ain[:1], eps=0.0)
        assert not any(x.any() for x in one)


# ---- the scheme ------------------------------------------------------------------------------------------------------------------------

def test_fixed_steps_converge_with_order_six():
    posm, vel, period = H.kepler(0.0)
    err = {}
    for steps in (16, 32, 64, 128):                                # 256 steps and beyond approach rounding: left out on purpose
        h = H6.Hermite6(posm, vel)
        h.step(period / steps, steps)
        err[steps] = closing_error(h.posm, posm)
        assert h.evaluations == steps + 1
    ratios = [err[s] / err[2 * s] for s in (16, 32, 64)]
    print("errors", err, "ratios", ratios)
    assert all(60.0 <= r <= 68.0 for r in ratios), (err, ratios)   # theory: 64; the fourth-order test's relative margin
    four = H.Hermite(posm, vel)
    four.step(period / 256, 256)
    assert err[64] < closing_error(four.posm, posm)                # 64 sixth-order steps beat 256 fourth-order ones (1.8e-7 : 2.9e-7)


REF_STEPS = 70                                                     # kepler(0.9), eta = 0.5, eta_start = 0.01, dt_max = P / 16


def test_the_adaptive_driver():
    posm, vel, period = H.kepler(0.9)
    h = H6.Hermite6(posm, vel)
    t_done, steps, dts = h.advance(period, eta=0.5, eta_start=0.01, dt_max=period / 16)
    err = closing_error(h.posm, posm)
    four = H.Hermite(posm, vel)
    _, steps4, _ = four.advance(period, eta=0.01, eta_start=0.01, dt_max=period / 16)
    err4 = closing_error(four.posm, posm)
    print(f"sixth order: {steps} steps, {err:.3e}; fourth order: {steps4} steps, {err4:.3e}")
    assert t_done == period and steps == REF_STEPS == len(dts) and steps4 == 242
    assert 2 * steps < steps4 and err <= err4
    assert max(dts) == period / 16 and max(dts) > 50 * dts[1]      # the cap is reached at apocentre
    assert abs(sum(dts) - period) < 1e-12 * period
    h = H6.Hermite6(posm, vel)
    assert h.advance(period, max_steps=5)[1] == 5 and h.advance(0.0) == (0.0, 0, [])


def test_timescale_conventions():
    posm, vel = cloud(33, 3, mass=(1000.0, 3000.0))
    h = H6.Hermite6(posm, vel)
    t, body, kind = h.timescale()
    assert kind == 0 and (t, body) == jerk_time_of(h.a0, h.j0)
    h.step(1e-3)
    t, body, kind = h.timescale()
    k = H6.hermite6_k(h.a0, h.j0, h.s0, h.a3, h.a4, h.a5)
    assert kind == 1 and body == int(np.argmax(k)) and t == float(1.0 / np.cbrt(np.sqrt(k.max())))
    assert abs(t - k.max() ** (-1.0 / 6.0)) < 1e-14 * t
    z = np.zeros((2, 3)); o = np.ones((2, 3))
    assert H6.timescale(z, z, z, z, z, z) == (np.inf, 0, 1)        # 0 / 0 counts as 0: no time scale
    assert H6.timescale(z, z, z, o, o, o) == (0.0, 0, 1)           # x / 0 is +inf
    nan = o.copy(); nan[1, 0] = np.nan
    assert H6.timescale(o, o, o, nan, o, o) == (0.0, 1, 1)         # not finite counts as +inf


def test_a_single_body_drifts():
    posm = np.array([[1.5, -2.25, 3.0, 7.0]]); vel = np.array([[0.1, 0.7, -0.3, 0.0]])
    h = H6.Hermite6(posm, vel)
    h.step(0.37)
    assert h.posm[:, :3].tobytes() == (posm[:, :3] + np.float64(0.37) * vel[:, :3]).tobytes() and h.vel.tobytes() == vel.tobytes()
    assert h.timescale() == (np.inf, 0, 1)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------

SYMBOLS = ("nbody_get_snap_f64", "nbody_hermite6_step", "nbody_hermite6_timescale", "nbody_hermite6_advance", "nbody_hermite6_get")
METHODS = ("snap", "hermite6_step", "hermite6_timescale", "hermite6_advance", "hermite6_state")


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
    assert "no square root" in text                                # the header says how eta enters nbody_hermite6_advance


def test_command_line_usage_errors(capsys):
    """hermite6 is a choice of --integrator with hermite's demands and exclusions: every refusal below is the program's own, with its
    reason, none argparse's "invalid choice" (the success paths run on the device: tests/test_hermite6_gpu.py)."""
    from parallelnbody_amd.__main__ import main
    for argv, why in ((["--integrator", "hermite6"], "--integrator hermite6 needs --precision f64"),
                      (["--integrator", "hermite6", "--precision", "f32_kahan"], "--integrator hermite6 needs --precision f64"),
                      (["--integrator", "hermite6", "--precision", "f64", "--eta", "0"], "--eta belongs to"),
                      (["--integrator", "hermite6", "--precision", "f64", "--theta", "1.0"], "not with --theta"),
                      (["--integrator", "hermite6", "--precision", "f64", "--leapfrog-start"], "not with --theta"),
                      (["--integrator", "hermite6", "--precision", "f64", "--levels", "3"], "--levels belongs to")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and why in err and "invalid choice" not in err, (argv, err)
