"""The yardsticks of the jerk tests checked on the CPU: tests/jerk_ref.py's direct sum against a central difference of the direct
acceleration and against the two-body circular orbit, and its two emulations of the kernels' arithmetic against the direct sums on the
scenes tests/test_jerk_gpu.py uses (the figures quoted there next to every case are printed here)."""
import os

import numpy as np
import pytest

from jerk_ref import G, direct_jerk, emulate_jerk_f32, emulate_jerk_f64, jerk_time_of, k_of, probe_velocities, rel
from probe_scenes import GOLDEN, TOL_ACC, bodies, probes_for


def test_direct_jerk_is_the_central_difference_of_the_direct_acceleration(nb):
    """All bodies of the shipped scene moved along x + v h: (a(+h) - a(-h)) / 2h = j + (h^2 / 6) d^3a/dt^3 + O(h^4).

    The truncation term: for a body whose field one neighbour at distance r and relative speed w dominates, every time derivative of
    a ~ r^-2 brings a factor of about (k + 1) w / r, so |a'''| ~ 24 |a| / tau^3 and |j| ~ 2 |a| / tau with tau = r / w, and the
    relative truncation error is about 2 (h / tau)^2 = (h / t)^2 / 2 with t = |a| / |j| = tau / 2.  The scene's smallest t is 6.7e-3
    (body 986), so h = 1e-6 gives 1.1e-8 there and less everywhere else; the bound is 1e-7, eight times that estimate and more.  The rounding
    term eps |a| / (h |j|) is kept out of the way by forming the difference in long double (1e-19 * t / h <= 1e-11 for t <= 100)."""
    posm, vel = bodies(nb, 2000)
    ld = np.longdouble
    pos, mass, v = posm[:, :3].astype(ld), posm[:, 3], vel[:, :3].astype(ld)
    h = ld(1e-6)
    acc, jerk = direct_jerk(pos, mass, v, pos, v, skip_self=True)
    t, body = jerk_time_of(acc, jerk)
    assert body == 986 and t == pytest.approx(6.70305e-3, rel=1e-5)
    assert 8 * 0.5 * (float(h) / t) ** 2 < 1e-7
    ap, _ = direct_jerk(pos + v * h, mass, v, pos + v * h, v, skip_self=True, dtype=ld)
    am, _ = direct_jerk(pos - v * h, mass, v, pos - v * h, v, skip_self=True, dtype=ld)
    fd = ((ap - am) / (2 * h)).astype(np.float64)
    er = rel(fd, jerk)
    print(f"direct_jerk against the central difference, N=2000, h=1e-6: max rel err {er.max():.3e} at body {int(er.argmax())}")
    assert er.max() < 1e-7


def test_two_bodies_on_a_circular_orbit():
    """Separation r, masses m1, m2, omega^2 = G (m1 + m2) / r^3: d . w = 0, and body 1's jerk is -omega^2 v_rel m2 / (m1 + m2) with
    v_rel = v_1 - v_2 (body 2's the same with the roles swapped)."""
    m1, m2, r = 3.0, 5.0, 7.0
    om = np.sqrt(G * (m1 + m2) / r ** 3)
    x1, x2 = -r * m2 / (m1 + m2), r * m1 / (m1 + m2)
    pos = np.array([[x1, 0, 0], [x2, 0, 0]], np.float64)
    vel = np.array([[0, om * x1, 0], [0, om * x2, 0]], np.float64)
    acc, jerk = direct_jerk(pos, [m1, m2], vel, pos, vel, skip_self=True)
    vrel = vel[0] - vel[1]
    want = np.array([-om ** 2 * vrel * m2 / (m1 + m2), om ** 2 * vrel * m1 / (m1 + m2)])
    assert rel(jerk, want).max() < 1e-14
    assert rel(acc, -om ** 2 * pos).max() < 1e-14
    # |a| / |j| = 1 / omega for both; the tie goes to body 0
    assert k_of(acc, jerk) == pytest.approx(om ** 2, rel=1e-14)


def test_the_fp32_emulation_on_the_gpu_cases(nb):
    """What probe_jerk_pk_kernel's arithmetic alone gives on the scenes of tests/test_jerk_gpu.py: each at most TOL_ACC / 4."""
    worst = 0.0
    for n, eps in ((2000, 0.0), (2000, 0.05), (257, 0.0)):
        posm, vel = bodies(nb, n)
        pos, mass = posm[:, :3], posm[:, 3]
        ra, rj = direct_jerk(pos, mass, vel, pos, vel, eps=eps, skip_self=True)
        ea, ej = emulate_jerk_f32(pos, mass, vel, pos, vel, eps=eps, skip_self=True)
        print(f"emulated per body N={n} eps={eps}: acc {rel(ea, ra).max():.2e} jerk {rel(ej, rj).max():.2e}")
        worst = max(worst, rel(ea, ra).max(), rel(ej, rj).max())
    for n, m, eps in ((2000, 1, 0.0), (2000, 64, 0.0), (2000, 65, 0.0), (2000, 777, 0.0), (2000, 777, 0.05), (20000, 100, 0.0)):
        posm, vel = bodies(nb, n)
        pos, mass = posm[:, :3], posm[:, 3]
        pts, pv = probes_for(pos, m), probe_velocities(m)
        ra, rj = direct_jerk(pos, mass, vel, pts, pv, eps=eps)
        ea, ej = emulate_jerk_f32(pos, mass, vel, pts, pv, eps=eps)
        print(f"emulated at points N={n} M={m} eps={eps}: acc {rel(ea, ra).max():.2e} jerk {rel(ej, rj).max():.2e}")
        worst = max(worst, rel(ea, ra).max(), rel(ej, rj).max())
    assert worst <= TOL_ACC / 4


def test_the_fp64_sums_against_long_double():
    """The fp64 bound of tests/test_jerk_gpu.py is 1e-12 against the long-double sum: sums in the kernel's order sit far below it."""
    g = np.load(os.path.join(GOLDEN, "plummer_n1024_seed1.npz"))
    posm, vel = g["posm"].astype(np.float64), g["vel"].astype(np.float64)
    ra, rj = direct_jerk(posm[:, :3], posm[:, 3], vel, posm[:, :3], vel, skip_self=True, dtype=np.longdouble)
    ea, ej = emulate_jerk_f64(posm[:, :3], posm[:, 3], vel)
    print(f"fp64 sums in kernel order, plummer N=1024: acc {rel(ea, ra).max():.2e} jerk {rel(ej, rj).max():.2e}")
    assert max(rel(ea, ra).max(), rel(ej, rj).max()) < 1e-13
