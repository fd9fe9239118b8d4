"""The fp64 potential, tidal tensor and snap at points without a device: the six symbols are declared and bound, the yardstick of
tests/pot_tidal_f64_ref.py meets the closed forms, and the kernel's summation order stays far below the bound the GPU tests use."""
import os
import re

import numpy as np
import pytest

import pot_tidal_f64_ref as R
from jerk_ref import G, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
SYMBOLS = ("nbody_potential_at_f64", "nbody_get_potentials_f64", "nbody_tidal_at_f64", "nbody_get_tidal_f64", "nbody_tidal_time_f64",
           "nbody_snap_at_f64")


def test_the_six_symbols_are_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = nb.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert getattr(L, s).argtypes is not None, f"{s} has no prototype in parallelnbody_amd/_lib.py"
    assert len(L.nbody_snap_at_f64.argtypes) == 12 and len(L.nbody_tidal_at_f64.argtypes) == 6
    for name in ("potential_at_f64", "potentials_f64", "tidal_at_f64", "tidal_f64", "tidal_time_f64", "snap_at_f64"):
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__


@pytest.mark.parametrize("eps", [0.0, 0.75])
@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_the_yardstick_meets_the_closed_forms_of_one_body(eps, dtype):
    """One body of mass M on the origin: phi = -G M / s, T_ab = G M (3 x_a x_b / s^5 - delta_ab / s^3) with s^2 = r^2 + eps^2 (the
    Plummer forms; eps == 0: the Kepler ones), at generic points."""
    M = 37.5
    pts = np.array([[1.25, -2.5, 0.75], [-3.0, 0.5, 4.0], [0.3, 0.2, -0.1]])
    phi, t6 = R.direct(np.zeros((1, 3)), [M], pts, eps=eps, dtype=dtype)
    x = pts.astype(LD)
    s = np.sqrt((x * x).sum(1) + LD(eps) * LD(eps))
    want_phi = -LD(G) * LD(M) / s
    want = np.empty((3, 6), LD)
    for c, (a, b) in enumerate(R.PAIRS):
        want[:, c] = LD(G) * LD(M) * (3 * x[:, a] * x[:, b] / s ** 5 - (1 if a == b else 0) / s ** 3)
    assert R.rel_phi(phi, want_phi.astype(np.float64)) < 4e-16
    assert rel(t6, want.astype(np.float64)).max() < 1e-15
    if eps == 0.0:                                                 # traceless in vacuum
        assert np.abs((t6[:, 0] + t6[:, 1] + t6[:, 2]).astype(np.float64)).max() < 1e-14 * float(np.abs(t6).max())
    # the same through the kernel-order restatement
    kp, kt = R.kernel_order(np.zeros((1, 3)), [M], pts, eps=eps)
    assert R.rel_phi(kp, want_phi.astype(np.float64)) < 4e-16 and rel(kt, want.astype(np.float64)).max() < 1e-15


def test_the_d_equals_zero_rules_of_the_yardstick():
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, -1.0, 0.5]]); mass = [2.0, 3.0, 5.0]
    # eps == 0: a point on two coincident bodies drops both pairs; per body, the coincident partner is dropped too
    phi, t6 = R.direct(pos, mass, pos[:1], eps=0.0)
    ref_phi, ref_t = R.direct(pos[2:], mass[2:], pos[:1], eps=0.0)
    assert phi.tobytes() == ref_phi.tobytes() and t6.tobytes() == ref_t.tobytes()
    sphi, st = R.direct(pos, mass, pos, eps=0.0, skip_self=True)
    assert sphi[0] == phi[0] and sphi[1] == phi[0] and st[0].tobytes() == t6[0].tobytes()
    # eps > 0: the extra -G m / eps and -G m / eps^3 on the diagonal
    eps = 0.5
    phi, t6 = R.direct(pos[1:], mass[1:], pos[:1], eps=eps, dtype=LD)
    ref_phi, ref_t = R.direct(pos[2:], mass[2:], pos[:1], eps=eps, dtype=LD)
    assert abs(float(phi[0] - (ref_phi[0] - LD(G) * 3 / LD(eps)))) < 1e-15 * abs(float(phi[0]))
    assert np.abs((t6[0, :3] - (ref_t[0, :3] - LD(G) * 3 / LD(eps) ** 3)).astype(np.float64)).max() < 1e-15 * float(np.abs(t6).max())
    assert (t6[0, 3:] == ref_t[0, 3:]).all()
    # a single body: zeros, and the time scale of nothing is +inf
    phi, t6 = R.direct(pos[:1], mass[:1], pos[:1], skip_self=True)
    assert not phi.any() and not t6.any() and R.tidal_time_of(t6) == (np.inf, 0)
    kp, kt = R.kernel_order(pos[:1], mass[:1])
    assert not kp.any() and not kt.any()


def test_the_tidal_time_rule():
    t6 = np.array([[1.0, 2.0, 3.0, 0.5, 0.25, 0.125], [3.0, 2.0, 1.0, 0.5, 0.25, 0.125], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    n2 = 14.0 + 2.0 * (0.25 + 0.0625 + 0.015625)
    assert R.n2_of(t6).tolist() == [n2, n2, 0.0]
    assert R.tidal_time_of(t6) == (float(1.0 / np.sqrt(np.sqrt(n2))), 0)          # the lowest index of equal maxima
    assert R.tidal_time_of(np.array([[np.inf, 0, 0, 0, 0, 0.0]])) == (0.0, 0) and R.tidal_time_of(np.array([[np.nan, 0, 0, 0, 0, 0.0]])) == (0.0, 0)


@pytest.mark.parametrize("n", [257, 1000, 1025])
@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_the_kernels_order_stays_far_below_the_bound_of_the_gpu_tests(nb, n, eps):
    """The restated summation order against the long-double sums on the GPU tests' scenes: measured at most 1.3e-15 for phi and
    1.6e-14 for |dT|_F / |T|_F (N = 257, 1000, 1025; eps 0, 0.05), two orders below TOL_F64 = 1e-12.  The assertion leaves a factor of
    ten under the bound for what the restatement does not model (fused multiply-adds, the device's reciprocal root: a few ulp a pair)."""
    posm, _, tpos, _ = R.plummer_scene(nb, n, 25)
    lp, lt = R.direct(posm[:, :3], posm[:, 3], tpos, eps=eps, dtype=LD)
    kp, kt = R.kernel_order(posm[:, :3], posm[:, 3], tpos, eps=eps)
    ep, et = R.rel_phi(kp, lp.astype(np.float64)), rel(kt, lt.astype(np.float64)).max()
    lp, lt = R.direct(posm[:, :3], posm[:, 3], posm[:, :3], eps=eps, skip_self=True, dtype=LD)
    kp, kt = R.kernel_order(posm[:, :3], posm[:, 3], eps=eps)
    bp, bt = R.rel_phi(kp, lp.astype(np.float64)), rel(kt, lt.astype(np.float64)).max()
    print(f"N = {n}, eps = {eps}: points phi {ep:.3e}, T {et:.3e}; bodies phi {bp:.3e}, T {bt:.3e} of the long-double sums")
    assert max(ep, et, bp, bt) < 0.1 * TOL_F64
