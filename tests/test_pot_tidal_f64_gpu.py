"""The fp64 potential, tidal tensor and snap at points — nbody_potential_at_f64, nbody_get_potentials_f64, nbody_tidal_at_f64,
nbody_get_tidal_f64, nbody_tidal_time_f64, nbody_snap_at_f64 — on the device.

Three yardsticks.  The long-double sums of tests/pot_tidal_f64_ref.py (and tests/tracers_f64_ref.py: point_snap) hold the values to
the project's fp64 parity bound; tests/test_pot_tidal_f64_ref.py shows the kernel's summation order two orders below it on these
scenes.  A second fp64 context that holds the points appended as bodies of mass 0 (N + M <= 32768: 256-body chunks in both) holds the
point forms BYTE FOR BYTE to the per-body forms, as tests/test_tracers_f64_gpu.py explains.  And the per-body forms hold a body asked
about as a point, at eps == 0, byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pot_tidal_f64_ref as R
import tracers_f64_ref as TR
from jerk_ref import G, direct_jerk, probe_geometry, rel

pytestmark = pytest.mark.gpu

DT = 1e-3
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
LD = np.longdouble
CASES = [(1000, 25), (257, 300)]
EPS = [0.0, 0.05]
_scenes, _refs = {}, {}


def scene(nb, n, m=0):
    """(posm, vel, tpos, tvel) in fp64, read-only: test_tracers_f64_gpu.py's scene."""
    if (n, m) not in _scenes:
        _scenes[(n, m)] = R.plummer_scene(nb, n, m)
        for a in _scenes[(n, m)]:
            a.setflags(write=False)
    return _scenes[(n, m)]


def ld_points(nb, n, m, eps):
    """(phi, T) of the long-double sum at the scene's points, as float64; computed once."""
    key = ("points", n, m, eps)
    if key not in _refs:
        posm, _, tpos, _ = scene(nb, n, m)
        _refs[key] = tuple(x.astype(np.float64) for x in R.direct(posm[:, :3], posm[:, 3], tpos, eps=eps, dtype=LD))
    return _refs[key]


def ld_bodies(nb, n, eps, rows=None):
    """(phi, T) of the long-double per-body sum (rows: those bodies alone), as float64; computed once."""
    key = ("bodies", n, eps, None if rows is None else tuple(rows))
    if key not in _refs:
        posm = scene(nb, n)[0]
        if rows is None:
            got = R.direct(posm[:, :3], posm[:, 3], posm[:, :3], eps=eps, skip_self=True, dtype=LD)
        else:                                                      # a body's own pair has d == 0: give it no mass instead of an index
            phi, t6 = np.empty(len(rows), LD), np.empty((len(rows), 6), LD)
            for k, i in enumerate(rows):
                mass = posm[:, 3].copy(); mass[i] = 0.0
                p, t = R.direct(posm[:, :3], mass, posm[i:i + 1, :3], eps=eps, dtype=LD)
                phi[k], t6[k] = p[0], t[0]
            got = (phi, t6)
        _refs[key] = tuple(x.astype(np.float64) for x in got)
    return _refs[key]


def augmented(posm, vel, tpos, tvel):
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
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1]


def eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int((a != b).reshape(a.shape[0], -1).any(axis=-1).sum())} of {a.shape[0]} rows differ"


def probe_slab_points(n_total, width):
    """kernels_probe.hip's: the points whose partial rows (width float4 per point and chunk) fit 256 MiB, a multiple of 1024."""
    return max(1024, (256 << 20) // (probe_geometry(n_total)[0] * 16 * width) // 1024 * 1024)


def six_calls(e, pts, pv):
    return (e.potential_at_f64(pts), e.potentials_f64(), e.tidal_at_f64(pts), e.tidal_f64(), e.tidal_time_f64(), e.snap_at_f64(pts, pv))


# ---- 1: accuracy at points -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("eps", EPS)
def test_points_against_the_long_double_sum(nb, n, m, eps):
    posm, vel, tpos, _ = scene(nb, n, m)
    lp, lt = ld_points(nb, n, m, eps)
    with f64(nb, n, eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0 = passes(nb, e)
        phi = e.potential_at_f64(tpos)
        f1 = passes(nb, e)
        t6 = e.tidal_at_f64(tpos)
        f2 = passes(nb, e)
        assert (f1 - f0, f2 - f1) == (1, 1)                        # one pass under NBODY_KERNEL_FORCES each
        ep, et = R.rel_phi(phi, lp), rel(t6, lt).max()
        print(f"N = {n}, M = {m}, eps = {eps}: phi {ep:.3e}, T {et:.3e} of the long-double sum")
        assert phi.shape == (m,) and t6.shape == (m, 6)
        assert ep < TOL_F64 and et < TOL_F64
        # strides of the caller's own: the padding stays
        P, L = tpos.ctypes.data, e._L
        wide = np.full((m, 3), -1.0)
        assert L.nbody_potential_at_f64(e._h, P, 24, m, wide.ctypes.data, 24) == 0
        eq(wide[:, 0], phi, "phi into strided rows"); assert (wide[:, 1:] == -1.0).all()
        wide = np.full((m, 8), -1.0)
        assert L.nbody_tidal_at_f64(e._h, P, 24, m, wide.ctypes.data, 64) == 0
        eq(wide[:, :6], t6, "T into strided rows"); assert (wide[:, 6:] == -1.0).all()
        pts5 = np.full((m, 5), 7.0); pts5[:, :3] = tpos            # strided points
        out = np.empty(m)
        assert L.nbody_potential_at_f64(e._h, pts5.ctypes.data, 40, m, out.ctypes.data, 8) == 0
        eq(out, phi, "phi of strided points")
        p, v, _ = e.state(np.float64)
        eq(p, posm, "positions"); eq(v, vel, "velocities")


# ---- 2: accuracy per body --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("eps", EPS)
def test_bodies_against_the_long_double_sum(nb, n, eps):
    posm, vel, _, _ = scene(nb, n)
    lp, lt = ld_bodies(nb, n, eps)
    with f64(nb, n, eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0 = passes(nb, e)
        phi = e.potentials_f64(); f1 = passes(nb, e)
        t6 = e.tidal_f64(); f2 = passes(nb, e)
        assert (f1 - f0, f2 - f1) == (1, 1)
        ep, et = R.rel_phi(phi, lp), rel(t6, lt).max()
        print(f"N = {n}, eps = {eps}: per body phi {ep:.3e}, T {et:.3e} of the long-double sum")
        assert ep < TOL_F64 and et < TOL_F64
        wide = np.full((n, 9), -1.0)                               # a stride of its own
        assert e._L.nbody_get_tidal_f64(e._h, wide.ctypes.data, 72) == 0
        eq(wide[:, :6], t6, "T into strided rows"); assert (wide[:, 6:] == -1.0).all()
        wide = np.full((n, 2), -1.0)
        assert e._L.nbody_get_potentials_f64(e._h, wide.ctypes.data, 16) == 0
        eq(wide[:, 0], phi, "phi into strided rows"); assert (wide[:, 1] == -1.0).all()


def test_bodies_at_512_body_chunks(nb):
    """N = 32769: the first size with 512-body chunks, 65 of them — a geometry no smaller case reaches.  All bodies are computed; 64
    sampled ones and 3 caller points are held to the long-double sum."""
    n, eps = 32769, 0.05
    assert probe_geometry(n) == (65, 512)
    posm, vel, tpos, _ = scene(nb, n, 3)
    rows = list(range(0, n, n // 63))[:63] + [n - 1]
    assert len(rows) == 64
    lp, lt = ld_bodies(nb, n, eps, rows)
    pp, pt = ld_points(nb, n, 3, eps)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        phi, t6 = e.potentials_f64(), e.tidal_f64()
        ep, et = R.rel_phi(phi[rows], lp), rel(t6[rows], lt).max()
        qp, qt = R.rel_phi(e.potential_at_f64(tpos), pp), rel(e.tidal_at_f64(tpos), pt).max()
        print(f"N = {n}: per body phi {ep:.3e}, T {et:.3e}; points phi {qp:.3e}, T {qt:.3e} of the long-double sum")
        assert max(ep, et, qp, qt) < TOL_F64
        assert np.isfinite(phi).all() and np.isfinite(t6).all() and (phi < 0).all()
        assert R.tidal_time_of(t6) == e.tidal_time_f64()           # the reduction over more bodies than one workgroup per slot


# ---- 3: bit identities -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("eps", EPS)
def test_points_against_the_augmented_context(nb, n, m, eps):
    posm, vel, tpos, tvel = scene(nb, n, m)
    ap, av = augmented(posm, vel, tpos, tvel)
    with f64(nb, n, eps=eps) as e, f64(nb, n + m, eps=eps) as aug:
        e.set_state(posm, vel); aug.set_state(ap, av)
        eq(e.potential_at_f64(tpos), aug.potentials_f64()[n:], "phi against the augmented rows")
        eq(e.tidal_at_f64(tpos), aug.tidal_f64()[n:], "T against the augmented rows")
        # and the massless bodies change no real body's row
        eq(e.potentials_f64(), aug.potentials_f64()[:n], "the bodies' phi"); eq(e.tidal_f64(), aug.tidal_f64()[:n], "the bodies' T")


@pytest.mark.parametrize("n", [257, 1025])
def test_at_the_bodies_own_positions_is_the_per_body_call(nb, n):
    posm, vel, _, _ = scene(nb, n)
    rng = np.random.default_rng(n)
    with f64(nb, n, eps=0.0) as e:
        e.set_state(posm, vel)
        phi, t6 = e.potentials_f64(), e.tidal_f64()
        subset = rng.permutation(np.arange(max(n, 300)) % n)[:300]
        forms = [np.arange(n), subset, np.array([n - 1])] + [np.arange(m) % n for m in (255, 256, 257, 512, 513)]
        for idx in forms:
            eq(e.potential_at_f64(posm[idx, :3]), phi[idx], f"phi of {idx.size} points")
            eq(e.tidal_at_f64(posm[idx, :3]), t6[idx], f"T of {idx.size} points")


def test_points_beyond_one_slab_of_the_staging_area(nb):
    """N = 33000 (test_tracers_f64_gpu.py's): 65 chunks, so a slab of the tensor's rows (four float4 per point and chunk) is 64512
    points and one of the potential's (one float4) 258048.  450 more: 300 points round the boundary, the last 300 not overlapping."""
    n = 33000
    assert probe_geometry(n) == (65, 512)
    posm, vel, _, _ = scene(nb, n)
    with f64(nb, n, eps=0.05) as e:
        e.set_state(posm, vel)
        for width, call, slab_want in ((4, e.tidal_at_f64, 64512), (1, e.potential_at_f64, 258048)):
            slab = probe_slab_points(n, width)
            assert slab == slab_want
            m = slab + 450
            pts = np.random.default_rng(width).normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
            whole = call(pts)
            for lo in (0, slab - 150, m - 300):
                eq(whole[lo:lo + 300], call(pts[lo:lo + 300]), f"width {width}: points {lo} .. {lo + 300}")


# ---- 4: the snap at points -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("eps", EPS)
def test_snap_at_f64_at_the_bodies_own_state_is_get_snap_f64(nb, n, eps):
    posm, vel, _, _ = scene(nb, n)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        want = e.snap()
        subset = np.random.default_rng(n).permutation(np.arange(max(n, 300)) % n)[:300]
        for idx in (np.arange(n), subset):
            got = e.snap_at_f64(posm[idx, :3], vel[idx, :3])
            for name, a, b in zip(("acc", "jerk", "snap"), got, want):
                eq(a, b[idx], f"{name} of {idx.size} points")
        for a, b in zip(e.snap(), want):                           # (and nbody_get_snap_f64 is what it was behind it)
            eq(a, b, "snap() again")


@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("eps", EPS)
def test_snap_at_f64_at_moving_points(nb, n, m, eps):
    posm, vel, tpos, tvel = scene(nb, n, m)
    acc_in = direct_jerk(posm[:, :3], posm[:, 3], vel, posm[:, :3], vel, eps=eps, skip_self=True, dtype=LD)[0]
    pacc = direct_jerk(posm[:, :3], posm[:, 3], vel, tpos, tvel, eps=eps, dtype=LD)[0]
    want = TR.point_snap(posm, vel, acc_in, tpos, tvel, pacc, eps=eps, dtype=LD)
    with f64(nb, n, eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        f0 = passes(nb, e)
        got = e.snap_at_f64(tpos, tvel)
        assert passes(nb, e) - f0 == 3                             # the bodies' jerk pass, the point jerk pass, the point snap pass
        errs = [rel(a, b.astype(np.float64)).max() for a, b in zip(got, want)]
        print(f"N = {n}, M = {m}, eps = {eps}: acc {errs[0]:.3e}, jerk {errs[1]:.3e}, snap {errs[2]:.3e} of the long-double sum")
        assert max(errs) < TOL_F64
        aj = e.jerk_at_f64(tpos, tvel)
        eq(got[0], aj[0], "acc is jerk_at_f64's"); eq(got[1], aj[1], "jerk is jerk_at_f64's")
        for a, b in zip(e.snap_at_f64(tpos), e.snap_at_f64(tpos, np.zeros_like(tpos))):
            eq(a, b, "at rest")
        P, V, L = tpos.ctypes.data, tvel.ctypes.data, e._L
        for k in range(3):                                         # each output alone, into strided rows
            wide = np.full((m, 4), -1.0)
            args = [None, 0, None, 0, None, 0]
            args[2 * k], args[2 * k + 1] = wide.ctypes.data, 32
            assert L.nbody_snap_at_f64(e._h, P, 24, V, 24, m, *args) == 0
            eq(wide[:, :3], got[k], f"output {k} alone"); assert (wide[:, 3] == -1.0).all()


# ---- 5: the tidal time scale -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", EPS)
def test_tidal_time_f64_is_the_rule_on_tidal_f64(nb, eps):
    n = 1025
    posm, vel, _, _ = scene(nb, n)
    with f64(nb, n, eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        t6 = e.tidal_f64()
        f0 = passes(nb, e)
        got = e.tidal_time_f64()
        assert passes(nb, e) - f0 == 1
        assert got == R.tidal_time_of(t6) and 0 <= got[1] < n and 0 < got[0] < np.inf
        t, body = ctypes.c_double(), ctypes.c_int32(-1)           # either output alone
        assert e._L.nbody_tidal_time_f64(e._h, None, ctypes.byref(body)) == 0 and body.value == got[1]
        assert e._L.nbody_tidal_time_f64(e._h, ctypes.byref(t), None) == 0 and t.value == got[0]


def test_tidal_time_f64_of_one_and_of_two_bodies(nb):
    with f64(nb, 1) as e:
        e.set_state(np.array([[1.5, -2.25, 3.0, 7.0]]), np.zeros((1, 4)))
        assert e.tidal_time_f64() == (np.inf, 0)
        assert not e.potentials_f64().any() and not e.tidal_f64().any()
    posm = np.array([[1.5, -2.25, 3.0, 7.0], [-0.5, 1.0, 4.25, 11.0]]); vel = np.zeros((2, 4))
    d = (posm[1, :3] - posm[0, :3]).astype(LD)
    r = np.sqrt((d * d).sum())
    with f64(nb, 2) as e:
        e.set_state(posm, vel)
        t, body = e.tidal_time_f64()
        # body 0 feels the heavier one: ||T||_F = sqrt(6) G m / r^3
        want = 1 / np.sqrt(np.sqrt(LD(6)) * LD(G) * LD(11.0) / r ** 3)
        assert body == 0 and abs(t - float(want)) < TOL_F64 * float(want)
        t6 = e.tidal_f64().astype(LD)
        for i, mj, sign in ((0, 11.0, 1), (1, 7.0, -1)):
            dd = sign * d
            ref = np.array([LD(G) * LD(mj) * (3 * dd[a] * dd[b] / r ** 5 - (1 if a == b else 0) / r ** 3) for a, b in R.PAIRS])
            assert rel(t6[i:i + 1].astype(np.float64), ref[None, :].astype(np.float64)).max() < TOL_F64
        phi = e.potentials_f64()
        assert abs(phi[0] + float(LD(G) * 11 / r)) < TOL_F64 * abs(phi[0]) and abs(phi[1] + float(LD(G) * 7 / r)) < TOL_F64 * abs(phi[1])


# ---- 6: d == 0 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", EPS)
def test_a_point_exactly_on_a_body(nb, eps):
    n, k = 1000, 417
    posm, vel, _, _ = scene(nb, n, 25)
    pt = posm[k:k + 1, :3].copy()
    massless = posm.copy(); massless[k, 3] = 0.0                   # the scene without that body, every other body in its chunk
    with f64(nb, n, eps=eps) as e, f64(nb, n, eps=eps) as without:
        e.set_state(posm, vel); without.set_state(massless, vel)
        phi, t6 = e.potential_at_f64(pt), e.tidal_at_f64(pt)
        wphi, wt6 = without.potential_at_f64(pt), without.tidal_at_f64(pt)
        if eps == 0.0:                                             # the pair is dropped from every sum
            eq(phi, wphi, "phi: the pair is dropped"); eq(t6, wt6, "T: the pair is dropped")
            eq(phi, e.potentials_f64()[k:k + 1], "phi: the body's own row"); eq(t6, e.tidal_f64()[k:k + 1], "T: the body's own row")
        else:                                                      # -G m / eps in phi, -G m / eps^3 on the diagonal, nothing off it
            gm = LD(G) * LD(posm[k, 3])
            want = LD(wphi[0]) - gm / LD(eps)
            assert abs(float(LD(phi[0]) - want)) < TOL_F64 * abs(float(want))
            extra = (t6[0, :3].astype(LD) - wt6[0, :3].astype(LD)).astype(np.float64)
            want = float(-gm / (LD(eps) * LD(eps) * LD(eps)))
            assert np.abs(extra - want).max() < TOL_F64 * abs(want)
            eq(t6[:, 3:], wt6[:, 3:], "T: the off-diagonals")
            # the per-body row leaves the body out by index: it is the massless scene's
            eq(e.potentials_f64()[k:k + 1], wphi, "phi: the body's own row"); eq(e.tidal_f64()[k:k + 1], wt6, "T: the body's own row")


def test_two_coincident_bodies_at_eps_zero_drop_each_other(nb):
    n, a, b = 1000, 417, 700
    posm, vel, _, _ = scene(nb, n, 25)
    both = posm.copy(); both[b, :3] = both[a, :3]
    with f64(nb, n) as e:
        e.set_state(both, vel)
        phi, t6 = e.potentials_f64(), e.tidal_f64()
        assert np.isfinite(phi).all() and np.isfinite(t6).all()
        for row, other in ((a, b), (b, a)):
            alone = both.copy(); alone[other, 3] = 0.0
            e.set_state(alone, vel)
            eq(phi[row:row + 1], e.potentials_f64()[row:row + 1], f"phi of body {row}"); eq(t6[row:row + 1], e.tidal_f64()[row:row + 1], f"T of body {row}")


# ---- 7: nothing else moves -------------------------------------------------------------------------------------------------------------

def fourth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite_state() + e.hermite_tracers_state()


def sixth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite6_state() + e.hermite6_tracers_state()


def test_the_caches_and_the_tracers_stay(nb):
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    with f64(nb, n, eps=0.05) as e, f64(nb, n, eps=0.05) as twin:
        for x in (e, twin):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
            x.hermite6_step(DT, 2); x.hermite_timescale(); x.hermite_tracers_timescale()   # both orders' caches, bodies and tracers
        before = fourth(e) + sixth(e)
        six_calls(e, tpos, tvel)
        for k, (a, b) in enumerate(zip(fourth(e) + sixth(e), before)):
            eq(a, b, f"array {k} behind the six calls")
        e.hermite6_step(DT, 1); twin.hermite6_step(DT, 1)          # and the steps behind them go on as the twin's
        for k, (a, b) in enumerate(zip(sixth(e), sixth(twin))):
            eq(a, b, f"array {k} a sixth-order step later, against the twin")
        e.hermite_step(DT, 1); twin.hermite_step(DT, 1)
        for k, (a, b) in enumerate(zip(fourth(e), fourth(twin))):
            eq(a, b, f"array {k} a fourth-order step later, against the twin")


@pytest.mark.parametrize("order", [4, 6])
def test_a_block_session_in_mid_frame_goes_on_as_its_twin(nb, order):
    n, m, levels = 257, 25, 8
    posm, vel, tpos, tvel = scene(nb, n, m)
    lb = (np.arange(n) % 4).astype(np.int32); lt = (np.arange(m) % 5).astype(np.int32)
    begin = (lambda x: x.hermite_block_begin_tracers(DT, levels, level_in=lb, tracer_level_in=lt)) if order == 4 else \
            (lambda x: x.hermite6_block_begin_tracers(DT, levels, level_in=lb, tracer_level_in=lt))
    advance = (lambda x, **kw: x.hermite_block_advance(1, **kw)) if order == 4 else (lambda x, **kw: x.hermite6_block_advance(1, **kw))

    def session(x):
        cache = x.hermite_state() + x.hermite_tracers_state() if order == 4 else x.hermite6_state() + x.hermite6_tracers_state()
        ticks = x.hermite_block_state() + x.hermite_block_tracers_state()[:2] if order == 4 else \
            x.hermite6_block_state() + x.hermite6_block_tracers_state()[:2]
        return x.state(np.float64) + x.tracers_f64() + cache + ticks

    with f64(nb, n, eps=0.05) as e, f64(nb, n, eps=0.05) as twin:
        for x in (e, twin):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
            begin(x)
            st = advance(x, max_block_steps=3)
            assert not st["synchronised"] and st["block_steps"] == 3
        before = session(e)
        six_calls(e, tpos, tvel)
        for k, (a, b) in enumerate(zip(session(e), before)):
            eq(a, b, f"array {k} behind the six calls, in mid-frame")
        se, sw = advance(e), advance(twin)
        assert se == sw and se["synchronised"]
        for k, (a, b) in enumerate(zip(session(e), session(twin))):
            eq(a, b, f"array {k} at the frame end, against the twin")


# ---- 8: the contract -------------------------------------------------------------------------------------------------------------------

NAMES = ("nbody_potential_at_f64", "nbody_get_potentials_f64", "nbody_tidal_at_f64", "nbody_get_tidal_f64", "nbody_tidal_time_f64",
         "nbody_snap_at_f64")


def six_lambdas(e):
    pts = np.zeros((3, 3)) + [[1.0], [2.0], [3.0]]
    return ((lambda: e.potential_at_f64(pts)), e.potentials_f64, (lambda: e.tidal_at_f64(pts)), e.tidal_f64, e.tidal_time_f64,
            (lambda: e.snap_at_f64(pts)))


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    """tests/cpp/fake_rccl.c, the suite's stand-in for the communication library, as tests/test_tracers_f64_gpu.py builds it: a
    multi-device context over device 0 alone needs no real communicator to refuse a call."""
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
            for name, call in zip(NAMES, six_lambdas(e)):
                msg = raises(nb, E.ERR_UNSUPPORTED, call)
                assert name in msg and why in msg, (kw, msg)
    n, m = 257, 25
    posm, vel, tpos, tvel = scene(nb, n, m)
    with f64(nb, n) as e:
        for call in six_lambdas(e):                                # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(posm, vel)
        # what the fp32 calls report on an fp64 context is what it was
        for call in ((lambda: e.potential_at(pts32)), e.potentials, (lambda: e.tidal_at(pts32)), e.tidal, e.tidal_time):
            raises(nb, E.ERR_UNSUPPORTED, call)
        out = np.empty((m, 9))
        P, V, O, L = tpos.ctypes.data, tvel.ctypes.data, out.ctypes.data, e._L
        for f, low in ((L.nbody_potential_at_f64, 8), (L.nbody_tidal_at_f64, 48)):
            assert f(e._h, None, 24, m, O, 72) == E.ERR_INVALID                                         # null points
            assert f(e._h, P, 24, m, None, 72) == E.ERR_INVALID                                         # null output
            assert f(e._h, P, 24, -1, O, 72) == E.ERR_INVALID                                           # n < 0
            assert f(e._h, P, 23, m, O, 72) == E.ERR_INVALID and f(e._h, P, 24, m, O, low - 1) == E.ERR_INVALID   # short strides
            assert f(e._h, None, 0, 0, None, 0) == E.ERR_INVALID and f(e._h, None, 24, 0, O, 72) == E.ERR_INVALID   # null even with n == 0
            before = out.copy()
            assert f(e._h, P, 24, 0, O, low) == 0 and out.tobytes() == before.tobytes()                   # n == 0: a no-op
            assert f(e._h, P, 24, m, O, low) == 0
        for f, low in ((L.nbody_get_potentials_f64, 8), (L.nbody_get_tidal_f64, 48)):
            big_out = np.empty((n, 9))
            assert f(e._h, None, 72) == E.ERR_INVALID and f(e._h, big_out.ctypes.data, low - 1) == E.ERR_INVALID
            assert f(e._h, big_out.ctypes.data, low) == 0
        assert L.nbody_tidal_time_f64(e._h, None, None) == E.ERR_INVALID
        S = L.nbody_snap_at_f64
        assert S(e._h, None, 24, None, 24, m, O, 24, O, 24, O, 24) == E.ERR_INVALID                      # null points
        assert S(e._h, P, 24, V, 24, -1, O, 24, O, 24, O, 24) == E.ERR_INVALID                           # n < 0
        assert S(e._h, P, 24, V, 24, m, None, 24, None, 24, None, 24) == E.ERR_INVALID                   # all three outputs null
        for k in range(5):
            strides = [24] * 5; strides[k] = 23
            assert S(e._h, P, strides[0], V, strides[1], m, O, strides[2], O, strides[3], O, strides[4]) == E.ERR_INVALID
        assert S(e._h, P, 24, None, 0, m, O, 24, None, 0, None, 0) == 0                                  # (strides of absent arrays are not looked at)
        assert S(e._h, None, 0, None, 0, 0, None, 0, None, 0, None, 0) == E.ERR_INVALID                  # null points even with n == 0
        assert S(e._h, P, 24, None, 0, 0, O, 24, None, 0, None, 0) == 0                                  # n == 0: a no-op
        a, j, s = e.snap_at_f64(np.zeros((0, 3)))
        assert a.shape == j.shape == s.shape == (0, 3) and e.potential_at_f64(np.zeros((0, 3))).shape == (0,) and e.tidal_at_f64(np.zeros((0, 3))).shape == (0, 6)
        e.step_begin()                                             # a step is open
        for name, call in zip(NAMES, six_lambdas(e)):
            assert name in raises(nb, E.ERR_STATE, call)
        e.step_end(0.0)
        six_calls(e, tpos, tvel)
