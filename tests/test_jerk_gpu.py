"""The jerk j = da/dt beside the acceleration: nbody_jerk_at (at caller-given moving points), nbody_get_jerk / nbody_get_jerk_f64 (at the
bodies, self excluded by index) and nbody_jerk_time (the smallest |a_i| / |j_i| and its body) against the numpy direct sums of
tests/jerk_ref.py; the pair sum at every theta, on all three precisions; the argument and context errors of all four.

The error of a vector is |got - ref| / |ref|.  fp32 state: the bound is TOL_ACC (2e-5, the project's all-pairs bound) against the fp64
direct sum.  Next to every case stands what the kernel's arithmetic alone gives on that scene — emulate_jerk_f32 of tests/jerk_ref.py,
fp32 per pair and per chunk with a correctly rounded root, fp64 fold, run on the CPU by tests/test_jerk_ref.py, (acc, jerk) — which is
to stay below a quarter of the bound, the rest being v_rsq_f32's ulp.  fp64 state: 1e-12 against the long-double sum, the fp64 parity
bound of tests/test_parity_gpu.py (sums in the kernel's order sit at 1.4e-14 on plummer_n1024_seed1).

Partial rows at N = 20000 (probe_geometry: 79 chunks of 256 bodies; a jerk row is two float4 per point and chunk, as the tidal
tensor's): probe_slab_points(20000, 2) = 105472 points per slab; a workgroup takes 1024 points instead of 512 from M = 12289 on.
M = 106072 is 600 points into the second slab: the first slab runs the 1024-point shape, the second the 512-point one, and every
sub-range asked for alone the 512-point one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jerk_ref import G, direct_jerk, jerk_time_of, k_of, probe_geometry, probe_velocities, rel
from probe_scenes import GOLDEN, TOL_ACC, bodies, probes_for

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-12


def slab_points(n_total, width):
    return max(1024, (256 << 20) // (probe_geometry(n_total)[0] * 16 * width) // 1024 * 1024)


N_MANY = 20000
SLAB = slab_points(N_MANY, 2)
WG2 = 1024 * ((1024 + probe_geometry(N_MANY)[0] - 1) // probe_geometry(N_MANY)[0] - 1) + 1   # the smallest M of the 1024-point shape
M_MANY = SLAB + 600
assert (probe_geometry(N_MANY), SLAB, WG2, M_MANY) == ((79, 256), 105472, 12289, 106072)

_direct = {}


def direct_self(n, posm, vel, eps=0.0, dtype=np.float64):
    """The bodies' own (acc, jerk) by the direct sum, computed once per scene."""
    key = (n, eps, dtype, posm.tobytes()[:64], vel.tobytes()[:64])
    if key not in _direct:
        ra, rj = direct_jerk(posm[:, :3], posm[:, 3], vel, posm[:, :3], vel, eps=eps, skip_self=True, dtype=dtype)
        ra = ra.astype(np.float64); rj = rj.astype(np.float64)
        ra.setflags(write=False); rj.setflags(write=False)
        _direct[key] = (ra, rj)
    return _direct[key]


def check(what, got, ref, tol, emulated=None):
    ga, gj = got
    ra, rj = ref
    assert ga.shape == ra.shape and gj.shape == rj.shape and np.isfinite(ga).all() and np.isfinite(gj).all()
    ea, ej = rel(ga, ra), rel(gj, rj)
    print(f"{what}: max err acc {ea.max():.3e} jerk {ej.max():.3e}" + (f" (emulated {emulated[0]:.1e}, {emulated[1]:.1e})" if emulated else ""))
    if emulated:
        assert max(emulated) <= TOL_ACC / 4
    assert ea.max() < tol, (what, "acc", int(ea.argmax()), ea.max())
    assert ej.max() < tol, (what, "jerk", int(ej.argmax()), ej.max())


# ---- 1, 2: per body, fp32 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,eps,emulated", [(2000, 0.0, (1.9e-6, 2.7e-6)), (2000, 0.05, (1.9e-6, 3.0e-6)), (257, 0.0, (1.2e-6, 1.4e-6))])
def test_jerk_is_the_direct_sum_without_the_body_itself(nb, n, eps, emulated):
    # N = 2000: 8 tiles, the own-tile guard at bodies 255 / 256 and 511 / 512 (the 512 bodies of workgroup 0 span tiles 0 and 1);
    # N = 257: one full tile and a ragged, padded one
    posm, vel = bodies(nb, n)
    ref = direct_self(n, posm, vel, eps)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.jerk()
        got64 = e.jerk(np.float64)
        e.compute_forces()
        stored = e.accelerations()
        again = e.jerk()
    assert got[0].dtype == np.float32 and got[0].shape == (n, 3) and got64[0].dtype == np.float64
    check(f"jerk() N={n} eps={eps}", got, ref, TOL_ACC, emulated)
    for k in (255, 256, 511, 512):
        if k < n:
            assert rel(got[0][k:k + 1], ref[0][k:k + 1])[0] < TOL_ACC and rel(got[1][k:k + 1], ref[1][k:k + 1])[0] < TOL_ACC, k
    # the float form is the fp64 fold rounded once
    assert got[0].tobytes() == got64[0].astype(np.float32).tobytes() and got[1].tobytes() == got64[1].astype(np.float32).tobytes()
    # the stored accelerations of a force pass: another arithmetic, the same sum
    assert rel(got[0], stored.astype(np.float64)).max() < 2 * TOL_ACC
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


def test_a_single_body_has_no_jerk(nb):
    posm, vel = bodies(nb, 1)
    for kw in ({}, {"precision": "f64"}, {"theta": 1.0}):
        with nb.NBodyEngine(1, **kw) as e:
            e.set_state(posm.astype(np.float64) if kw.get("precision") == "f64" else posm, vel.astype(np.float64) if kw.get("precision") == "f64" else vel)
            a, j = e.jerk()
            a64, j64 = e.jerk(np.float64)
            assert not a.any() and not j.any() and not a64.any() and not j64.any()
            assert e.jerk_time() == (float("inf"), 0)


def test_two_bodies_on_a_circular_orbit(nb):
    # m = 3 and 5 at x = -5 and 3 (r = 8), omega^2 = G * 8 / 512 = 156.25, omega = 12.5: every input and every answer an fp32 number
    assert G == 1.0e4
    posm = np.array([[-5, 0, 0, 3], [3, 0, 0, 5]], np.float32)
    vel = np.array([[0, -62.5, 0, 0], [0, 37.5, 0, 0]], np.float32)
    want_a = np.array([[781.25, 0, 0], [-468.75, 0, 0]])          # -omega^2 x
    want_j = np.array([[0, 9765.625, 0], [0, -5859.375, 0]])      # -omega^2 v
    for prec, tol in (("f32", TOL_ACC), ("f32_kahan", TOL_ACC), ("f64", TOL_F64)):
        with nb.NBodyEngine(2, precision=prec) as e:
            e.set_state(posm.astype(np.float64) if prec == "f64" else posm, vel.astype(np.float64) if prec == "f64" else vel)
            check(f"two bodies {prec}", e.jerk(np.float64), (want_a, want_j), tol)
            t, body = e.jerk_time()
            assert body == 0 and t == pytest.approx(1 / 12.5, rel=2 * tol)      # |a| / |j| = 1 / omega for both: the tie goes to body 0


def test_a_symmetric_pair_ties_at_body_0(nb):
    posm = np.array([[-1.5, 0.25, 0, 7], [1.5, -0.25, 0, 7]], np.float32)
    vel = np.array([[0.5, -3, 1, 0], [-0.5, 3, -1, 0]], np.float32)
    for prec in ("f32", "f64"):
        with nb.NBodyEngine(2, precision=prec) as e:
            e.set_state(posm.astype(np.float64) if prec == "f64" else posm, vel.astype(np.float64) if prec == "f64" else vel)
            a, j = e.jerk(np.float64)
            assert (a[0] == -a[1]).all() and (j[0] == -j[1]).all() and a[0].any() and j[0].any()
            assert e.jerk_time()[1] == 0


# ---- 3, 4: at points -----------------------------------------------------------------------------------------------------------------

# (n, m, eps, the emulation's max err (acc, jerk)); N = 20000: 79 chunks in the fold
AT_CASES = [(2000, 1, 0.0, (4.5e-8, 4.8e-8)), (2000, 64, 0.0, (6.1e-7, 2.3e-6)), (2000, 65, 0.0, (6.1e-7, 2.3e-6)),
            (2000, 777, 0.0, (6.1e-7, 2.3e-6)), (2000, 777, 0.05, (7.5e-7, 2.1e-6)), (20000, 100, 0.0, (6.5e-7, 1.8e-6))]


@pytest.mark.parametrize("n,m,eps,emulated", AT_CASES)
def test_direct_sum_at_every_moving_point(nb, n, m, eps, emulated):
    posm, vel = bodies(nb, n)
    pos, mass = posm[:, :3], posm[:, 3]
    pts, pv = probes_for(pos, m), probe_velocities(m)
    ref = direct_jerk(pos, mass, vel, pts, pv, eps=eps)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.jerk_at(pts, pv)
    assert got[0].dtype == np.float32 and got[0].shape == (m, 3) and got[1].shape == (m, 3)
    check(f"jerk_at N={n} M={m} eps={eps}", got, ref, TOL_ACC, emulated)
    if m >= 60 and eps > 0.0:
        # points 0-49 sit ON bodies 0-49: each feels that body's G m w / eps^3 in the jerk and nothing of it in the acceleration
        for k in range(50):
            keep = np.arange(n) != k
            wa, wj = direct_jerk(pos[keep], mass[keep], vel[keep], pts[k:k + 1], pv[k:k + 1], eps=eps)
            own = G * float(mass[k]) * (vel[k, :3].astype(np.float64) - pv[k].astype(np.float64)) / eps ** 3
            d = got[1][k].astype(np.float64) - wj[0]
            assert np.linalg.norm(d - own) <= 1e-4 * np.linalg.norm(own), k
            assert rel(got[0][k:k + 1], wa)[0] < TOL_ACC, k


# ---- 5: bits -------------------------------------------------------------------------------------------------------------------------

def test_bit_level_properties(nb):
    n, m = 2000, 777
    posm, vel = bodies(nb, n)
    pts, pv = probes_for(posm[:, :3], m), probe_velocities(m)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        e.step(0.01, 2)
        before = (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done())
        a, j = e.jerk_at(pts, pv)
        again = e.jerk_at(pts, pv)
        assert again[0].tobytes() == a.tobytes() and again[1].tobytes() == j.tobytes()
        # vel = None is an array of zeros
        r0, rz = e.jerk_at(pts), e.jerk_at(pts, np.zeros_like(pts))
        assert r0[0].tobytes() == rz[0].tobytes() and r0[1].tobytes() == rz[1].tobytes() and r0[0].tobytes() == a.tobytes()
        assert r0[1].tobytes() != j.tobytes()
        h = m // 2                                                 # a point does not see the others
        lo, hi = e.jerk_at(pts[:h], pv[:h]), e.jerk_at(pts[h:], pv[h:])
        assert np.concatenate([lo[0], hi[0]]).tobytes() == a.tobytes() and np.concatenate([lo[1], hi[1]]).tobytes() == j.tobytes()
        # strides in and out, through the C entry point itself
        rec = np.zeros(m, nb.PARTICLE_DTYPE)
        rec["Mass"] = 7.0; rec["Position"] = pts; rec["Velocity"] = pv
        f = e._L.nbody_jerk_at
        out = np.full((m, 10), 5.0, np.float32)
        assert f(e._h, rec["Position"].ctypes.data, 40, rec["Velocity"].ctypes.data, 40, m, out.ctypes.data, 40, out[:, 4:].ctypes.data, 40) == 0
        assert np.ascontiguousarray(out[:, :3]).tobytes() == a.tobytes() and np.ascontiguousarray(out[:, 4:7]).tobytes() == j.tobytes()
        assert (out[:, 3] == 5.0).all() and (out[:, 7:] == 5.0).all()
        only = np.full((m, 3), 5.0, np.float32)                    # either output alone
        assert f(e._h, pts.ctypes.data, 12, pv.ctypes.data, 12, m, only.ctypes.data, 12, None, 0) == 0 and only.tobytes() == a.tobytes()
        assert f(e._h, pts.ctypes.data, 12, pv.ctypes.data, 12, m, None, 0, only.ctypes.data, 12) == 0 and only.tobytes() == j.tobytes()
        only[:] = 5.0
        assert f(e._h, pts.ctypes.data, 12, pv.ctypes.data, 12, 0, only.ctypes.data, 12, None, 0) == 0 and (only == 5.0).all()   # n == 0
        ba, bj = e.jerk()
        big = np.full((n, 8), 5.0, np.float32)
        assert e._L.nbody_get_jerk(e._h, big.ctypes.data, 32, big[:, 4:].ctypes.data, 32) == 0
        assert np.ascontiguousarray(big[:, :3]).tobytes() == ba.tobytes() and np.ascontiguousarray(big[:, 4:7]).tobytes() == bj.tobytes()
        assert (big[:, 3] == 5.0).all() and (big[:, 7] == 5.0).all()
        big64 = np.full((n, 8), 5.0, np.float64)
        assert e._L.nbody_get_jerk_f64(e._h, None, 0, big64[:, 4:].ctypes.data, 64) == 0
        assert np.ascontiguousarray(big64[:, 4:7]).tobytes() == e.jerk(np.float64)[1].tobytes() and (big64[:, :4] == 5.0).all()
        assert e.jerk_time() == e.jerk_time()
        assert (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done()) == before


def test_many_points_across_the_workgroup_shapes_and_the_slab_boundary(nb):
    n, m = N_MANY, M_MANY
    posm, vel = bodies(nb, n)
    pos = posm[:, :3]
    pts, pv = probes_for(pos, m), probe_velocities(m)
    pts[SLAB - 25:SLAB - 15] = pos[200:210]                       # on bodies and beside bodies on either side of the slab boundary
    pts[SLAB + 15:SLAB + 25] = pos[210:220] + np.float32(1e-3)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        a, j = e.jerk_at(pts, pv)
        assert a.shape == (m, 3) and np.isfinite(a).all() and np.isfinite(j).all()
        ranges = [(0, 777), (1024 - 3, 1024 + 300), (WG2 - 101, WG2 + 99), (0, WG2 - 1), (0, WG2), (SLAB - 300, SLAB + 300), (SLAB, SLAB + 1),
                  (SLAB - 1, SLAB), (SLAB, m), (m - 1, m)]
        for lo, hi in ranges:
            sa, sj = e.jerk_at(pts[lo:hi], pv[lo:hi])
            assert sa.tobytes() == a[lo:hi].tobytes() and sj.tobytes() == j[lo:hi].tobytes(), (lo, hi)
    sample = np.unique(np.concatenate([np.arange(SLAB - 30, SLAB + 30), np.arange(m - 20, m), np.random.default_rng(9).integers(0, m, 100)]))
    ref = direct_jerk(pos, posm[:, 3], vel, pts[sample], pv[sample])
    check(f"jerk_at N={n} M={m} on {sample.size} sampled points", (a[sample], j[sample]), ref, TOL_ACC)


# ---- 6: coincident bodies -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_two_coincident_bodies(nb, eps):
    n = 300
    posm, vel = bodies(nb, n)
    posm = posm.copy()
    posm[5, :3] = posm[9, :3]
    pos, mass = posm[:, :3], posm[:, 3]
    assert (vel[5, :3] != vel[9, :3]).any()
    ref = direct_jerk(pos, mass, vel, pos, vel, eps=eps, skip_self=True)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.jerk()
    check(f"coincident bodies N={n} eps={eps}", got, ref, TOL_ACC)
    for k, other in ((5, 9), (9, 5)):
        keep = (np.arange(n) != k) & (np.arange(n) != other)
        wa, wj = direct_jerk(pos[keep], mass[keep], vel[keep], pos[k:k + 1], vel[k:k + 1], eps=eps)
        assert rel(got[0][k:k + 1], wa)[0] < TOL_ACC                                 # no acceleration from the other, at any eps
        if eps == 0.0:
            assert rel(got[1][k:k + 1], wj)[0] < TOL_ACC                             # neither feels the other
        else:
            own = G * float(mass[other]) * (vel[other, :3].astype(np.float64) - vel[k, :3].astype(np.float64)) / eps ** 3
            d = got[1][k].astype(np.float64) - wj[0]
            assert np.linalg.norm(d - own) <= 1e-4 * np.linalg.norm(own)


# ---- 7, 8: the other precisions -------------------------------------------------------------------------------------------------------

def _plummer():
    g = np.load(os.path.join(GOLDEN, "plummer_n1024_seed1.npz"))
    return g["posm"].astype(np.float64), g["vel"].astype(np.float64)


@pytest.mark.parametrize("scene,eps", [("plummer1024", 0.0), ("box257", 0.0), ("box257", 0.05)])
def test_fp64_contexts(nb, scene, eps):
    if scene == "plummer1024":
        posm, vel = _plummer()
    else:
        posm, vel = (x.astype(np.float64) for x in bodies(nb, 257))
        posm[:, :3] += 1e-7 * posm[:, :3] ** 2                    # (positions that are not fp32 numbers)
    n = posm.shape[0]
    ref = direct_self(n, posm, vel, eps, np.longdouble)
    with nb.NBodyEngine(n, precision="f64", eps=eps) as e:
        e.set_state(posm, vel)
        got = e.jerk(np.float64)
        f32 = e.jerk()
        t, body = e.jerk_time()
        with pytest.raises(nb.NBodyError) as er:
            e.jerk_at(posm[:4, :3].astype(np.float32))
        assert er.value.code == nb._lib.ERR_UNSUPPORTED and "nbody_jerk_at" in str(er.value)
    assert got[0].dtype == np.float64
    check(f"fp64 context {scene} eps={eps}", got, ref, TOL_F64)
    assert f32[0].tobytes() == got[0].astype(np.float32).tobytes() and f32[1].tobytes() == got[1].astype(np.float32).tobytes()
    assert (t, body) == jerk_time_of(*got)


def test_kahan_contexts_give_the_plain_contexts_bits(nb):
    n, m = 2000, 65
    posm, vel = bodies(nb, n)
    pts, pv = probes_for(posm[:, :3], m), probe_velocities(m)
    out = []
    for prec in ("f32", "f32_kahan"):
        with nb.NBodyEngine(n, precision=prec) as e:
            e.set_state(posm, vel)
            out.append(tuple(x.tobytes() for x in e.jerk() + e.jerk(np.float64) + e.jerk_at(pts, pv)) + (e.jerk_time(),))
    assert out[0] == out[1]


# ---- 9, 10: theta > 0 and the live buffers ---------------------------------------------------------------------------------------------

def test_theta_1_is_the_same_pair_sum_and_touches_nothing(nb):
    n, m = 2000, 65
    posm, vel = bodies(nb, n)
    pts, pv = probes_for(posm[:, :3], m), probe_velocities(m)
    with nb.NBodyEngine(n) as e0, nb.NBodyEngine(n, theta=1.0) as e1:
        e0.set_state(posm, vel)
        e1.set_state(posm, vel)
        # before any frame: no tree exists, none is needed, none is built
        for f in (lambda e: e.jerk(), lambda e: e.jerk(np.float64), lambda e: e.jerk_at(pts, pv)):
            r0, r1 = f(e0), f(e1)
            assert r0[0].tobytes() == r1[0].tobytes() and r0[1].tobytes() == r1[1].tobytes()
        assert e0.jerk_time() == e1.jerk_time()
        e1.step(0.01, 2)
        stats = e1.bh_stats()
        before = (stats["nodes"], stats["levels"], stats["root_com"].tobytes(), e1.particles().tobytes(), e1.steps_done())
        got = e1.jerk()
        e1.jerk(np.float64), e1.jerk_at(pts, pv), e1.jerk_time()
        stats = e1.bh_stats()
        assert (stats["nodes"], stats["levels"], stats["root_com"].tobytes(), e1.particles().tobytes(), e1.steps_done()) == before
        p, v, _ = e1.state()
    check("jerk() at theta = 1 after two frames", got, direct_jerk(p[:, :3], p[:, 3], v, p[:, :3], v, skip_self=True), TOL_ACC)


# one context per stepping path: the one-launch block kernel (it swaps position buffers), NBODY_ALGO_TILED, NBODY_ALGO_SYMMETRIC — which
# accepts every size: 257, this file's smallest with more than one tile — and fp64
@pytest.mark.parametrize("n,kw", [(2000, {}), (2000, {"algorithm": 1}), (257, {"algorithm": 2}), (257, {"precision": "f64"})])
def test_the_live_buffers_after_stepping(nb, n, kw):
    posm, vel = bodies(nb, n)
    f64 = kw.get("precision") == "f64"
    dt = np.float64 if f64 else np.float32
    with nb.NBodyEngine(n, **kw) as e:
        e.set_state(posm.astype(dt), vel.astype(dt))
        e.step(0.01, 3)
        got = e.jerk(np.float64)
        again = e.jerk(np.float64)
        p, v, _ = e.state(dt)
        assert e.steps_done() == 3
    assert (p[:, :3] != posm[:, :3]).any()
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    ref = direct_jerk(p[:, :3], p[:, 3], v, p[:, :3], v, skip_self=True, dtype=np.longdouble if f64 else np.float64)
    check(f"jerk() after three steps N={n} {kw}", got, ref, TOL_F64 if f64 else TOL_ACC)


# ---- 11: jerk_time --------------------------------------------------------------------------------------------------------------------

def test_jerk_time_on_the_shipped_scene(nb):
    n = 2000
    posm, vel = bodies(nb, n)
    ref = direct_self(n, posm, vel)
    want_t, want_body = jerk_time_of(*ref)
    k = np.sort(k_of(*ref))
    assert want_body == 986 and want_t == pytest.approx(6.70305e-3, rel=1e-5)
    assert k[-2] < k[-1] * (1 - 8 * TOL_ACC)                      # the runner-up is not within rounding of it
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        t, body = e.jerk_time()
        assert e.jerk_time() == (t, body)
        assert (t, body) == jerk_time_of(*e.jerk(np.float64))      # bitwise, the same body: the formula on the context's own vectors
        only_t, only_body = ctypes.c_double(), ctypes.c_int32()
        assert e._L.nbody_jerk_time(e._h, ctypes.byref(only_t), None) == 0 and only_t.value == t
        assert e._L.nbody_jerk_time(e._h, None, ctypes.byref(only_body)) == 0 and only_body.value == body
    print(f"jerk_time N={n}: t_min {t:.6e} at body {body} (fp64 direct sum: {want_t:.6e} at {want_body})")
    # t = |a| / |j|, each norm within TOL_ACC of the reference's
    assert body == 986 and abs(t - want_t) <= 2 * TOL_ACC * want_t


# ---- 12: errors -----------------------------------------------------------------------------------------------------------------------

def _four_calls(e, pts):
    return (lambda: e.jerk_at(pts)), e.jerk, (lambda: e.jerk(np.float64)), e.jerk_time


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    """tests/cpp/fake_rccl.c, the suite's stand-in for the communication library (tests/test_multi_parts_gpu.py): a multi-device context
    over device 0 alone needs no real communicator to refuse a call, and creating one costs seconds."""
    so = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "fake_rccl.c"), "-o", so, "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return so


def test_errors(nb, fake_rccl, monkeypatch):
    monkeypatch.setenv("NBODY_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("NBODY_MULTI_SHARE_DEVICE", "1")
    n = 2000
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], 16)
    pv = probe_velocities(16)
    E = nb._lib
    for theta in (0.0, 1.0):
        with nb.NBodyEngine(n, theta=theta) as e:
            for call in _four_calls(e, pts):                       # no particles set
                with pytest.raises(nb.NBodyError) as er:
                    call()
                assert er.value.code == E.ERR_STATE
            e.set_state(posm, vel)
            a = np.zeros((16, 3), np.float32)
            j = np.zeros((16, 3), np.float32)
            P, V, A, J = pts.ctypes.data, pv.ctypes.data, a.ctypes.data, j.ctypes.data
            f = e._L.nbody_jerk_at
            assert f(e._h, None, 12, V, 12, 16, A, 12, J, 12) == E.ERR_INVALID
            assert f(e._h, P, 12, V, 12, -1, A, 12, J, 12) == E.ERR_INVALID
            assert f(e._h, P, 12, V, 12, 16, None, 12, None, 12) == E.ERR_INVALID
            assert f(e._h, P, 8, V, 12, 16, A, 12, J, 12) == E.ERR_INVALID
            assert f(e._h, P, 12, V, 8, 16, A, 12, J, 12) == E.ERR_INVALID
            assert f(e._h, P, 12, V, 12, 16, A, 11, J, 12) == E.ERR_INVALID
            assert f(e._h, P, 12, V, 12, 16, A, 12, J, 11) == E.ERR_INVALID
            assert not a.any() and not j.any()
            assert f(e._h, P, 12, None, 0, 16, A, 12, J, 12) == 0 and a.any() and j.any()     # (a NULL velocity's stride is not looked at)
            ba = np.zeros((n, 3), np.float32)
            g = e._L.nbody_get_jerk
            assert g(e._h, None, 12, None, 12) == E.ERR_INVALID
            assert g(e._h, ba.ctypes.data, 11, None, 0) == E.ERR_INVALID
            assert g(e._h, None, 0, ba.ctypes.data, 11) == E.ERR_INVALID
            bd = np.zeros((n, 3), np.float64)
            g = e._L.nbody_get_jerk_f64
            assert g(e._h, None, 24, None, 24) == E.ERR_INVALID
            assert g(e._h, bd.ctypes.data, 23, None, 0) == E.ERR_INVALID
            assert g(e._h, None, 0, bd.ctypes.data, 12) == E.ERR_INVALID
            assert not ba.any() and not bd.any()
            assert e._L.nbody_jerk_time(e._h, None, None) == E.ERR_INVALID
    for kw in ({"i_begin": 0, "i_count": 1000}, {"devices": [0]}):
        with nb.NBodyEngine(n, **kw) as e:
            e.set_state(posm, vel)
            for call in _four_calls(e, pts):
                with pytest.raises(nb.NBodyError) as er:
                    call()
                assert er.value.code == E.ERR_UNSUPPORTED, kw
