"""The tidal tensor at theta = 0: nbody_tidal_at (at caller-given points), nbody_get_tidal (at the bodies, self excluded by index) and
nbody_tidal_time (the smallest ||T_i||_F^(-1/2) and its body), against the numpy fp64 direct sum of tests/bh_tidal_ref.py at the
project's all-pairs tolerance; the argument and context errors of all three at any theta.

The error of a point is err = ||T_got - T_ref||_F / ||T_ref||_F, the off-diagonal entries counted twice.  The bound is TOL_ACC (2e-5)
throughout.  Next to every case stands what the kernels' arithmetic alone gives on that scene — emulate_tidal_f32 of
tests/bh_tidal_ref.py, fp32 per pair and per chunk with a correctly rounded root, fp64 fold, run on the CPU — which is to stay below a
quarter of the bound, the rest being v_rsq_f32's ulp.  The shipped scene's own-body figures (5.4e-6) sit at that quarter; they are the
issue's scene and stay.

Partial rows at N = 20000 (probe_geometry: chunks of ceil(ceil(20000 / 128) / 256) * 256 = 256 bodies, 79 of them; a tensor row is two
float4 per point and chunk): probe_slab_points(20000, 2) = floor(256 MiB / (79 * 32 B)) in whole 1024s = 105472 points per slab; a
workgroup takes 1024 points instead of 512 from ceil(M / 1024) * 79 >= 1024 on, M >= 12289.  M = 106072 is 600 points into the second
slab: the first slab runs the 1024-point shape, the second the 512-point one, and every sub-range asked for alone the 512-point one."""
import ctypes

import numpy as np
import pytest

from bh_tidal_ref import G, direct_tidal, frob
from probe_scenes import N_PROBES, TOL_ACC, bodies, probes_for

pytestmark = pytest.mark.gpu


def probe_geometry(n_total):
    chunk = max(1, ((n_total + 127) // 128 + 255) // 256) * 256
    return (n_total + chunk - 1) // chunk, chunk


def slab_points(n_total, width):
    return max(1024, (256 << 20) // (probe_geometry(n_total)[0] * 16 * width) // 1024 * 1024)


N_MANY = 20000
SLAB = slab_points(N_MANY, 2)
WG2 = 1024 * ((1024 + probe_geometry(N_MANY)[0] - 1) // probe_geometry(N_MANY)[0] - 1) + 1   # the smallest M of the 1024-point shape
M_MANY = SLAB + 600
assert (SLAB, WG2, M_MANY) == (105472, 12289, 106072)

_direct = {}


def direct_ref(n, pos, mass, pts, eps=0.0, skip_self=False):
    key = (n, pts.shape[0], eps, skip_self, pos.tobytes()[:64], pts.tobytes()[:64])
    if key not in _direct:
        ref = direct_tidal(pos, mass, pts, eps=eps, skip_self=skip_self)
        ref.setflags(write=False)
        _direct[key] = ref
    return _direct[key]


def err(got, ref):
    """||got - ref||_F / ||ref||_F per point; a point whose reference is exactly zero must be exactly zero."""
    got = np.asarray(got, np.float64)
    f = frob(ref)
    zero = f == 0.0
    assert not got[zero].any()
    return np.where(zero, 0.0, frob(got - ref) / np.where(zero, 1.0, f))


def scene(nb, n, seed=None):
    posm, vel = bodies(nb, n) if seed is None else nb.ic_reference_box(n, 1000.0, seed=seed)
    return posm, vel, posm[:, :3], posm[:, 3]


# ---- tidal_at -----------------------------------------------------------------------------------------------------------------------

# (n, m, eps, seed of ic_reference_box or None for probe_scenes.bodies, the emulation's max err on the CPU)
# N = 257 against 5000 probes: a single fp32 chain of 256 bodies, and among 5000 probes some where the tensor all but cancels;
# bodies(257) (seed 257) emulates to 5.8e-6, over a quarter of the bound, so the scene is seed 12's.
AT_CASES = [(2000, 777, 0.0, None, 2.8e-6), (2000, 1, 0.0, None, 1.3e-7), (2000, 64, 0.0, None, 1.8e-6), (2000, 65, 0.0, None, 1.8e-6),
            (257, 5000, 0.0, 12, 4.8e-6), (1, 64, 0.0, None, 4.9e-7), (20000, 100, 0.0, None, 1.4e-6), (2000, 777, 0.05, None, 4.0e-6)]


@pytest.mark.parametrize("n,m,eps,seed,emulated", AT_CASES)
def test_direct_sum_at_every_probe(nb, n, m, eps, seed, emulated):
    posm, vel, pos, mass = scene(nb, n, seed)
    pts = probes_for(pos, m)
    ref = direct_ref(n, pos, mass, pts, eps=eps)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.tidal_at(pts)
    assert got.shape == (m, 6) and got.dtype == np.float32 and np.isfinite(got).all() and np.isfinite(ref).all()
    er = err(got, ref)
    print(f"tidal_at theta=0 N={n} M={m} eps={eps}: max err {er.max():.3e} (emulated {emulated:.1e})")
    assert emulated <= TOL_ACC / 4
    assert er.max() < TOL_ACC, (n, m, int(er.argmax()), er.max())
    if eps == 0.0:
        f = frob(got)
        tr = np.abs(got[:, :3].astype(np.float64).sum(1)) / np.where(f > 0.0, f, 1.0)
        print(f"tidal_at theta=0 N={n} M={m}: max |trace| / ||T||_F {tr.max():.3e}")
        assert tr.max() <= TOL_ACC, (n, m, int(tr.argmax()), tr.max())
    if m >= 60 and n >= 110 and eps > 0.0:
        # probe 0 sits ON body 0 (the scene's heaviest): it feels that body's -G m / eps^3 on the diagonal and nothing of it off
        # the diagonal — got and `without` are each within TOL_ACC of their own direct sums, whose scale is that term's
        without = direct_tidal(pos[1:], mass[1:], pts[:1], eps=eps)[0]
        d = got[0].astype(np.float64) - without
        own = G * float(mass[0]) / eps ** 3
        assert d[:3] == pytest.approx(-own, rel=1e-4)
        assert np.abs(d[3:]).max() <= TOL_ACC * frob(got[:1])[0]


def test_a_probe_next_to_a_heavy_body_does_not_overflow(nb):
    # body 0 of the shipped scene: mass 5000 at the origin.  2^-22 away G m / s^3 = 3.7e27 is an fp32 number, G m / s^5 is not.
    n = 2000
    posm, vel, pos, mass = scene(nb, n)
    assert not pos[0].any() and mass[0] == 5000.0
    pts = np.array([[2.0 ** -22, 0.0, 0.0], [0.0, -2.0 ** -22, 0.0]], np.float32)
    ref = direct_tidal(pos, mass, pts)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        got = e.tidal_at(pts)
    assert np.isfinite(got).all() and abs(got[0, 0]) > 1e27
    assert err(got, ref).max() < TOL_ACC


@pytest.mark.parametrize("n,eps,emulated", [(2000, 0.0, 5.4e-6), (2000, 0.05, 5.4e-6), (257, 0.0, 4.7e-6), (1, 0.0, 0.0)])
def test_tidal_is_the_direct_sum_without_the_body_itself(nb, n, eps, emulated):
    posm, vel, pos, mass = scene(nb, n)
    ref = direct_ref(n, pos, mass, pos, eps=eps, skip_self=True)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.tidal()
        at = e.tidal_at(pos)
    assert got.shape == (n, 6) and got.dtype == np.float32 and np.isfinite(got).all()
    er = err(got, ref)
    print(f"tidal theta=0 N={n} eps={eps}: max err {er.max():.3e} (emulated {emulated:.1e})")
    assert er.max() < TOL_ACC, (n, int(er.argmax()), er.max())
    if n == 1:
        return
    if eps > 0.0:
        # the two modes differ where they must: a point ON body i feels body i's -G m / eps^3 on the diagonal, the body itself does not
        d = at.astype(np.float64) - got.astype(np.float64)
        own = G * mass.astype(np.float64) / eps ** 3
        assert np.abs(d[:, :3] + own[:, None]).max() <= 2 * TOL_ACC * frob(at).max()
        assert np.abs(d[:, 3:]).max() <= 2 * TOL_ACC * frob(at).max()
    else:
        assert at.tobytes() == got.tobytes()                      # eps == 0: d == 0 drops the same pair the index drops


def test_two_coincident_bodies_skip_each_other(nb):
    n = 2000
    posm, vel, _, _ = scene(nb, n)
    posm = posm.copy()
    posm[5, :3] = posm[9, :3]
    pos, mass = posm[:, :3], posm[:, 3]
    ref = direct_tidal(pos, mass, pos, skip_self=True)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        got = e.tidal()
        t, body = e.tidal_time()
    assert np.isfinite(got).all() and err(got, ref).max() < TOL_ACC              # (emulated: 5.4e-6)
    # the time scale is the finite one the other bodies produce
    want = frob(ref) ** -0.5
    assert np.isfinite(t) and t > 0.0 and body == int(want.argmin()) and t == pytest.approx(want.min(), rel=TOL_ACC)


def test_every_zero_mode_gives_the_default_contexts_bytes(nb):
    n, m = 2000, N_PROBES
    posm, vel, pos, _ = scene(nb, n)
    pts = probes_for(pos, m)
    out = []
    for zm in (nb._lib.ZERO_EXACT, nb._lib.ZERO_FLOOR, nb._lib.ZERO_SELECT):
        with nb.NBodyEngine(n, zero_mode=zm) as e:
            e.set_state(posm, vel)
            out.append((e.tidal_at(pts).tobytes(), e.tidal().tobytes(), e.tidal_time()))
    assert out[1] == out[0] and out[2] == out[0]


def test_bit_level_properties(nb):
    n, m = 2000, N_PROBES
    posm, vel, pos, _ = scene(nb, n)
    pts = probes_for(pos, m)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        e.step(0.01, 2)
        before = (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done())
        a = e.tidal_at(pts)
        assert e.tidal_at(pts).tobytes() == a.tobytes()                            # two calls
        h = m // 2
        assert np.concatenate([e.tidal_at(pts[:h]), e.tidal_at(pts[h:])]).tobytes() == a.tobytes()   # a point does not see the others
        p4 = np.zeros((m, 4), np.float32); p4[:, :3] = pts; p4[:, 3] = 123.0
        v16 = p4[:, :3]
        assert v16.strides == (16, 4) and e.tidal_at(v16).tobytes() == a.tobytes()
        rec = np.zeros(m, nb.PARTICLE_DTYPE)
        rec["Mass"] = 7.0; rec["Velocity"] = 9.0; rec["Position"] = pts
        v40 = rec["Position"]
        assert v40.strides == (40, 4) and e.tidal_at(v40).tobytes() == a.tobytes()
        # ... and on the output side, through the C entry point itself: stride 24 and a larger one
        f = e._L.nbody_tidal_at
        out24 = np.full((m, 6), 5.0, np.float32)
        assert f(e._h, pts.ctypes.data, 12, m, out24.ctypes.data, 24) == 0 and out24.tobytes() == a.tobytes()
        out40 = np.full((m, 10), 5.0, np.float32)
        assert f(e._h, rec["Position"].ctypes.data, 40, m, out40.ctypes.data, 40) == 0
        assert np.ascontiguousarray(out40[:, :6]).tobytes() == a.tobytes() and (out40[:, 6:] == 5.0).all()
        out24[:] = 5.0
        assert f(e._h, pts.ctypes.data, 12, 0, out24.ctypes.data, 24) == 0 and (out24 == 5.0).all()     # n == 0: a no-op
        t = e.tidal()
        assert e.tidal().tobytes() == t.tobytes()
        big = np.full((n, 8), 5.0, np.float32)
        assert e._L.nbody_get_tidal(e._h, big.ctypes.data, 32) == 0
        assert np.ascontiguousarray(big[:, :6]).tobytes() == t.tobytes() and (big[:, 6:] == 5.0).all()
        tt = e.tidal_time()
        assert e.tidal_time() == tt
        assert (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done()) == before


def test_many_points_across_the_workgroup_shapes_and_the_slab_boundary(nb):
    n, m = N_MANY, M_MANY
    posm, vel, pos, mass = scene(nb, n)
    pts = probes_for(pos, m)
    pts[SLAB - 25:SLAB - 15] = pos[200:210]                       # on bodies and beside bodies on either side of the slab boundary
    pts[SLAB + 15:SLAB + 25] = pos[210:220] + np.float32(1e-3)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        got = e.tidal_at(pts)
        assert got.shape == (m, 6) and np.isfinite(got).all()
        ranges = [(0, 777), (1024 - 3, 1024 + 300), (WG2 - 101, WG2 + 99), (0, WG2 - 1), (0, WG2), (SLAB - 300, SLAB + 300), (SLAB, SLAB + 1),
                  (SLAB - 1, SLAB), (SLAB, m), (m - 1, m)]
        for a, b in ranges:
            assert e.tidal_at(pts[a:b]).tobytes() == got[a:b].tobytes(), (a, b)
    sample = np.unique(np.concatenate([np.arange(0, 64), np.arange(WG2 - 20, WG2 + 20), np.arange(SLAB - 40, SLAB + 40), np.arange(m - 64, m),
                                       np.random.default_rng(9).integers(0, m, 250)]))
    assert sample.size <= 500
    er = err(got[sample], direct_tidal(pos, mass, pts[sample]))
    print(f"tidal_at theta=0 N={n} M={m}: max err on {sample.size} sampled points {er.max():.3e} (emulated 4.7e-6)")
    assert er.max() < TOL_ACC, (int(sample[er.argmax()]), er.max())


# ---- tidal_time ---------------------------------------------------------------------------------------------------------------------

def test_tidal_time_on_the_shipped_scene(nb):
    # body 1671 with t = 1.3187e-3; the runner-up (body 740) is at 2.31e-3: the index is not at the mercy of rounding
    n = 2000
    posm, vel, pos, mass = scene(nb, n)
    want = frob(direct_ref(n, pos, mass, pos, skip_self=True)) ** -0.5
    assert int(want.argmin()) == 1671 and want.min() == pytest.approx(1.3187e-3, rel=1e-4)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        t, body = e.tidal_time()
        assert e.tidal_time() == (t, body)                        # identical bits every run
        only_t, only_body = ctypes.c_double(), ctypes.c_int32()
        assert e._L.nbody_tidal_time(e._h, ctypes.byref(only_t), None) == 0 and only_t.value == t
        assert e._L.nbody_tidal_time(e._h, None, ctypes.byref(only_body)) == 0 and only_body.value == body
        assert e._L.nbody_tidal_time(e._h, None, None) == nb._lib.ERR_INVALID
        # the same number from the rounded tensors, to their rounding
        assert t == pytest.approx(float((frob(e.tidal()) ** -0.5).min()), rel=1e-6)
    print(f"tidal_time theta=0 N={n}: t_min {t:.6e} at body {body} (fp64 direct sum: {want.min():.6e})")
    assert body == 1671 and abs(t - want.min()) <= TOL_ACC * want.min()


def test_tidal_time_of_a_single_body_is_infinite(nb):
    posm, vel, _, _ = scene(nb, 1)
    for theta in (0.0, 1.0):
        with nb.NBodyEngine(1, theta=theta) as e:
            e.set_state(posm, vel)
            assert e.tidal_time() == (float("inf"), 0)
            assert not e.tidal().any()


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def _three_calls(e, pts):
    return (lambda: e.tidal_at(pts)), e.tidal, e.tidal_time


def test_errors(nb):
    n = 2000
    posm, vel, pos, _ = scene(nb, n)
    pts = probes_for(pos, 16)
    E = nb._lib
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError) as er:                  # no tree yet
            e.tidal_at(pts)
        assert er.value.code == E.ERR_STATE and "nbody_tidal_at" in str(er.value) and "nbody_compute_forces" in str(er.value)
        e.compute_forces()
        e.tidal_at(pts)
        e.set_theta(0.5)
        with pytest.raises(nb.NBodyError) as er:                  # the tree is another angle's
            e.tidal_at(pts)
        assert er.value.code == E.ERR_STATE
        e.tidal()                                                 # builds its own tree ...
        e.tidal_at(pts)                                           # ... which a query may walk
        e.set_theta(1.0)
        e.tidal_time()                                            # ... and so does the time scale
        e.tidal_at(pts)
    for theta in (0.0, 1.0):
        with nb.NBodyEngine(n, theta=theta) as e:
            e.set_state(posm, vel)
            e.compute_forces()
            out = np.zeros((16, 6), np.float32)
            f = e._L.nbody_tidal_at
            assert f(e._h, pts.ctypes.data, 8, 16, out.ctypes.data, 24) == E.ERR_INVALID
            assert f(e._h, pts.ctypes.data, 12, 16, out.ctypes.data, 23) == E.ERR_INVALID
            assert f(e._h, pts.ctypes.data, 12, 16, out.ctypes.data, 12) == E.ERR_INVALID
            assert f(e._h, None, 12, 16, out.ctypes.data, 24) == E.ERR_INVALID
            assert f(e._h, pts.ctypes.data, 12, 16, None, 24) == E.ERR_INVALID
            assert f(e._h, pts.ctypes.data, 12, -1, out.ctypes.data, 24) == E.ERR_INVALID
            assert not out.any()
            big = np.zeros((n, 6), np.float32)
            assert e._L.nbody_get_tidal(e._h, None, 24) == E.ERR_INVALID
            assert e._L.nbody_get_tidal(e._h, big.ctypes.data, 23) == E.ERR_INVALID
            assert e._L.nbody_tidal_time(e._h, None, None) == E.ERR_INVALID
    for kw in ({"precision": "f64"}, {"precision": "f32_kahan"}, {"i_begin": 0, "i_count": 1000}, {"devices": [0]}):
        with nb.NBodyEngine(n, **kw) as e:
            e.set_state(posm, vel)
            for call in _three_calls(e, pts):
                with pytest.raises(nb.NBodyError) as er:
                    call()
                assert er.value.code == E.ERR_UNSUPPORTED, kw


def test_a_last_tree_deeper_than_42_levels_answers_no_tidal_tensor(nb):
    # tests/test_bh_deep_gpu.py's construction: a runaway body holds Size at 1e9, and two bodies 1e-4 apart split below level 42
    n = 2000
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=1)
    posm[0, :3] = (1.0e9, -2.0e8, 3.0e8)
    posm[0, 3] = np.float32(1e-6)
    posm[1, :3] = (500.25, 300.5, -200.75)
    posm[2, :3] = posm[1, :3] + np.float32(1e-4)
    vel[:7, :3] = 0.0
    pts = probes_for(posm[:, :3], 16)
    E = nb._lib
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_bh_max_depth(200)
        e.set_state(posm, vel)
        e.compute_forces()
        assert e.bh_stats()["levels"] > 42
        for call in _three_calls(e, pts):
            with pytest.raises(nb.NBodyError) as er:
                call()
            assert er.value.code == E.ERR_UNSUPPORTED and "deeper than 42 levels" in str(er.value) and "tidal tensor" in str(er.value)
