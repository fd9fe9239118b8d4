"""The fp64 neighbour census — nbody_get_neighbours_f64, nbody_neighbours_at_f64, nbody_get_density_f64, nbody_density_centre_f64 — on
the device.

The yardstick is tests/neighbours_f64_ref.py in long double on the scenes of pot_tidal_f64_ref.plummer_scene.  A sorted list can be held
to a reference only where its entries are far enough apart, so every test that compares indices first asserts the GAP CONDITION on ALL
of its rows (no row is ever left out): the smallest relative distance between consecutive entries of the nine nearest exceeds 1e-9,
1000 x the bound of the values (tests/test_neighbours_f64_ref.py shows the scenes three orders above it, on the CPU).  d2 is held within
TOL_F64 relative; the density within TOL_F64 of long double's; the core's sums within TOL_F64 of the long-double sums relative to the
sum of |terms|.  Everything else here is byte for byte.

Measured on an MI355X, the largest over all rows of all accuracy tests here: d2 3.8e-16, rho 7.1e-16, the core's sums 1.3e-16, its
centre 2.4e-17 of sum w |x| / sum w, its radius 9.4e-16."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import census_f64_ref as C
import neighbours_f64_ref as N
from jerk_ref import probe_geometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1e-3
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
LD = np.longdouble
INF = np.inf
K8 = N.K_MAX


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
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
        f"{what}: {int((a != b).reshape(a.shape[0], -1).any(axis=-1).sum())} of {a.shape[0]} rows differ"


def held(what, got, ref, k, rows=None):
    """(index, d2) of a k-neighbour call, at `rows` of it (None: all), against a long-double (index, d2, gap) of K8 columns: the gap
    condition on every row first, then every index, then d2.  Returns the largest error."""
    N.gaps_hold(ref)
    idx, d2 = got if rows is None else (got[0][rows], got[1][rows])
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and idx.shape == d2.shape == (ref[0].shape[0], k)
    assert (idx == ref[0][:, :k]).all(), f"{what}: {int((idx != ref[0][:, :k]).any(1).sum())} rows differ in an index"
    err = float(np.abs((d2.astype(LD) - ref[1][:, :k]) / ref[1][:, :k]).max())
    print(f"{what}: d2 {err:.3e} of the long-double lists")
    assert err < TOL_F64
    return err


# ---- 1: against long double ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", N.CASES)
@pytest.mark.parametrize("k", [6, 8])
def test_bodies_and_points_against_long_double(nb, n, m, k):
    posm, vel, tpos, _ = C.scene(nb, n, m)
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        f = [passes(nb, e)]
        bodies = e.neighbours_f64(k); f.append(passes(nb, e))
        points = e.neighbours_at_f64(tpos, k); f.append(passes(nb, e))
        assert np.diff(f).tolist() == [1, 1]                       # one pass under NBODY_KERNEL_FORCES each
        held(f"N = {n}, k = {k}, bodies", bodies, N.reference(nb, "bodies", n, m), k)
        held(f"N = {n}, M = {m}, k = {k}, points", points, N.reference(nb, "points", n, m), k)
        p, v, _ = e.state(np.float64)
        eq(p, posm, "positions"); eq(v, vel, "velocities")


# ---- 2: prefixes, every width, and the nearest of the pair census --------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(1000, 25), (257, 300)])
def test_every_k_is_a_prefix_of_eight_and_one_is_the_nearest(nb, n, m):
    posm, vel, tpos, _ = C.scene(nb, n, m)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        bi, bd = e.neighbours_f64(K8)
        pi, pd = e.neighbours_at_f64(tpos, K8)
        for k in range(1, K8 + 1):                                 # k <= 4 runs the list of four, 5 and 6 the list of six, 7 and 8 the list of eight
            gi, gd = e.neighbours_f64(k)
            eq(gi, bi[:, :k], f"bodies, index, k = {k}"); eq(gd, bd[:, :k], f"bodies, d2, k = {k}")
            gi, gd = e.neighbours_at_f64(tpos, k)
            eq(gi, pi[:, :k], f"points, index, k = {k}"); eq(gd, pd[:, :k], f"points, d2, k = {k}")
        ni, nd = e.nearest_f64()
        eq(e.neighbours_f64(1)[0][:, 0], ni, "k = 1 against nearest_f64, index"); eq(e.neighbours_f64(1)[1][:, 0], nd, "k = 1 against nearest_f64, d2")
        ni, nd = e.nearest_at_f64(tpos)
        eq(e.neighbours_at_f64(tpos, 1)[0][:, 0], ni, "k = 1 against nearest_at_f64, index")
        eq(e.neighbours_at_f64(tpos, 1)[1][:, 0], nd, "k = 1 against nearest_at_f64, d2")


# ---- 3: 512-body chunks ----------------------------------------------------------------------------------------------------------------

def test_bodies_at_512_body_chunks(nb):
    """N = 32769: 65 chunks of 512 bodies, the last one holds one body and 255 pads.  All bodies are computed; 134 sampled ones — the
    first and the last 64, and those round the tile and chunk boundaries — are held to long double."""
    n = N.N_CHUNKS
    assert probe_geometry(n) == (65, 512)
    posm, vel, _, _ = C.scene(nb, n)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        idx, d2 = e.neighbours_f64(K8)
        held(f"N = {n}, 134 bodies", (idx, d2), N.reference(nb, "chunks"), K8, rows=N.ROWS_CHUNKS)
        assert (idx >= 0).all() and (idx < n).all() and (idx != np.arange(n)[:, None]).all()
        s = np.sort(idx, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all()                       # distinct within a row
        assert (d2[:, 1:] >= d2[:, :-1]).all() and np.isfinite(d2).all()
        ni, nd = e.nearest_f64()
        eq(e.neighbours_f64(1)[0][:, 0], ni, "k = 1 against nearest_f64 over 65 chunks"); eq(d2[:, 0], nd, "the first d2 against nearest_f64")


# ---- 4: the padding of a chunk's last tile is nobody ---------------------------------------------------------------------------------

def test_the_padding_is_not_a_body(nb):
    """N = 257: the second chunk holds one body and 255 pads on the origin.  Points at and next to the origin would list pads at
    d2 = 0 / 1e-6 if they were admitted by anything but their index."""
    n = 257
    posm, vel, _, _ = C.scene(nb, n)
    pts = np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [0.0, -1e-3, 0.0], [1e-3, 1e-3, 1e-3], [0.0, 0.0, 1e-6]])
    ref = N.neighbours(posm, pts, dtype=LD)
    true_d2 = ((posm[None, :, :3] - pts[:, None, :]) ** 2).sum(-1).min(1)
    assert true_d2.min() > 1e-4                                    # (no body is anywhere near as close as a pad would be)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        idx, d2 = e.neighbours_at_f64(pts, K8)
        assert (idx >= 0).all() and (idx < n).all()
        assert (d2 >= (true_d2 * (1 - 1e-12))[:, None]).all()
        held(f"N = {n}, points round the origin", (idx, d2), ref, K8)
        moved = posm.copy(); moved[256, :3] = 0.0                   # a body put onto the origin is found there, as a body
        e.set_state(moved, vel)
        idx, d2 = e.neighbours_at_f64(pts, K8)
        assert idx[:, 0].tolist() == [256] * 5 and d2[0, 0] == 0.0 and d2[1, 0] == 1e-3 * 1e-3
        assert (idx[:, 1:] != 256).all() and (idx >= 0).all() and (idx < n).all()


# ---- 5: exact ties and coincident bodies, byte for byte ------------------------------------------------------------------------------

def test_exact_ties_and_coincident_bodies_byte_for_byte(nb):
    """300 equal masses on a small-integer lattice, shuffled, six of them on top of others: every operation in d2 is exact, so index
    and d2 are numpy's stable (d2, index) order in every byte — across tiles and across the two chunks — and coincident bodies come
    first."""
    posm, vel = C.lattice_scene()
    n = posm.shape[0]
    ref = N.neighbours(posm)
    pts = posm[::7, :3] + [0.5, 0.0, 0.0]                           # half-way between sites: ties again, exact again
    pref = N.neighbours(posm, pts)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        for k in (3, 5, K8):
            idx, d2 = e.neighbours_f64(k)
            eq(idx, ref[0][:, :k], f"index, k = {k}"); eq(d2, ref[1][:, :k], f"d2, k = {k}")
            idx, d2 = e.neighbours_at_f64(pts, k)
            eq(idx, pref[0][:, :k], f"index at points, k = {k}"); eq(d2, pref[1][:, :k], f"d2 at points, k = {k}")
        idx, d2 = e.neighbours_f64(K8)
        twins = d2[:, 0] == 0
        assert twins.sum() == 12 and (idx[twins, 0] != np.arange(n)[twins]).all() and (d2[twins, 1] > 0).all()
        # rows whose tied entries lie in both chunks of 256: the lower chunk's come first
        tie = d2[:, 1:] == d2[:, :-1]
        across = tie & (idx[:, :-1] < 256) & (idx[:, 1:] >= 256)
        assert across.sum() > 10 and (idx[:, 1:][tie] > idx[:, :-1][tie]).all()
        onto = e.neighbours_at_f64(posm[:, :3], 2)                  # a body asked about as a point: itself — or the lower of two coincident ones
        assert (onto[1][:, 0] == 0).all() and (onto[0][:, 0] <= np.arange(n)).all()


# ---- 6: small N ------------------------------------------------------------------------------------------------------------------------

def test_small_systems(nb):
    with f64(nb, 1) as e:
        e.set_state(np.array([[1.5, -2.25, 3.0, 7.0]]), np.zeros((1, 4)))
        for k in (1, 4, K8):
            idx, d2 = e.neighbours_f64(k)
            assert idx.shape == (1, k) and (idx == -1).all() and (d2 == INF).all()
        rho, rk2 = e.density_f64(2)
        assert rho.tolist() == [0.0] and rk2.tolist() == [INF]
        idx, d2 = e.neighbours_at_f64(np.array([[1.5, -2.25, 4.0]]), 3)
        assert idx.tolist() == [[0, -1, -1]] and d2.tolist() == [[1.0, INF, INF]]
    posm = np.array([[1.5, -2.25, 3.0, 7.0], [-0.5, 1.0, 4.25, 11.0]])
    with f64(nb, 2) as e:
        e.set_state(posm, np.zeros((2, 4)))
        idx, d2 = e.neighbours_f64(3)
        assert idx.tolist() == [[1, -1, -1], [0, -1, -1]] and d2[0, 0] == d2[1, 0] == 4.0 + 10.5625 + 1.5625 and (d2[:, 1:] == INF).all()
        c = e.core_f64(2)                                          # N <= k: every density is 0, nobody is used
        assert c.used == 0 and c.densest == -1 and c.rho_max == 0.0 and np.isnan(c.centre).all() and np.isnan(c.core_radius)
        assert c.rho_sum == 0.0 and c.rho2_sum == 0.0 and c.core_mass == 0.0 and c.core_count == 0 and c.k == 2
    rng = np.random.default_rng(6)
    five = np.concatenate([rng.normal(0, 1, (5, 3)), np.ones((5, 1))], 1)
    with f64(nb, 5) as e:
        e.set_state(five, np.zeros((5, 4)))
        idx, d2 = e.neighbours_f64(K8)
        ref = N.neighbours(five, dtype=LD)
        assert (idx == ref[0]).all() and (idx[:, :4] >= 0).all() and (idx[:, 4:] == -1).all() and (d2[:, 4:] == INF).all()
        assert np.isfinite(d2[:, :4]).all()
    for k in (2, 6, K8):                                           # N = k: the k-th neighbour is missing; N = k + 1: it is there
        for n in (k, k + 1):
            p = np.concatenate([rng.normal(0, 1, (n, 3)), rng.uniform(1, 2, (n, 1))], 1)
            with f64(nb, n) as e:
                e.set_state(p, np.zeros((n, 4)))
                rho, rk2 = e.density_f64(k)
                if n == k:
                    assert (rho == 0).all() and (rk2 == INF).all()
                else:
                    assert (rho > 0).all() and np.isfinite(rho).all() and np.isfinite(rk2).all()


def test_a_body_whose_position_is_nan(nb):
    n, bad_i = 257, 100
    posm, vel, tpos, _ = C.scene(nb, n, 300)
    bad = posm.copy(); bad[bad_i, 0] = np.nan
    rest = np.arange(n) != bad_i
    with f64(nb, n) as e, f64(nb, n - 1) as without:
        e.set_state(bad, vel); without.set_state(posm[rest], vel[rest])
        idx, d2 = e.neighbours_f64(K8)
        assert (idx[bad_i] == -1).all() and (d2[bad_i] == INF).all()       # its own row is empty
        assert (idx != bad_i).all()                                        # and it is in nobody's list
        wi, wd = without.neighbours_f64(K8)                                # all other rows are as without it: its chunk-mates move up by one
        up = lambda a: np.where(a >= bad_i, a + 1, a).astype(np.int32)
        eq(idx[rest], up(wi), "index"); eq(d2[rest], wd, "d2")
        pi, pd = e.neighbours_at_f64(tpos, K8)
        qi, qd = without.neighbours_at_f64(tpos, K8)
        eq(pi, up(qi), "index at points"); eq(pd, qd, "d2 at points")
        pi, pd = e.neighbours_at_f64(np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]]), 3)
        assert (pi == -1).all() and (pd == INF).all()
        rho, rk2 = e.density_f64(6)
        assert rho[bad_i] == 0.0 and rk2[bad_i] == INF and (rho[rest] > 0).all()


# ---- 7: points beyond one slab of the staging area -----------------------------------------------------------------------------------

def test_points_beyond_one_slab_of_the_staging_area(nb):
    """N = 33000: 65 chunks, so a slab of the rows of eight (eight float4 per point and chunk) is 31744 points.  1000 more: the rows on
    either side of the boundary equal the same points asked for alone, and 32 sampled points are held to long double."""
    n = N.N_SLAB
    posm, vel, _, _ = C.scene(nb, n)
    pts, sampled = N.slab_points(nb)
    slab = C.probe_slab_points(n, K8)
    assert slab == 31744 and pts.shape[0] == slab + 1000
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        got = e.neighbours_at_f64(pts, K8)
        held(f"N = {n}, 32 of {pts.shape[0]} points", got, N.reference(nb, "slab"), K8, rows=sampled)
        lo, hi = slab - 8, slab + 8
        for a, b in zip(e.neighbours_at_f64(pts[lo:hi], K8), got):
            eq(a, b[lo:hi], "the 16 points astride the slab boundary")
        for a, b in zip(e.neighbours_at_f64(pts[-300:], K8), got):
            eq(a, b[-300:], "the last 300 points")


# ---- 8: a row depends on the row and the bodies alone --------------------------------------------------------------------------------

def test_rows_are_independent_of_each_other(nb):
    n, m = 4097, 3000
    posm, vel, _, _ = C.scene(nb, n, 64)
    rng = np.random.default_rng(5)
    pts = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        for k in (3, 6, K8):
            big = e.neighbours_at_f64(pts, k)
            # 3000 and 1500 points go two rows a lane, 300 and 1 go one
            for lo, hi in ((100, 400), (500, 2000), (2999, 3000)):
                for a, b in zip(e.neighbours_at_f64(pts[lo:hi], k), big):
                    eq(a, b[lo:hi], f"points {lo} .. {hi} alone, k = {k}")
            bi, bd = e.neighbours_f64(k)
            oi, od = e.neighbours_at_f64(posm[:, :3], k)            # a body as a point: itself at d2 = 0, then its own list
            eq(oi[:, 0], np.arange(n, dtype=np.int32), "a body as a point: itself"); assert not od[:, 0].any()
            eq(oi[:, 1:], bi[:, :k - 1], "a body as a point: its neighbours behind it"); eq(od[:, 1:], bd[:, :k - 1], "and their d2")


# ---- 9: density, density centre, core radius -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(1000, 25), (257, 300)])
@pytest.mark.parametrize("k", [2, 6, 8])
def test_the_density_is_the_formula_on_the_devices_own_lists(nb, n, m, k):
    posm, vel, _, _ = C.scene(nb, n, m)
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        idx, d2 = e.neighbours_f64(k)
        f0 = passes(nb, e)
        rho, rk2 = e.density_f64(k)
        assert passes(nb, e) - f0 == 1
        want, wr2 = N.density(idx, d2, posm[:, 3], k)               # float64: operation by operation the device's
        eq(rho, want, "rho"); eq(rk2, np.ascontiguousarray(wr2), "rk2")
        ref = N.reference(nb, "bodies", n, m)
        ld, _ = N.density(ref[0], ref[1], posm[:, 3], k, LD)
        err = float(np.abs((rho.astype(LD) - ld) / ld).max())
        print(f"N = {n}, k = {k}: rho {err:.3e} of long double")
        assert err < TOL_F64


def core_held(what, c, rho, posm):
    """a CoreResult against the long-double sums over the device's own densities: each sum within TOL_F64 of its sum of |terms|"""
    r = N.core(rho, posm)
    assert (c.used, c.densest, c.rho_max) == (r["used"], r["densest"], r["rho_max"])
    e0 = float(abs(LD(c.rho_sum) - r["rho_sum"]) / r["rho_sum"])
    e1 = float(abs(LD(c.rho2_sum) - r["rho2_sum"]) / r["rho2_sum"])
    # centre = S / S0: S within TOL of sum w |x|, S0 within TOL of itself — and |centre| <= sum w |x| / S0
    ec = float((np.abs(c.centre.astype(LD) - r["centre"]) / (2 * r["abs_s"] / r["rho_sum"])).max())
    # core_radius = sqrt(Q2 / Q0), both sums of non-negative terms: half the sum of their relative errors
    er = float(abs(LD(c.core_radius) - r["core_radius"]) / r["core_radius"])
    print(f"{what}: rho_sum {e0:.3e}, rho2_sum {e1:.3e}, centre {ec:.3e} of sum w |x| / sum w, core_radius {er:.3e}")
    assert max(e0, e1, ec, er) < TOL_F64
    return r


@pytest.mark.parametrize("k", [2, 6])
def test_the_density_centre_and_the_core_radius(nb, k):
    n = 1000
    posm, vel, _, _ = C.scene(nb, n, 25)
    with f64(nb, n, time_kernels=True) as e:
        e.set_state(posm, vel)
        rho, _ = e.density_f64(k)
        f0 = passes(nb, e)
        c = e.core_f64(k)
        assert passes(nb, e) - f0 == 1 and c.k == k and c.used == n  # one pass: the reductions and mass_within are none
        core_held(f"N = {n}, k = {k}", c, rho, posm)
        again = e.core_f64(k)
        for a, b in zip(c, again):                                 # the same bits every run
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        d2c = ((posm[:, :3] - c.centre) ** 2).sum(1)
        inside = d2c <= c.core_radius ** 2
        assert c.core_count == int(inside.sum()) and abs(c.core_mass - posm[inside, 3].sum()) < 1e-12 * posm[:, 3].sum()


def test_a_planted_clump_is_the_density_centre(nb):
    posm, vel, members, scale = N.clump_scene(nb)
    n = posm.shape[0]
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        held("the clump scene", e.neighbours_f64(K8), N.neighbours(posm, dtype=LD), K8)
        rho, _ = e.density_f64(6)
        c = e.core_f64(6)
        core_held("the clump scene", c, rho, posm)
        spot = posm[members, :3].mean(0)
        assert np.linalg.norm(c.centre - spot) < 3 * N.CLUMP_SIGMA * scale      # inside the clump
        assert c.densest in members and c.rho_max == rho.max()
        com = np.asarray(e.moments().com)
        assert np.linalg.norm(com - spot) > scale                  # the centre of mass lies elsewhere
        inside = ((posm[:, :3] - c.centre) ** 2).sum(1) <= c.core_radius ** 2
        assert c.core_radius < 3 * N.CLUMP_SIGMA * scale and c.core_count == int(inside.sum()) and np.isin(np.flatnonzero(inside), members).all()


# ---- 10: nothing else moves ----------------------------------------------------------------------------------------------------------

def four_calls(e, pts):
    return e.neighbours_f64(), e.neighbours_at_f64(pts, 3), e.density_f64(), e.core_f64(K8)


def fourth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite_state() + e.hermite_tracers_state()


def sixth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite6_state() + e.hermite6_tracers_state()


def test_the_caches_and_the_tracers_stay(nb):
    n, m = 257, 300
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    with f64(nb, n, eps=0.05) as e, f64(nb, n, eps=0.05) as twin:
        for x in (e, twin):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
            x.hermite6_step(DT, 2); x.hermite_timescale(); x.hermite_tracers_timescale()   # both orders' caches, bodies and tracers
        before = fourth(e) + sixth(e)
        four_calls(e, tpos)
        for k, (a, b) in enumerate(zip(fourth(e) + sixth(e), before)):
            eq(a, b, f"array {k} behind the four calls")
        for k, (a, b) in enumerate(zip(fourth(e) + sixth(e), fourth(twin) + sixth(twin))):
            eq(a, b, f"array {k} against the twin")
        e.hermite6_step(DT, 1); twin.hermite6_step(DT, 1)          # and the steps behind them go on as the twin's
        for k, (a, b) in enumerate(zip(sixth(e), sixth(twin))):
            eq(a, b, f"array {k} a sixth-order step later, against the twin")
        e.hermite_step(DT, 1); twin.hermite_step(DT, 1)
        for k, (a, b) in enumerate(zip(fourth(e), fourth(twin))):
            eq(a, b, f"array {k} a fourth-order step later, against the twin")


@pytest.mark.parametrize("order", [4, 6])
def test_a_block_session_in_mid_frame_goes_on_as_its_twin(nb, order):
    n, m, levels = 257, 300, 8
    posm, vel, tpos, tvel = C.scene(nb, n, m)
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
        got = four_calls(e, tpos)
        for k, (a, b) in enumerate(zip(session(e), before)):
            eq(a, b, f"array {k} behind the four calls, in mid-frame")
        p, _, _ = e.state(np.float64)                              # the lists describe each body where it is: the live state's
        held("mid-frame", got[0], tuple(a[:, :6] if a.ndim == 2 else a for a in N.neighbours(p, dtype=LD)), 6)
        se, sw = advance(e), advance(twin)
        assert se == sw and se["synchronised"]
        for k, (a, b) in enumerate(zip(session(e), session(twin))):
            eq(a, b, f"array {k} at the frame end, against the twin")


# ---- 11: the contract ------------------------------------------------------------------------------------------------------------------

NAMES = ("nbody_get_neighbours_f64", "nbody_neighbours_at_f64", "nbody_get_density_f64", "nbody_density_centre_f64")


def four_lambdas(e, k=None):
    pts = np.zeros((3, 3)) + [[1.0], [2.0], [3.0]]
    kw = {} if k is None else {"k": k}
    return ((lambda: e.neighbours_f64(**kw)), (lambda: e.neighbours_at_f64(pts, **kw)), (lambda: e.density_f64(**kw)), (lambda: e.core_f64(**kw)))


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    """tests/cpp/fake_rccl.c, the suite's stand-in for the communication library, as tests/test_census_f64_gpu.py builds it: a
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
    for kw, why in (({}, "fp32"), ({"precision": "f32_kahan"}, "fp32"), ({"precision": "f64", "i_begin": 0, "i_count": 1000}, "slice"),
                    ({"devices": [0]}, "multi-device")):
        with nb.NBodyEngine(big, **kw) as e:
            if kw.get("precision") == "f64":
                e.set_state(p32.astype(np.float64), v32.astype(np.float64))
            else:
                e.set_state(p32, v32)
            for name, call in zip(NAMES, four_lambdas(e)):
                msg = raises(nb, E.ERR_UNSUPPORTED, call)
                assert name in msg and why in msg, (kw, msg)
    n, m = 257, 300
    posm, vel, tpos, _ = C.scene(nb, n, m)
    with f64(nb, n, time_kernels=True) as e:
        for call in four_lambdas(e):                               # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(posm, vel)
        f = [passes(nb, e)]
        for call in four_lambdas(e):                               # every call counts one pass
            call(); f.append(passes(nb, e))
        assert np.diff(f).tolist() == [1] * 4
        for k in (0, -1, 9, 1 << 20):                              # k out of range: 1 .. 8 for the lists, 2 .. 8 for the density calls
            for name, call in zip(NAMES, four_lambdas(e, k)):
                assert name in raises(nb, E.ERR_INVALID, call)
        for name, call in zip(NAMES[2:], four_lambdas(e, 1)[2:]):
            assert name in raises(nb, E.ERR_INVALID, call)
        assert e.neighbours_f64(1)[0].shape == (n, 1) and e.neighbours_at_f64(tpos, 1)[1].shape == (m, 1)
        assert passes(nb, e) - f[-1] == 2                          # a refused call is no pass
        k = 5
        idx = np.full((m, k), -7, np.int32); d2 = np.full((m, k), -7.0)
        P, I, D, L = tpos.ctypes.data, idx.ctypes.data, d2.ctypes.data, e._L
        A = L.nbody_neighbours_at_f64
        assert A(e._h, None, 24, m, k, I, D) == E.ERR_INVALID                                      # null points
        assert A(e._h, P, 24, m, k, None, None) == E.ERR_INVALID                                   # every output null
        assert A(e._h, P, 24, -1, k, I, D) == E.ERR_INVALID and A(e._h, P, 23, m, k, I, D) == E.ERR_INVALID   # n < 0, a short stride
        assert A(e._h, None, 0, 0, k, I, D) == E.ERR_INVALID                                       # null even with n == 0
        assert A(e._h, P, 24, 0, k, I, D) == 0                                                     # n == 0: a no-op
        assert (idx == -7).all() and (d2 == -7.0).all()
        want = e.neighbours_at_f64(tpos, k)
        assert A(e._h, P, 24, m, k, I, None) == 0 and (d2 == -7.0).all(); eq(idx, want[0], "the index alone")
        assert A(e._h, P, 24, m, k, None, D) == 0; eq(d2, want[1], "d2 alone")
        pts5 = np.full((m, 5), 7.0); pts5[:, :3] = tpos; idx[:] = -7; d2[:] = -7.0                    # strided rows in
        assert A(e._h, pts5.ctypes.data, 40, m, k, I, D) == 0; eq(idx, want[0], "index of strided points"); eq(d2, want[1], "d2 of strided points")
        bi = np.empty((n, k), np.int32); bd = np.empty((n, k)); rho = np.empty(n); rk2 = np.empty(n)
        G, R = L.nbody_get_neighbours_f64, L.nbody_get_density_f64
        assert G(e._h, k, None, None) == E.ERR_INVALID and R(e._h, k, None, None) == E.ERR_INVALID
        assert G(e._h, k, bi.ctypes.data, None) == 0 and G(e._h, k, None, bd.ctypes.data) == 0
        eq(bi, e.neighbours_f64(k)[0], "the bodies' index alone"); eq(bd, e.neighbours_f64(k)[1], "the bodies' d2 alone")
        assert R(e._h, k, rho.ctypes.data, None) == 0 and R(e._h, k, None, rk2.ctypes.data) == 0
        eq(rho, e.density_f64(k)[0], "rho alone"); eq(rk2, e.density_f64(k)[1], "rk2 alone"); eq(rk2, bd[:, k - 1], "rk2 is the k-th d2")
        core = E.Core()
        assert L.nbody_density_centre_f64(e._h, k, None) == E.ERR_INVALID                           # a null struct, a wrong size
        assert L.nbody_density_centre_f64(e._h, k, ctypes.byref(core)) == E.ERR_INVALID
        core.struct_size = ctypes.sizeof(core)
        assert L.nbody_density_centre_f64(e._h, k, ctypes.byref(core)) == 0 and core.k == k and core.used == n
        assert e.neighbours_at_f64(np.zeros((0, 3)))[0].shape == (0, 6)
        e.step_begin()                                             # a step is open
        for name, call in zip(NAMES, four_lambdas(e)):
            assert name in raises(nb, E.ERR_STATE, call)
        e.step_end(0.0)
        four_calls(e, tpos)


def test_command_line_core_every(nb):
    """--core-every 2 over four frames prints two core lines, and their values are core_f64()'s on the same state."""
    n = 512
    cmd = [sys.executable, "-m", "parallelnbody_amd", "--precision", "f64", "--plummer", "--n", str(n), "--steps", "4", "--core-every", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines()]
    cores = [ln for ln in lines if "core" in ln]
    assert [ln["frame"] for ln in cores] == [2, 4] and len(lines) == 3
    posm, vel = nb.ic_plummer(n, G=1.0e4, seed=1)
    with nb.NBodyEngine(n, precision="f64", G=1.0e4) as e:
        e.set_state(posm, vel)
        for ln in cores:
            e.step(0.01, 2)
            c = e.core_f64(6)
            assert ln["core"] == {"k": 6, "centre": [float(x) for x in c.centre], "core_radius": c.core_radius, "densest": c.densest,
                                  "rho_max": c.rho_max, "used": c.used, "core_mass": c.core_mass, "core_count": c.core_count}
            assert c.used == n and c.core_count > 0
    bad = subprocess.run([sys.executable, "-m", "parallelnbody_amd", "--n", "64", "--steps", "1", "--core-every", "1"], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert bad.returncode == 2 and "--core-every needs --precision f64" in bad.stderr
