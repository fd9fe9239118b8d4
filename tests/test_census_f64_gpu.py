"""The fp64 pair census — nbody_get_nearest_f64, nbody_nearest_at_f64, nbody_closest_pair_f64, nbody_get_partners_f64,
nbody_partner_at_f64, nbody_hardest_pair_f64, nbody_pair_time_f64 — on the device.

The yardstick is tests/census_f64_ref.py in long double on the scenes of pot_tidal_f64_ref.plummer_scene.  An argmin can be held to a
reference only where its runner-up is far enough away, so every test that compares indices first asserts the GAP CONDITION on ALL of
its rows (no row is ever left out): the reference's gap exceeds 1e-9, 1000 x the bound of the values (tests/test_census_f64_ref.py
shows the scenes four orders above it, on the CPU).  Values: d2 within TOL_F64 relative; e within TOL_F64 of 0.5 |w|^2 + (G m_j + g) t,
the two terms e is the difference of.

Measured on an MI355X, the largest over all rows of all accuracy tests here: d2 3.7e-16, e 3.1e-16 of its scale."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import census_f64_ref as C
from jerk_ref import G, probe_geometry

pytestmark = pytest.mark.gpu

DT = 1e-3
TOL_F64 = 1e-12                                                    # the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
LD = np.longdouble
INF = np.inf


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


def held(what, near, part, ref, rows=None):
    """(index, d2) of a nearest call and (index, e, d2) of a partner call, at `rows` of them (None: all), against one long-double
    census dict: the gap condition on every row first, then every index, then the values.  Returns the three largest errors."""
    C.gaps_hold(ref)
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    ni, nd2 = (pick(a) for a in near)
    pi, pe, pd2 = (pick(a) for a in part)
    assert ni.dtype == np.int32 and pi.dtype == np.int32
    assert (ni == ref["near"]).all(), f"{what}: {int((ni != ref['near']).sum())} nearest indices differ"
    assert (pi == ref["part"]).all(), f"{what}: {int((pi != ref['part']).sum())} partner indices differ"
    ed = float(np.abs((nd2.astype(LD) - ref["near_d2"]) / ref["near_d2"]).max())
    ep = float(np.abs((pd2.astype(LD) - ref["part_d2"]) / ref["part_d2"]).max())
    ee = float(np.abs((pe.astype(LD) - ref["part_e"]) / ref["part_scale"]).max())
    print(f"{what}: nearest d2 {ed:.3e}, partner d2 {ep:.3e}, e {ee:.3e} of the long-double census")
    assert max(ed, ep, ee) < TOL_F64
    return ed, ep, ee


# ---- 1: against long double ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", C.CASES)
@pytest.mark.parametrize("eps", C.EPS)
def test_bodies_and_points_against_the_long_double_census(nb, n, m, eps):
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    with f64(nb, n, eps=eps, time_kernels=True) as e:
        e.set_state(posm, vel)
        f = [passes(nb, e)]
        near = e.nearest_f64(); f.append(passes(nb, e))
        part = e.partners_f64(); f.append(passes(nb, e))
        pnear = e.nearest_at_f64(tpos); f.append(passes(nb, e))
        ppart = e.partner_at_f64(tpos, tvel); f.append(passes(nb, e))
        closest = e.closest_pair_f64(); f.append(passes(nb, e))
        hardest = e.hardest_pair_f64(); f.append(passes(nb, e))
        e.pair_time_f64(); f.append(passes(nb, e))
        assert np.diff(f).tolist() == [1] * 7                      # one pass under NBODY_KERNEL_FORCES each
        held(f"N = {n}, eps = {eps}, bodies", near, part, C.reference(nb, "bodies", n, m)[eps])
        held(f"N = {n}, M = {m}, eps = {eps}, points", pnear, ppart, C.reference(nb, "points", n, m)[eps])
        assert near[0].shape == near[1].shape == (n,) and ppart[0].shape == ppart[1].shape == ppart[2].shape == (m,)
        assert closest == C.pair_of(*near) and hardest[:3] == C.pair_of(part[0], part[1]) and hardest[3] == part[2][hardest[0]]
        assert closest[0] < closest[1] and hardest[0] < hardest[1]
        p, v, _ = e.state(np.float64)
        eq(p, posm, "positions"); eq(v, vel, "velocities")


# ---- 2: 512-body chunks ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", C.EPS)
def test_bodies_at_512_body_chunks(nb, eps):
    """N = 32769: 65 chunks of 512 bodies, the last one holds one body and 255 pads.  All bodies are computed; 134 sampled ones — the
    first and the last 64, and those round the tile and chunk boundaries — are held to the long-double census."""
    n = C.N_CHUNKS
    assert probe_geometry(n) == (65, 512)
    posm, vel, _, _ = C.scene(nb, n)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        near, part = e.nearest_f64(), e.partners_f64()
        held(f"N = {n}, eps = {eps}, 134 bodies", near, part, C.reference(nb, "chunks", 0)[eps], rows=C.ROWS_CHUNKS)
        assert (near[0] >= 0).all() and (near[0] < n).all() and (part[0] >= 0).all() and (part[0] < n).all()
        assert (near[0] != np.arange(n)).all() and (part[0] != np.arange(n)).all()
        # the reductions over more bodies than one workgroup per slot
        assert e.closest_pair_f64() == C.pair_of(*near) and e.hardest_pair_f64()[:3] == C.pair_of(part[0], part[1])


# ---- 3: the padding of a chunk's last tile is nobody ---------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", C.EPS)
def test_the_padding_is_not_a_body(nb, eps):
    """N = 257: the second chunk holds one body and 255 pads on the origin, at rest, of mass 0.  Points at and next to the origin would
    find a pad at d2 = 0 / 1e-6 if it were admitted by anything but its index."""
    n = 257
    posm, vel, _, _ = C.scene(nb, n)
    pts = np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [0.0, -1e-3, 0.0], [1e-3, 1e-3, 1e-3], [0.0, 0.0, 1e-6]])
    ref = C.census(posm[:, :3], posm[:, 3], vel, pts, eps=(eps,), dtype=LD)[0]
    true_d2 = ((posm[None, :, :3] - pts[:, None, :]) ** 2).sum(-1).min(1)
    assert true_d2.min() > 1e-4                                    # (no body is anywhere near as close as a pad would be)
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        near, part = e.nearest_at_f64(pts), e.partner_at_f64(pts)
        assert (near[1] >= true_d2 * (1 - 1e-12)).all() and (part[2] >= true_d2 * (1 - 1e-12)).all()
        assert (near[0] >= 0).all() and (near[0] < n).all() and (part[0] >= 0).all() and (part[0] < n).all()
        held(f"N = {n}, eps = {eps}, points round the origin", near, part, ref)
        # and a body put onto the origin is found there, by everyone near it, as a body
        moved = posm.copy(); moved[256, :3] = 0.0
        e.set_state(moved, vel)
        near = e.nearest_at_f64(pts)
        assert near[0].tolist() == [256] * 5 and near[1][0] == 0.0 and near[1][1] == 1e-3 * 1e-3


# ---- 4: exact ties and coincident bodies, byte for byte ------------------------------------------------------------------------------

def test_exact_ties_and_coincident_bodies_byte_for_byte(nb):
    """300 equal masses on a small-integer lattice with integer velocities, shuffled, six of them on top of others: every operation
    in d2 and |w|^2 is exact, so index and d2 are plain numpy float64's in every byte and every tie goes to the lowest index — across
    tiles and across the two chunks.  Partner ties are those of equal (d2, |w|^2): e comes from the same operations on the same
    operands.  Beyond the exact ties no runner-up is within 1e-9."""
    posm, vel = C.lattice_scene()
    n = posm.shape[0]
    beyond = C.census(posm[:, :3], posm[:, 3], vel, dtype=LD, beyond_exact_ties=True)[0]
    assert float(beyond["near_gap"].min()) > C.GAP_MIN and float(beyond["part_gap"].min()) > C.GAP_MIN
    ref = C.census(posm[:, :3], posm[:, 3], vel)[0]                 # float64: exact where the device is
    ld = C.census(posm[:, :3], posm[:, 3], vel, dtype=LD)[0]
    assert (ref["near"] == ld["near"]).all() and (ref["part"] == ld["part"]).all()
    pts = posm[::7, :3] + [0.5, 0.0, 0.0]                           # half-way between sites: ties again, exact again
    pref = C.census(posm[:, :3], posm[:, 3], vel, pts, vel[::7, :3])[0]
    pbeyond = C.census(posm[:, :3], posm[:, 3], vel, pts, vel[::7, :3], dtype=LD, beyond_exact_ties=True)[0]
    assert float(pbeyond["near_gap"].min()) > C.GAP_MIN and float(pbeyond["part_gap"].min()) > C.GAP_MIN
    assert (pref["near"] == pbeyond["near"]).all() and (pref["part"] == pbeyond["part"]).all()
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        near, part = e.nearest_f64(), e.partners_f64()
        eq(near[0], ref["near"], "nearest index"); eq(near[1], ref["near_d2"], "nearest d2")
        eq(part[0], ref["part"], "partner index"); eq(part[2], ref["part_d2"], "partner d2")
        assert np.abs((part[1].astype(LD) - ld["part_e"]) / ld["part_scale"]).max() < TOL_F64
        assert (near[1] == 0).sum() == 12 and (near[0][near[1] == 0] != np.arange(n)[near[1] == 0]).all()
        pnear, ppart = e.nearest_at_f64(pts), e.partner_at_f64(pts, vel[::7, :3])
        eq(pnear[0], pref["near"], "nearest index at points"); eq(pnear[1], pref["near_d2"], "nearest d2 at points")
        eq(ppart[0], pref["part"], "partner index at points"); eq(ppart[2], pref["part_d2"], "partner d2 at points")
        onto = e.nearest_at_f64(posm[:, :3])                        # a body asked about as a point gets itself — or the lower of two coincident ones
        assert (onto[1] == 0).all() and (onto[0] <= np.arange(n)).all()
        assert ((onto[0] == np.arange(n)) | (near[1] == 0)).all()


# ---- 5: identities without a reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", C.EPS)
def test_symmetry_subsets_and_the_pair_calls(nb, eps):
    n, m = 4097, 3000
    posm, vel, _, _ = C.scene(nb, n, 64)
    rng = np.random.default_rng(5)
    pts = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3)); pv = rng.normal(0.0, float(np.abs(vel[:, :3]).std()), (m, 3))
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        (ni, nd2), (pi, pe, pd2) = e.nearest_f64(), e.partners_f64()
        i = np.arange(n)
        mutual = ni[ni] == i
        assert mutual.sum() > n // 4
        eq(nd2[mutual], nd2[ni[mutual]], "d2 of mutual nearest neighbours")
        mutual = pi[pi] == i
        assert mutual.sum() > n // 8
        eq(pe[mutual], pe[pi[mutual]], "e of mutual partners"); eq(pd2[mutual], pd2[pi[mutual]], "d2 of mutual partners")
        same = ni == pi                                            # where the partner is the nearest, its d2 is the nearest's
        assert same.any()
        eq(pd2[same], nd2[same], "the partner's d2 where it is the nearest")
        k = int(np.argmin(nd2))
        assert e.closest_pair_f64() == (k, int(ni[k]), float(nd2[k]))
        k = int(np.argmin(pe))
        assert e.hardest_pair_f64() == (k, int(pi[k]), float(pe[k]), float(pd2[k]))
        # a subset of the points alone is its rows of the big query: 3000 and 1500 points go two rows a lane, 300 and 1 go one
        near, part = e.nearest_at_f64(pts), e.partner_at_f64(pts, pv)
        for lo, hi in ((100, 400), (500, 2000), (2999, 3000)):
            for a, b in zip(e.nearest_at_f64(pts[lo:hi]) + e.partner_at_f64(pts[lo:hi], pv[lo:hi]), near + part):
                eq(a, b[lo:hi], f"points {lo} .. {hi} alone")
        for a, b in zip(e.partner_at_f64(pts), e.partner_at_f64(pts, np.zeros_like(pts))):
            eq(a, b, "at rest")
        # a body queried as a point gets itself at d2 = 0
        oi, od2 = e.nearest_at_f64(posm[:, :3])
        eq(oi, i.astype(np.int32), "a body as a point: itself"); assert not od2.any()


def test_points_beyond_one_slab_of_the_staging_area(nb):
    """N = 33000: 65 chunks, so a slab of the partner's rows (two float4 per point and chunk) is 129024 points.  1000 more: the 16
    points astride the boundary equal the same points queried alone, and 32 sampled points are held to long double."""
    n, eps = C.N_SLAB, 0.05
    posm, vel, _, _ = C.scene(nb, n)
    pts, pv, sampled = C.slab_points(nb)
    slab = C.probe_slab_points(n, 2)
    assert slab == 129024 and pts.shape[0] == slab + 1000
    with f64(nb, n, eps=eps) as e:
        e.set_state(posm, vel)
        part = e.partner_at_f64(pts, pv)
        near = e.nearest_at_f64(pts)
        lo, hi = slab - 8, slab + 8
        for a, b in zip(e.partner_at_f64(pts[lo:hi], pv[lo:hi]), part):
            eq(a, b[lo:hi], "the 16 points astride the slab boundary")
        for a, b in zip(e.partner_at_f64(pts[-300:], pv[-300:]), part):
            eq(a, b[-300:], "the last 300 points")
        held(f"N = {n}, eps = {eps}, 32 of {pts.shape[0]} points", near, part, C.reference(nb, "slab", 0)[eps], rows=sampled)


# ---- 6: edges --------------------------------------------------------------------------------------------------------------------------

def test_one_body_and_two_bodies(nb):
    with f64(nb, 1) as e:
        e.set_state(np.array([[1.5, -2.25, 3.0, 7.0]]), np.zeros((1, 4)))
        ni, nd2 = e.nearest_f64(); pi, pe, pd2 = e.partners_f64()
        assert ni.tolist() == [-1] and pi.tolist() == [-1] and nd2[0] == INF and pe[0] == INF and pd2[0] == INF
        assert e.closest_pair_f64() == (-1, -1, INF) and e.hardest_pair_f64() == (-1, -1, INF, INF) and e.pair_time_f64() == (INF, -1, -1)
        assert e.binaries_f64().shape == (0,)
        ni, nd2 = e.nearest_at_f64(np.array([[1.5, -2.25, 4.0]]))
        assert ni.tolist() == [0] and nd2[0] == 1.0
    posm = np.array([[1.5, -2.25, 3.0, 7.0], [-0.5, 1.0, 4.25, 11.0]]); vel = np.array([[0.5, 0.0, 0.0, 0.0], [0.0, -0.25, 0.0, 0.0]])
    d = (posm[1, :3] - posm[0, :3]).astype(LD); w = (vel[1, :3] - vel[0, :3]).astype(LD)
    d2 = (d * d).sum()
    for eps in C.EPS:
        t = 1 / np.sqrt(d2 + LD(eps) * LD(eps))
        want, scale = (w * w).sum() / 2 - LD(G) * 18 * t, (w * w).sum() / 2 + LD(G) * 18 * t
        with f64(nb, 2, eps=eps) as e:
            e.set_state(posm, vel)
            ni, nd2 = e.nearest_f64(); pi, pe, pd2 = e.partners_f64()
            assert ni.tolist() == [1, 0] and pi.tolist() == [1, 0]
            assert nd2[0] == nd2[1] == pd2[0] == pd2[1] and pe[0] == pe[1]
            assert abs(float(nd2[0] - d2)) < TOL_F64 * float(d2) and abs(float(pe[0] - want)) < TOL_F64 * float(scale)
            assert e.closest_pair_f64() == (0, 1, nd2[0]) and e.hardest_pair_f64() == (0, 1, pe[0], pd2[0])
            assert e.pair_time_f64() == (C.pair_time_of(nd2[0], 7.0, 11.0), 0, 1)
        with f64(nb, 2, eps=eps) as e:                             # a massless pair has no free-fall scale
            massless = posm.copy(); massless[:, 3] = 0.0
            e.set_state(massless, vel)
            assert e.pair_time_f64() == (INF, 0, 1) and e.closest_pair_f64() == (0, 1, nd2[0])


@pytest.mark.parametrize("eps", C.EPS)
def test_a_body_whose_position_is_nan(nb, eps):
    n, k = 257, 100
    posm, vel, tpos, tvel = C.scene(nb, n, 300)
    bad = posm.copy(); bad[k, 0] = np.nan
    rest = np.arange(n) != k
    with f64(nb, n, eps=eps) as e, f64(nb, n - 1, eps=eps) as without:
        e.set_state(bad, vel); without.set_state(posm[rest], vel[rest])
        near, part = e.nearest_f64(), e.partners_f64()
        assert near[0][k] == -1 and near[1][k] == INF and part[0][k] == -1 and part[1][k] == INF and part[2][k] == INF
        assert (near[0] != k).all() and (part[0] != k).all()       # nobody chooses it
        wn, wp = without.nearest_f64(), without.partners_f64()     # all other rows are as without it: its chunk-mates move up by one
        up = lambda idx: np.where(idx >= k, idx + 1, idx).astype(np.int32)
        eq(near[0][rest], up(wn[0]), "nearest index"); eq(part[0][rest], up(wp[0]), "partner index")
        eq(near[1][rest], wn[1], "nearest d2"); eq(part[1][rest], wp[1], "partner e"); eq(part[2][rest], wp[2], "partner d2")
        pn, pp = e.nearest_at_f64(tpos), e.partner_at_f64(tpos, tvel)
        qn, qp = without.nearest_at_f64(tpos), without.partner_at_f64(tpos, tvel)
        eq(pn[0], up(qn[0]), "nearest index at points"); eq(pn[1], qn[1], "nearest d2 at points")
        eq(pp[0], up(qp[0]), "partner index at points"); eq(pp[1], qp[1], "partner e at points"); eq(pp[2], qp[2], "partner d2 at points")
        pn, pp = e.nearest_at_f64(np.array([[np.nan, 0.0, 0.0]])), e.partner_at_f64(np.array([[0.0, np.inf, 0.0]]))
        assert pn[0][0] == -1 and pn[1][0] == INF and pp[0][0] == -1 and pp[1][0] == INF and pp[2][0] == INF


# ---- 7: a planted binary ---------------------------------------------------------------------------------------------------------------

def test_a_planted_binary_is_found(nb):
    posm, vel, a, ecc = C.binary_scene(nb)
    n = posm.shape[0]
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        i, j, energy, d2 = e.hardest_pair_f64()
        assert (i, j) == (0, 1)
        mu = G * (posm[0, 3] + posm[1, 3])
        b = e.binaries_f64()
        assert b.dtype == e.BINARY_DTYPE and (b["i"] < b["j"]).all() and (b["energy"] < 0).all()
        pi, pe, _ = e.partners_f64()
        for row in b:
            assert pi[row["i"]] == row["j"] and pi[row["j"]] == row["i"] and pe[row["i"]] == row["energy"]
        first = b[0]
        assert (first["i"], first["j"], first["energy"]) == (0, 1, energy)
        print(f"the planted binary: a {first['a']!r}, ecc {first['ecc']!r}; {b.size} bound mutual pairs in all")
        assert abs(first["a"] - a) < 1e-9 * a and abs(first["ecc"] - ecc) < 1e-9
        assert abs(energy + mu / (2 * a)) < 1e-9 * mu / (2 * a)
        ci, cj, cd2 = e.closest_pair_f64()
        assert e.pair_time_f64() == (C.pair_time_of(cd2, posm[ci, 3], posm[cj, 3]), ci, cj)
        assert (ci, cj) == (0, 1) and abs(cd2 - 0.25) < 1e-12      # at pericentre: a (1 - e) = 0.5


# ---- 8: nothing else moves, and the contract -----------------------------------------------------------------------------------------

def seven_calls(e, pts, pv):
    return (e.nearest_f64(), e.nearest_at_f64(pts), e.closest_pair_f64(), e.partners_f64(), e.partner_at_f64(pts, pv), e.hardest_pair_f64(),
            e.pair_time_f64(), e.binaries_f64())


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
        seven_calls(e, tpos, tvel)
        for k, (a, b) in enumerate(zip(fourth(e) + sixth(e), before)):
            eq(a, b, f"array {k} behind the seven calls")
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
        got = seven_calls(e, tpos, tvel)
        for k, (a, b) in enumerate(zip(session(e), before)):
            eq(a, b, f"array {k} behind the seven calls, in mid-frame")
        # the rows describe each body where it is, at its own time: the live state's census
        p, v, _ = e.state(np.float64)
        ref = C.census(p[:, :3], p[:, 3], v, eps=(0.05,), dtype=LD)[0]
        held("mid-frame", got[0], got[3], ref)
        se, sw = advance(e), advance(twin)
        assert se == sw and se["synchronised"]
        for k, (a, b) in enumerate(zip(session(e), session(twin))):
            eq(a, b, f"array {k} at the frame end, against the twin")


NAMES = ("nbody_get_nearest_f64", "nbody_nearest_at_f64", "nbody_closest_pair_f64", "nbody_get_partners_f64", "nbody_partner_at_f64",
         "nbody_hardest_pair_f64", "nbody_pair_time_f64")


def seven_lambdas(e):
    pts = np.zeros((3, 3)) + [[1.0], [2.0], [3.0]]
    return (e.nearest_f64, (lambda: e.nearest_at_f64(pts)), e.closest_pair_f64, e.partners_f64, (lambda: e.partner_at_f64(pts)),
            e.hardest_pair_f64, e.pair_time_f64)


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    """tests/cpp/fake_rccl.c, the suite's stand-in for the communication library, as tests/test_pot_tidal_f64_gpu.py builds it: a
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
            for name, call in zip(NAMES, seven_lambdas(e)):
                msg = raises(nb, E.ERR_UNSUPPORTED, call)
                assert name in msg and why in msg, (kw, msg)
            raises(nb, E.ERR_UNSUPPORTED, e.binaries_f64)
    n, m = 257, 300
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    with f64(nb, n) as e:
        for call in seven_lambdas(e):                              # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(posm, vel)
        idx = np.full(m, -7, np.int32); val = np.full(m, -7.0); d2 = np.full(m, -7.0)
        P, V, I, A, D, L = tpos.ctypes.data, tvel.ctypes.data, idx.ctypes.data, val.ctypes.data, d2.ctypes.data, e._L
        N, Q = L.nbody_nearest_at_f64, L.nbody_partner_at_f64
        assert N(e._h, None, 24, m, I, D) == E.ERR_INVALID and Q(e._h, None, 24, V, 24, m, I, A, D) == E.ERR_INVALID           # null points
        assert N(e._h, P, 24, m, None, None) == E.ERR_INVALID and Q(e._h, P, 24, V, 24, m, None, None, None) == E.ERR_INVALID   # every output null
        assert N(e._h, P, 24, -1, I, D) == E.ERR_INVALID and Q(e._h, P, 24, V, 24, -1, I, A, D) == E.ERR_INVALID                 # n < 0
        assert N(e._h, P, 23, m, I, D) == E.ERR_INVALID and Q(e._h, P, 23, V, 24, m, I, A, D) == E.ERR_INVALID                   # short strides
        assert Q(e._h, P, 24, V, 23, m, I, A, D) == E.ERR_INVALID
        assert N(e._h, None, 0, 0, I, D) == E.ERR_INVALID                                                                       # null even with n == 0
        assert N(e._h, P, 24, 0, I, D) == 0 and Q(e._h, P, 24, None, 0, 0, I, A, D) == 0                                         # n == 0: a no-op
        assert (idx == -7).all() and (val == -7.0).all() and (d2 == -7.0).all()
        near, part = e.nearest_at_f64(tpos), e.partner_at_f64(tpos, tvel)
        assert N(e._h, P, 24, m, I, None) == 0 and (d2 == -7.0).all(); eq(idx, near[0], "the index alone")                       # each output alone
        assert N(e._h, P, 24, m, None, D) == 0; eq(d2, near[1], "d2 alone")
        assert Q(e._h, P, 24, V, 24, m, None, A, None) == 0; eq(val, part[1], "e alone"); eq(d2, near[1], "(d2 untouched)")
        assert Q(e._h, P, 24, V, 24, m, I, None, D) == 0; eq(idx, part[0], "the partner index"); eq(d2, part[2], "the partner d2")
        pts5 = np.full((m, 5), 7.0); pts5[:, :3] = tpos; vel4 = np.full((m, 4), 7.0); vel4[:, :3] = tvel                          # strided rows in
        assert Q(e._h, pts5.ctypes.data, 40, vel4.ctypes.data, 32, m, I, A, D) == 0
        eq(idx, part[0], "index of strided points"); eq(val, part[1], "e of strided points"); eq(d2, part[2], "d2 of strided points")
        bi = np.empty(n, np.int32); bv = np.empty(n); bd = np.empty(n)
        assert L.nbody_get_nearest_f64(e._h, None, None) == E.ERR_INVALID and L.nbody_get_partners_f64(e._h, None, None, None) == E.ERR_INVALID
        assert L.nbody_get_nearest_f64(e._h, bi.ctypes.data, None) == 0 and L.nbody_get_partners_f64(e._h, None, bv.ctypes.data, None) == 0
        eq(bi, e.nearest_f64()[0], "the bodies' index alone"); eq(bv, e.partners_f64()[1], "the bodies' e alone")
        assert L.nbody_get_partners_f64(e._h, None, None, bd.ctypes.data) == 0; eq(bd, e.partners_f64()[2], "the bodies' partner d2 alone")
        assert L.nbody_closest_pair_f64(e._h, None, None, None) == E.ERR_INVALID
        assert L.nbody_hardest_pair_f64(e._h, None, None, None, None) == E.ERR_INVALID
        assert L.nbody_pair_time_f64(e._h, None, None, None) == E.ERR_INVALID
        i, j, x = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_double(-7.0)
        assert L.nbody_closest_pair_f64(e._h, None, ctypes.byref(j), None) == 0 and j.value == e.closest_pair_f64()[1]
        assert L.nbody_hardest_pair_f64(e._h, ctypes.byref(i), None, None, ctypes.byref(x)) == 0
        assert (i.value, x.value) == (e.hardest_pair_f64()[0], e.hardest_pair_f64()[3])
        assert L.nbody_pair_time_f64(e._h, ctypes.byref(x), None, None) == 0 and x.value == e.pair_time_f64()[0]
        assert e.nearest_at_f64(np.zeros((0, 3)))[0].shape == (0,) and e.partner_at_f64(np.zeros((0, 3)))[1].shape == (0,)
        e.step_begin()                                             # a step is open
        for name, call in zip(NAMES, seven_lambdas(e)):
            assert name in raises(nb, E.ERR_STATE, call)
        e.step_end(0.0)
        seven_calls(e, tpos, tvel)
