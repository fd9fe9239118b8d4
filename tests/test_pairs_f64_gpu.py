"""The fp64 separation census — nbody_get_pair_counts_f64, nbody_pair_counts_at_f64 — on the device.

The yardstick is tests/pairs_f64_ref.py: include/nbody.h's definitions in numpy, float64.  d2 is formed without contraction, so numpy
forms the same bits and every pair is decided alike: every answer is an exact integer and EVERY comparison here is an equality of int64
arrays.  Per size ONE mirror run answers a master list of distinct radii in a shuffled order; the sets of k = 1, G - 1, G, G + 1 (and 64)
radii are its first k — each radius is answered on its own, so their counts are the first k of the master's."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import census_f64_ref as C
import groups_f64_ref as R
import pairs_f64_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1e-3
G = P.G
I64 = ctypes.POINTER(ctypes.c_int64)
F64 = ctypes.POINTER(ctypes.c_double)


def f64(nb, n, **kw):
    return nb.NBodyEngine(n, precision="f64", **kw)


def loaded(nb, posm, **kw):
    e = f64(nb, len(posm), **kw)
    e.set_state(np.array(posm), np.zeros((len(posm), 4)))
    return e


def eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.int64, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what}: {a.tolist()} != {b.tolist()}"


def raises(nb, code, call):
    with pytest.raises(nb.NBodyError) as er:
        call()
    assert er.value.code == code, (er.value.code, str(er.value))
    return str(er.value)


def passes(nb, e):
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]


# ---- 1: every size against the mirror -------------------------------------------------------------------------------------------------------

def master_radii(n):
    """the distinct radii a Gaussian scene of n bodies is asked at, shuffled: up to beyond the system where the mirror stays quick"""
    if n <= 1000:
        return P.radii_set(P.K_MAX, 0.02, 12.0)
    return P.radii_set(P.K_MAX, 0.01, 0.5) if n <= 4097 else P.radii_set(G + 1, 0.005, 0.1)


@functools.lru_cache(maxsize=None)
def master(n):
    radii = master_radii(n)
    want = P.pair_counts(R.scene(f"gauss{n}"), radii)
    radii.setflags(write=False); want.setflags(write=False)
    return radii, want


@pytest.mark.parametrize("n", R.GAUSS_SIZES)
def test_counts_of_every_size_and_every_k_round_a_launch_group(nb, n):
    radii, want = master(n)
    with loaded(nb, R.scene(f"gauss{n}"), time_kernels=True) as e:
        for k in (1, G - 1, G, G + 1) + ((P.K_MAX,) if n <= 4097 else ()):
            f0, u0 = passes(nb, e)
            got = e.pair_counts_f64(radii[:k])
            print(f"N = {n}, k = {k}: {got.tolist()}")
            eq(got, want[:k], f"N = {n}, k = {k}")
            assert passes(nb, e) == (f0 + (k + G - 1) // G, u0)     # ceil(k_distinct / G) passes, no update
            eq(e.pair_counts_f64(radii[:k]), got, f"N = {n}, k = {k}: a second call")
        if n <= 1000:
            assert want.max() == n * (n - 1) // 2                   # (the largest radius holds every pair)


def test_unsorted_radii_with_repeats_zero_and_one_beyond_the_system(nb):
    n = 1000
    posm = R.scene(f"gauss{n}")
    radii = np.array([0.4, 0.05, 0.4, 0.0, 50.0, 0.2, 0.05, 0.2000000000000001, -0.0, 1.0, 0.4])
    with loaded(nb, posm, time_kernels=True) as e:
        f0, u0 = passes(nb, e)
        got = e.pair_counts_f64(radii)
        assert passes(nb, e) == (f0 + 1, u0)                        # fewer than G distinct squares: one pass
        eq(got, P.pair_counts(posm, radii), "the mirror")
        eq(got, np.array([e.pair_counts_f64([r])[0] for r in radii], np.int64), "each radius on its own")
        assert got[0] == got[2] == got[10] and got[3] == got[8] == 0 and got[4] == n * (n - 1) // 2
        many = np.concatenate([P.radii_set(2 * G, 0.02, 3.0), P.radii_set(2 * G, 0.02, 3.0)[::-1]])   # 64 radii, 32 distinct
        f0, u0 = passes(nb, e)
        eq(e.pair_counts_f64(many), P.pair_counts(posm, many), "64 radii, 32 distinct")
        assert passes(nb, e) == (f0 + 2, u0)                        # ... in two passes
        shaped = e.pair_counts_f64(radii[:6].reshape(2, 3))         # shaped like the radii
        assert shaped.shape == (2, 3) and shaped.dtype == np.int64 and shaped.reshape(-1).tolist() == got[:6].tolist()


def test_the_identities_with_the_group_census_and_mass_within(nb):
    n = 1000
    posm = R.scene(f"gauss{n}")
    radii = np.array([0.0, 0.05, 0.2, 0.4, 1.0, 2.5, 100.0])
    with loaded(nb, posm) as e:
        got = e.pair_counts_f64(radii)
        for r, c in zip(radii, got):
            assert int(c) == e.groups_f64(r).summary.links == int(e.radius_counts_f64(r).astype(np.int64).sum()) // 2, r
        points = np.random.default_rng(3).normal(0.0, 1.0, (300, 3))
        at = e.pair_counts_at_f64(points, radii)
        eq(at, np.array([e.radius_counts_at_f64(points, r).astype(np.int64).sum() for r in radii], np.int64), "the sum of the radius counts")
        for c in (np.zeros(3), posm[17, :3], np.array([0.3, -0.2, 1.1])):
            eq(e.pair_counts_at_f64(c[None, :], radii), e.mass_within(c, radii)[1], "one point against mass_within's count")
        # the points at the bodies' own positions: every ordered pair, and every body whose d2 to itself is 0
        eq(e.pair_counts_at_f64(posm[:, :3], radii), 2 * got + n, "the bodies as points")


# ---- 2: the points ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", (None, "1", "2"))
@pytest.mark.parametrize("m", R.POINT_COUNTS)
def test_counts_at_points_one_and_two_rows_per_lane(nb, monkeypatch, m, lanes):
    n = 4097
    posm = R.scene(f"gauss{n}")
    points = np.random.default_rng(100 + m).normal(0.0, 1.0, (m, 3))
    points[0] = posm[n - 1, :3]                                     # on the one body of the last chunk
    radii = np.concatenate([[0.0, 50.0], P.radii_set(G, 0.05, 0.6)])   # G + 2 radii: two passes
    want = P.pair_counts_at(points, posm, radii)
    assert want[0] == 1 and want[1] == m * n
    if lanes is None:
        monkeypatch.delenv("NBODY_PAIRS64_LANES", raising=False)
    else:
        monkeypatch.setenv("NBODY_PAIRS64_LANES", lanes)            # read at every call
    with loaded(nb, posm, time_kernels=True) as e:
        f0, u0 = passes(nb, e)
        got = e.pair_counts_at_f64(points, radii)
        eq(got, want, f"M = {m}, lanes = {lanes}")
        assert passes(nb, e) == (f0 + 2, u0)
        eq(e.pair_counts_at_f64(points, radii), got, "a second call")
        monkeypatch.delenv("NBODY_PAIRS64_LANES", raising=False)
        eq(e.pair_counts_at_f64(points, radii), got, "the library's own choice of lanes")
        none = e.pair_counts_at_f64(np.zeros((0, 3)), radii)        # M = 0: NBODY_OK, zeros, no pass
        assert none.dtype == np.int64 and none.tolist() == [0] * len(radii) and passes(nb, e) == (f0 + 6, u0)


# ---- 3: structure ----------------------------------------------------------------------------------------------------------------------------

def test_a_lattice_at_and_just_below_its_spacing(nb):
    with loaded(nb, R.scene("lattice")) as e:
        assert e.pair_counts_f64([1.0, 0.99]).tolist() == [3 * 9 * 9 * 8, 0]


def test_all_bodies_on_one_point_at_radius_zero(nb):
    posm = R.scene("coincident")
    n = len(posm)
    with loaded(nb, posm) as e:
        assert e.pair_counts_f64([0.0, 1.0]).tolist() == [n * (n - 1) // 2] * 2
        assert e.pair_counts_at_f64(posm[:7, :3], [0.0]).tolist() == [7 * n]


def test_nan_and_infinite_positions_count_nowhere(nb):
    posm = R.scene("nonfinite")
    radii = np.array([0.4, 0.0, 1e3, 1e150])
    with loaded(nb, posm) as e:
        got = e.pair_counts_f64(radii)
        eq(got, P.pair_counts(posm, radii), "the mirror")
        assert got[0] == R.case("nonfinite", 0.4)["summary"].links
        finite = len(posm) - len(R.NONFINITE_BODIES)
        assert got[2] == got[3] == finite * (finite - 1) // 2       # the six bodies that are not finite are in no pair at any radius
        at = e.pair_counts_at_f64(posm[:, :3], radii)
        eq(at, P.pair_counts_at(posm[:, :3], posm, radii), "the mirror at the bodies' own positions")
        eq(at, 2 * got + finite, "a body that is not finite is not within any radius of itself")


@pytest.mark.parametrize("n", (65537, 131072))
def test_totals_beyond_32_bits(nb, n):
    """every body in a box of side 1, one radius beyond its diagonal and one that holds no pair: exactly n (n - 1) / 2 — more than 2^32
    ordered pairs from N = 65537, more than 2^32 unordered ones at N = 131072.  No mirror is needed."""
    posm = np.ones((n, 4))
    posm[:, :3] = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3))
    total = n * (n - 1) // 2
    assert 2 * total > 2 ** 32 and (n < 131072 or total > 2 ** 32)
    with loaded(nb, posm) as e:
        got = e.pair_counts_f64([2.0, 0.0, 1e6])
        assert got.dtype == np.int64 and got.tolist() == [total, 0, total]
        pts = posm[:1000, :3]
        assert e.pair_counts_at_f64(pts, [2.0, 0.0]).tolist() == [1000 * n, 1000]


# ---- 4: nothing else moves -----------------------------------------------------------------------------------------------------------------

def fourth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite_state() + e.hermite_tracers_state()


def sixth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite6_state() + e.hermite6_tracers_state()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def test_the_state_the_caches_and_the_tracers(nb):
    n, m = 257, 300
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    radii = P.radii_set(G + 1, 0.01, 5.0)
    with f64(nb, n, eps=0.05) as e, f64(nb, n, eps=0.05) as twin:
        for x in (e, twin):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
            x.hermite6_step(DT, 2); x.hermite_timescale(); x.hermite_tracers_timescale()   # both orders' caches, bodies and tracers
        before = fourth(e) + sixth(e)
        live = e.state(np.float64)[0]
        eq(e.pair_counts_f64(radii), P.pair_counts(live, radii), "the live state")
        eq(e.pair_counts_at_f64(tpos, radii), P.pair_counts_at(tpos[:, :3], live, radii), "the live state at points")
        for k, (a, c) in enumerate(zip(fourth(e) + sixth(e), before)):
            same(a, c, f"array {k} behind the calls")
        e.hermite6_step(DT, 1); twin.hermite6_step(DT, 1)          # and the steps behind them go on as the twin's
        for k, (a, c) in enumerate(zip(sixth(e), sixth(twin))):
            same(a, c, f"array {k} a sixth-order step later, against the twin")
        e.hermite_step(DT, 1); twin.hermite_step(DT, 1)
        for k, (a, c) in enumerate(zip(fourth(e), fourth(twin))):
            same(a, c, f"array {k} a fourth-order step later, against the twin")


@pytest.mark.parametrize("order", [4, 6])
def test_a_block_session_in_mid_frame_goes_on_as_its_twin(nb, order):
    n, m, levels = 257, 300, 8
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    radii = P.radii_set(G + 1, 0.01, 5.0)
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
        live = e.state(np.float64)[0]
        eq(e.pair_counts_f64(radii), P.pair_counts(live, radii), "mid-frame")
        eq(e.pair_counts_at_f64(tpos, radii), P.pair_counts_at(tpos[:, :3], live, radii), "mid-frame at points")
        for k, (a, c) in enumerate(zip(session(e), before)):
            same(a, c, f"array {k} behind the calls, in mid-frame")
        se, sw = advance(e), advance(twin)
        assert se == sw and se["synchronised"]
        for k, (a, c) in enumerate(zip(session(e), session(twin))):
            same(a, c, f"array {k} at the frame end, against the twin")


# ---- 5: the contract -----------------------------------------------------------------------------------------------------------------------

def test_errors(nb):
    E = nb._lib
    big = 2000
    p32, v32 = nb.ic_reference_box(big, 1000.0, seed=1)
    for kw, why in (({}, "fp32"), ({"precision": "f32_kahan"}, "fp32"), ({"precision": "f64", "i_begin": 0, "i_count": 1000}, "slice")):
        with nb.NBodyEngine(big, **kw) as e:
            if kw.get("precision") == "f64":
                e.set_state(p32.astype(np.float64), v32.astype(np.float64))
            else:
                e.set_state(p32, v32)
            for name, call in (("nbody_get_pair_counts_f64", lambda: e.pair_counts_f64([50.0])),
                               ("nbody_pair_counts_at_f64", lambda: e.pair_counts_at_f64(np.zeros((3, 3)), [50.0]))):
                msg = raises(nb, E.ERR_UNSUPPORTED, call)
                assert name in msg and why in msg, (kw, msg)
    n = 257
    posm = R.scene(f"gauss{n}")
    with f64(nb, n) as e:
        raises(nb, E.ERR_STATE, lambda: e.pair_counts_f64([0.4]))  # no particles set
        raises(nb, E.ERR_STATE, lambda: e.pair_counts_at_f64(np.zeros((3, 3)), [0.4]))
        e.set_state(np.array(posm), np.zeros((n, 4)))
        L, h = e._L, e._h
        A, At = L.nbody_get_pair_counts_f64, L.nbody_pair_counts_at_f64
        count = np.full(P.K_MAX + 1, -7, np.int64)
        out = count.ctypes.data_as(I64)
        pts = np.ascontiguousarray(posm[:, :3])
        good = np.full(P.K_MAX + 1, 0.4)
        rp = lambda a: a.ctypes.data_as(F64)
        for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf, 1e200):  # negative, NaN, infinite, a square that overflows
            for where in (0, 2):                                    # ... behind good radii too: nothing is written first
                radii = np.array([0.4, 0.2, 0.1]); radii[where] = bad
                assert A(h, rp(radii), 3, out) == E.ERR_INVALID, bad
                assert At(h, pts.ctypes.data, 24, n, rp(radii), 3, out) == E.ERR_INVALID, bad
            assert "nbody_get_pair_counts_f64" in raises(nb, E.ERR_INVALID, lambda: e.pair_counts_f64([0.4, bad]))
        for k in (0, -1, P.K_MAX + 1):                              # k outside 1 .. 64
            assert A(h, rp(good), k, out) == E.ERR_INVALID, k
            assert At(h, pts.ctypes.data, 24, n, rp(good), k, out) == E.ERR_INVALID, k
        assert A(h, None, 3, out) == E.ERR_INVALID                                                  # null radii,
        assert A(h, rp(good), 3, None) == E.ERR_INVALID                                             # null output
        assert At(h, None, 24, n, rp(good), 3, out) == E.ERR_INVALID                                # null points,
        assert At(h, pts.ctypes.data, 24, n, None, 3, out) == E.ERR_INVALID                         # null radii,
        assert At(h, pts.ctypes.data, 24, n, rp(good), 3, None) == E.ERR_INVALID                    # null output,
        assert At(h, pts.ctypes.data, 16, n, rp(good), 3, out) == E.ERR_INVALID                     # a stride < 24,
        assert At(h, pts.ctypes.data, 24, -1, rp(good), 3, out) == E.ERR_INVALID                    # n < 0
        e.step_begin()                                             # a step is open
        assert "nbody_get_pair_counts_f64" in raises(nb, E.ERR_STATE, lambda: e.pair_counts_f64([0.4]))
        assert At(h, pts.ctypes.data, 24, n, rp(good), 3, out) == E.ERR_STATE
        e.step_end(0.0)
        assert (count == -7).all()                                 # nothing written by any refusal
        assert At(h, pts.ctypes.data, 24, 0, rp(good), 3, out) == 0 and count.tolist() == [0] * 3 + [-7] * (P.K_MAX - 2)   # n == 0: zeros
        assert A(h, rp(good), P.K_MAX, out) == 0 and count[P.K_MAX] == -7                           # 64 equal radii: 64 equal answers
        assert count[:P.K_MAX].tolist() == [R.case(f"gauss{n}", 0.4)["summary"].links] * P.K_MAX


def test_histogram_and_correlation(nb):
    n, nr = 1000, 1500
    posm = R.scene(f"gauss{n}")
    edges = np.geomspace(0.05, 2.0, 9)
    randoms = np.random.default_rng(11).normal(0.0, 1.0, (nr, 3))
    with loaded(nb, posm) as e:
        dd = np.diff(P.pair_counts(posm, edges))
        eq(e.pair_histogram_f64(edges), dd, "the histogram")
        c = e.correlation_f64(edges, randoms)
        eq(c.dd, dd, "DD"); eq(c.dr, np.diff(P.pair_counts_at(randoms, posm, edges)), "DR")
        rposm = np.ones((nr, 4)); rposm[:, :3] = randoms
        eq(c.rr, np.diff(P.pair_counts(rposm, edges)), "RR")
        from parallelnbody_amd.engine import landy_szalay
        assert c.xi.tobytes() == landy_szalay(c.dd, c.dr, c.rr, n, nr).tobytes()
        assert (np.isnan(c.xi) == (c.rr == 0)).all()                # NaN where no random pair fell, and only there
        with pytest.raises(ValueError):
            e.pair_histogram_f64([1.0, 0.5])


def test_command_line_pairs_every(nb):
    """--pairs-every 2 over four frames prints two lines, and their values are pair_counts_f64()'s on the same state."""
    n, radii = 512, [2.0, 0.5, 8.0]
    cmd = [sys.executable, "-m", "parallelnbody_amd", "--precision", "f64", "--plummer", "--n", str(n), "--steps", "4", "--pairs-every", "2",
           "--pair-radii", ",".join(str(r) for r in radii)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines()]
    prs = [ln for ln in lines if "pairs" in ln]
    assert [ln["frame"] for ln in prs] == [2, 4] and len(lines) == 3
    posm, vel = nb.ic_plummer(n, G=1.0e4, seed=1)
    with nb.NBodyEngine(n, precision="f64", G=1.0e4) as e:
        e.set_state(posm, vel)
        for ln in prs:
            e.step(0.01, 2)
            assert ln["pairs"] == {"radii": radii, "counts": e.pair_counts_f64(radii).tolist()}
            assert ln["pairs"]["counts"][1] <= ln["pairs"]["counts"][0] <= ln["pairs"]["counts"][2]
