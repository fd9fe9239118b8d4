"""The fp64 radial census — nbody_radial_order_f64, nbody_lagrange_radii_f64 — on the device.

The yardstick is tests/radial_f64_ref.py: include/nbody.h's definitions in numpy, float64.  The order is a total order and the cumulative
mass a fixed sequence of fp64 additions, so the order, the sorted d2 and mass_cum are compared BYTE FOR BYTE at every size, and the
Lagrangian rows byte for byte with the selection applied to the device's own mass_cum.  Against long double a row's body is compared only
behind the GAP CONDITION — gap >= 4 n 2^-53 on every (scene, fraction) pair, none left out; tests/test_radial_f64_ref.py shows the
scenes orders of magnitude above it on the CPU.  Nothing here is held to a tolerance."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import census_f64_ref as C
import radial_f64_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1e-3
ZERO = np.zeros(3)


def f64(nb, n, **kw):
    return nb.NBodyEngine(n, precision="f64", **kw)


def raises(nb, code, call):
    with pytest.raises(nb.NBodyError) as er:
        call()
    assert er.value.code == code, (er.value.code, str(er.value))
    return str(er.value)


def eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def rows_of(g):
    """a LagrangeResult's columns as the records of struct nbody_lagrange"""
    rows = np.zeros(g.fraction.shape[0], R.ROW)
    for name in R.ROW.names:
        rows[name] = getattr(g, name)
    return rows


def order_held(what, got, posm, centre):
    """(order, d2, mass_cum, n_finite) of the device against the numpy mirror, byte for byte (a NaN's payload is left open)"""
    order, d2s, cum, n_finite, _ = R.radial(posm, centre)
    assert got[3] == n_finite, (what, got[3], n_finite)
    eq(got[0], order, f"{what}: order")
    eq(got[1][:n_finite], d2s[:n_finite], f"{what}: d2")
    assert (got[1][n_finite:] == np.inf).sum() == (d2s[n_finite:] == np.inf).sum() and np.isnan(got[1][n_finite:]).sum() == np.isnan(d2s).sum()
    assert (np.isnan(got[1]) == np.isnan(d2s)).all()
    eq(got[2], cum, f"{what}: mass_cum")
    return order, d2s, cum, n_finite


def rows_held(what, g, got, fractions):
    """the rows against the selection applied to the device's own mass_cum, byte for byte"""
    want, total = R.select(got[0], got[1], got[2], fractions)
    assert g.total_mass == total == got[2][-1]
    eq(rows_of(g), want, f"{what}: rows")


# ---- 1: every size, byte for byte ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SIZES)
def test_order_cumulative_mass_and_rows_byte_for_byte(nb, n):
    c = R.gauss_case(n)
    with f64(nb, n) as e:
        e.set_state(c["posm"], c["vel"])
        got = e.radial_order_f64(R.CENTRE)
        assert got[0].dtype == np.int32 and got[1].dtype == got[2].dtype == np.float64
        eq(got[0], c["order"], "order"); eq(got[1], c["d2"], "d2"); eq(got[2], c["cum"], "mass_cum")
        assert got[3] == c["n_finite"] == n
        g = e.lagrange_f64(R.FRACTIONS, R.CENTRE)
        rows_held(f"N = {n}", g, got, R.FRACTIONS)
        eq(rows_of(g), c["rows"], "rows against the mirror's")
        # against long double: the gap on every fraction first, then the same body
        print(f"N = {n}: smallest gap {c['gap'].min():.3e}, bound {R.gap_bound(n):.3e}")
        assert (c["gap"] >= R.gap_bound(n)).all()
        assert (g.count == c["p_ld"] + 1).all() and (g.body == c["order"][c["p_ld"]]).all()
        again, g2 = e.radial_order_f64(R.CENTRE), e.lagrange_f64(R.FRACTIONS, R.CENTRE)   # the same bytes from two calls
        for a, b in zip(got[:3], again[:3]):
            eq(a, b, "a second call")
        eq(rows_of(g2), rows_of(g), "a second call's rows")


# ---- 2: keys of every kind ---------------------------------------------------------------------------------------------------------------

def test_distances_from_zero_through_subnormals_to_1e300(nb):
    posm = R.wide_scene()
    d2 = R.d2_of(posm[:, :3], ZERO)
    key = d2.view(np.uint64)
    assert d2.min() == 0.0 and ((d2 > 0.0) & (d2 < 2.3e-308)).sum() >= 20 and d2.max() > 1e299 and np.isfinite(d2).all()
    for d in range(8):                                             # every digit of the key has more than one value in use
        assert np.unique((key >> np.uint64(8 * d)) & np.uint64(0xFF)).size > 1
    with f64(nb, posm.shape[0]) as e:
        e.set_state(posm, np.zeros_like(posm))
        got = e.radial_order_f64(ZERO)
        order_held("the wide scene", got, posm, ZERO)
        rows_held("the wide scene", e.lagrange_f64(R.FRACTIONS, ZERO), got, R.FRACTIONS)


def test_a_lattice_has_thousands_of_equal_distances_across_tiles(nb):
    posm = R.lattice_scene()
    n = posm.shape[0]
    d2 = R.d2_of(posm[:, :3], ZERO)
    assert n > 2 * 4096 and np.unique(d2).size < n // 20           # runs of equal keys, far longer than a tile's share
    with f64(nb, n) as e:
        e.set_state(posm, np.zeros_like(posm))
        got = e.radial_order_f64(ZERO)
        order, d2s, _, _ = order_held("the lattice", got, posm, ZERO)
        same = d2s[1:] == d2s[:-1]
        assert (np.diff(order.astype(np.int64))[same] > 0).all()    # the lowest index first inside every run
        rows_held("the lattice", e.lagrange_f64(R.FRACTIONS, ZERO), got, R.FRACTIONS)


def test_all_bodies_on_the_centre_keep_their_order(nb):
    n = 5000
    posm = np.zeros((n, 4)); posm[:, :3] = (0.5, -2.0, 3.0); posm[:, 3] = np.random.default_rng(2).uniform(0.5, 1.5, n) / n
    with f64(nb, n) as e:
        e.set_state(posm, np.zeros_like(posm))
        got = e.radial_order_f64((0.5, -2.0, 3.0))
        order_held("all on the centre", got, posm, np.array([0.5, -2.0, 3.0]))
        assert (got[0] == np.arange(n)).all() and (got[1] == 0.0).all() and got[3] == n


def test_a_nan_and_an_infinity_come_last_and_add_nothing(nb):
    c = R.gauss_case(4097)
    posm = c["posm"].copy()
    posm[100, 1] = np.nan; posm[4000, 2] = np.inf; posm[7, 0] = -np.inf; posm[4096, 0] = np.nan
    with f64(nb, 4097) as e:
        e.set_state(posm, c["vel"])
        got = e.radial_order_f64(R.CENTRE)
        order_held("a NaN and an infinity", got, posm, R.CENTRE)
        assert got[3] == 4093 and got[0][-4:].tolist() == [7, 4000, 100, 4096]      # +inf in index order, then NaN in index order
        assert np.isinf(got[1][-4:-2]).all() and np.isnan(got[1][-2:]).all()
        assert (got[2][-5:] == got[2][-5]).all()                   # they add nothing
        g = e.lagrange_f64((0.5, 1.0), R.CENTRE)
        rows_held("a NaN and an infinity", g, got, (0.5, 1.0))
        assert g.count[1] == 4093 and g.body[1] == got[0][4092] and g.total_mass == got[2][4092]


# ---- 3: mass_within sees the same distances --------------------------------------------------------------------------------------------

def test_mass_within_counts_the_sorted_distances(nb):
    c = R.gauss_case(4097)
    with f64(nb, 4097) as e:
        e.set_state(c["posm"], c["vel"])
        _, d2s, _, _ = e.radial_order_f64(R.CENTRE)
        g = e.lagrange_f64(R.FRACTIONS, R.CENTRE)
        radii = np.concatenate((g.radius, [0.0, 0.5, 1.0, float(np.sqrt(d2s[-1])), 10.0]))
        assert radii.shape[0] >= 12
        _, count = e.mass_within(R.CENTRE, radii)
        assert count.tolist() == np.searchsorted(d2s, radii * radii, "right").tolist()
        # a row's r2 is d2 of its body: exact where sqrt(r2)^2 rounds back to it, and always through r2 itself
        for q in range(len(R.FRACTIONS)):
            assert np.searchsorted(d2s, g.r2[q], "right") >= g.count[q] and d2s[g.count[q] - 1] == g.r2[q]
            assert g.radius[q] == np.sqrt(g.r2[q])


# ---- 4: the selection ---------------------------------------------------------------------------------------------------------------------

def test_the_dyadic_tie_full_mass_shuffled_fractions_and_k(nb):
    posm = R.dyadic_scene()
    with f64(nb, 1024) as e:
        e.set_state(posm, np.zeros_like(posm))
        got = e.radial_order_f64(ZERO)
        order_held("dyadic masses", got, posm, ZERO)
        assert (got[2] == np.arange(1, 1025) * 2.0 ** -10).all()
        g = e.lagrange_f64((0.5, 1.0, 2.0 ** -10), ZERO)
        assert g.count.tolist() == [512, 1024, 1] and g.mass.tolist() == [0.5, 1.0, 2.0 ** -10] and g.total_mass == 1.0
        assert g.body.tolist() == [got[0][511], got[0][1023], got[0][0]]
    c = R.gauss_case(4097)
    posm = c["posm"].copy()
    last = c["order"][-3:]
    posm[last, 3] = 0.0                                            # the three outermost bodies are massless
    with f64(nb, 4097) as e:
        e.set_state(posm, c["vel"])
        got = e.radial_order_f64(R.CENTRE)
        order_held("massless outer bodies", got, posm, R.CENTRE)
        one = e.lagrange_f64((1.0,), R.CENTRE)                     # k = 1; f = 1 selects the last position that adds mass
        assert one.count[0] == 4097 - 3 and one.body[0] == c["order"][-4] and one.mass[0] == one.total_mass == got[2][-1]
        rows_held("k = 1", one, got, (1.0,))
        f64s = np.random.default_rng(8).uniform(0.0, 1.0, 64); f64s[f64s == 0.0] = 1.0; f64s[5] = 1.0
        full = e.lagrange_f64(f64s, R.CENTRE)                      # k = 64
        rows_held("k = 64", full, got, f64s)
        perm = np.random.default_rng(9).permutation(64)
        shuffled = e.lagrange_f64(f64s[perm], R.CENTRE)            # a row depends neither on the other fractions nor on their order
        eq(rows_of(shuffled), rows_of(full)[perm], "shuffled fractions")
        for q in (0, 17, 63):
            eq(rows_of(e.lagrange_f64(f64s[q:q + 1], R.CENTRE)), rows_of(full)[q:q + 1], "a fraction alone")


def test_no_mass_and_no_finite_body_give_empty_rows(nb):
    c = R.gauss_case(257)
    none = np.zeros(2, R.ROW); none["fraction"] = (0.5, 1.0); none["r2"] = none["radius"] = none["mass"] = np.nan; none["body"] = -1
    posm = c["posm"].copy(); posm[:, 3] = 0.0
    with f64(nb, 257) as e:
        e.set_state(posm, c["vel"])
        g = e.lagrange_f64((0.5, 1.0), R.CENTRE)                   # NBODY_OK
        assert g.total_mass == 0.0 and g.body.tolist() == [-1, -1] and g.count.tolist() == [0, 0]
        assert np.isnan(g.r2).all() and np.isnan(g.radius).all() and np.isnan(g.mass).all() and g.fraction.tolist() == [0.5, 1.0]
        assert e.radial_order_f64(R.CENTRE)[3] == 257
    posm = c["posm"].copy(); posm[:, 0] = np.nan; posm[::2, 0] = np.inf
    with f64(nb, 257) as e:
        e.set_state(posm, c["vel"])
        got = e.radial_order_f64(R.CENTRE)
        order_held("no finite body", got, posm, R.CENTRE)
        assert got[3] == 0 and (got[2] == 0.0).all()
        g = e.lagrange_f64((0.5, 1.0), R.CENTRE)
        assert g.total_mass == 0.0 and g.body.tolist() == [-1, -1] and g.count.tolist() == [0, 0] and np.isnan(g.r2).all()
    posm = c["posm"].copy(); posm[:, 3] = -posm[:, 3]              # a negative total
    with f64(nb, 257) as e:
        e.set_state(posm, c["vel"])
        g = e.lagrange_f64((0.5, 1.0), R.CENTRE)
        assert g.total_mass < 0.0 and g.body.tolist() == [-1, -1] and g.count.tolist() == [0, 0]


# ---- 5: nothing else moves ---------------------------------------------------------------------------------------------------------------

def two_calls(e):
    return e.radial_order_f64(R.CENTRE), e.lagrange_f64(R.FRACTIONS, R.CENTRE), e.lagrange_f64()


def passes(nb, e):
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]


def fourth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite_state() + e.hermite_tracers_state()


def sixth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite6_state() + e.hermite6_tracers_state()


def test_the_state_the_caches_and_the_tracers_stay(nb):
    n, m = 257, 300
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    with f64(nb, n, eps=0.05, time_kernels=True) as e, f64(nb, n, eps=0.05, time_kernels=True) as twin:
        for x in (e, twin):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
            x.hermite6_step(DT, 2); x.hermite_timescale(); x.hermite_tracers_timescale()   # both orders' caches, bodies and tracers
        before = fourth(e) + sixth(e)
        p0 = passes(nb, e)
        got = e.radial_order_f64(R.CENTRE)
        e.lagrange_f64(R.FRACTIONS, R.CENTRE)
        assert passes(nb, e) == p0                                 # no pair pass: neither timer counts it
        e.lagrange_f64()                                           # (centre=None is core_f64's pass, which counts as before)
        assert got[0].shape == (n,) and sorted(got[0].tolist()) == list(range(n))          # tracers are never listed
        for k, (a, b) in enumerate(zip(fourth(e) + sixth(e), before)):
            eq(a, b, f"array {k} behind the calls")
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
        got = two_calls(e)
        for k, (a, b) in enumerate(zip(session(e), before)):
            eq(a, b, f"array {k} behind the calls, in mid-frame")
        p, _, _ = e.state(np.float64)                              # the order describes each body where it is: the live state's
        order_held("mid-frame", got[0], p, R.CENTRE)
        se, sw = advance(e), advance(twin)
        assert se == sw and se["synchronised"]
        for k, (a, b) in enumerate(zip(session(e), session(twin))):
            eq(a, b, f"array {k} at the frame end, against the twin")


# ---- 6: the contract ---------------------------------------------------------------------------------------------------------------------

NAMES = ("nbody_radial_order_f64", "nbody_lagrange_radii_f64")


def lambdas(e):
    return (lambda: e.radial_order_f64(R.CENTRE)), (lambda: e.lagrange_f64(R.FRACTIONS, R.CENTRE))


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
            for name, call in zip(NAMES, lambdas(e)):
                msg = raises(nb, E.ERR_UNSUPPORTED, call)
                assert name in msg and why in msg, (kw, msg)
    c = R.gauss_case(257)
    n = 257
    with f64(nb, n) as e:
        for call in lambdas(e):                                    # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(c["posm"], c["vel"])
        L, h = e._L, e._h
        O, G = L.nbody_radial_order_f64, L.nbody_lagrange_radii_f64
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        centre, fr = R.CENTRE.copy(), np.array(R.FRACTIONS)
        order = np.full(n, -7, np.int32); d2 = np.full(n, -7.0); cum = np.full(n, -7.0); nf = ctypes.c_int32(-7)
        rows = (E.Lagrange * 64)(); total = ctypes.c_double(-7.0)
        assert O(h, None, order.ctypes.data, d2.ctypes.data, cum.ctypes.data, ctypes.byref(nf)) == E.ERR_INVALID      # a null centre
        assert O(h, dp(centre), None, None, None, None) == E.ERR_INVALID                                              # every output null
        for bad in (np.nan, np.inf, -np.inf):                      # a centre that is not finite
            c3 = centre.copy(); c3[1] = bad
            assert O(h, dp(c3), order.ctypes.data, d2.ctypes.data, cum.ctypes.data, ctypes.byref(nf)) == E.ERR_INVALID
            assert G(h, dp(c3), dp(fr), 9, rows, ctypes.byref(total)) == E.ERR_INVALID
        assert G(h, None, dp(fr), 9, rows, ctypes.byref(total)) == E.ERR_INVALID                                      # null centre,
        assert G(h, dp(centre), None, 9, rows, ctypes.byref(total)) == E.ERR_INVALID                                  # fractions,
        assert G(h, dp(centre), dp(fr), 9, None, ctypes.byref(total)) == E.ERR_INVALID                                # rows
        f65 = np.full(65, 0.5)
        for k in (0, -1, 65, 1 << 20):                             # k outside 1 .. 64
            assert G(h, dp(centre), dp(f65), k, rows, ctypes.byref(total)) == E.ERR_INVALID
        for bad in (0.0, -0.5, 1.0000000000000002, 2.0, np.nan, np.inf):   # a fraction outside (0, 1]
            fb = fr.copy(); fb[4] = bad
            assert G(h, dp(centre), dp(fb), 9, rows, ctypes.byref(total)) == E.ERR_INVALID
            assert "nbody_lagrange_radii_f64" in raises(nb, E.ERR_INVALID, lambda: e.lagrange_f64(fb, R.CENTRE))
        assert (order == -7).all() and (d2 == -7.0).all() and (cum == -7.0).all() and nf.value == -7 and total.value == -7.0   # nothing written
        want = e.radial_order_f64(R.CENTRE)
        assert O(h, dp(centre), order.ctypes.data, None, None, None) == 0 and (d2 == -7.0).all(); eq(order, want[0], "the order alone")
        assert O(h, dp(centre), None, d2.ctypes.data, None, None) == 0 and (cum == -7.0).all(); eq(d2, want[1], "d2 alone")
        assert O(h, dp(centre), None, None, cum.ctypes.data, None) == 0 and nf.value == -7; eq(cum, want[2], "mass_cum alone")
        assert O(h, dp(centre), None, None, None, ctypes.byref(nf)) == 0 and nf.value == n
        assert G(h, dp(centre), dp(fr), 9, rows, None) == 0                                                           # total_mass may be null
        eq(np.frombuffer(rows, R.ROW)[:9], c["rows"], "rows without the total")
        assert G(h, dp(centre), dp(np.array([1.0])), 1, rows, ctypes.byref(total)) == 0 and total.value == c["total"]
        e.step_begin()                                             # a step is open
        for name, call in zip(NAMES, lambdas(e)):
            assert name in raises(nb, E.ERR_STATE, call)
        e.step_end(0.0)
        for call in lambdas(e):
            call()


def test_the_default_centre_is_the_density_centre(nb):
    n = 1000
    posm, vel, _, _ = C.scene(nb, n, 25)
    with f64(nb, n) as e:
        e.set_state(posm, vel)
        core = e.core_f64(6)
        assert core.used == n
        g, at = e.lagrange_f64(), e.lagrange_f64(R.FRACTIONS, core.centre)
        eq(g.centre, core.centre, "the centre used"); eq(rows_of(g), rows_of(at), "rows about the density centre")
        assert g.total_mass == at.total_mass and (np.diff(g.radius) > 0).all()
        eq(rows_of(e.lagrange_f64(k=8)), rows_of(e.lagrange_f64(R.FRACTIONS, e.core_f64(8).centre)), "k = 8")
        prof = e.radial_profile_f64()                              # the shells end at the rows
        assert prof.count.sum() == g.count[-1] and (np.cumsum(prof.count) == g.count).all() and (prof.r_out == g.radius).all()
        order, _, cum, _ = e.radial_order_f64(core.centre)
        assert abs(prof.mass.sum() - g.mass[-1]) <= 1e-13 * g.total_mass and (prof.density > 0).all() and np.isfinite(prof.beta).all()
    lone = np.zeros((1, 4)); lone[0] = (3.0, 4.0, 0.0, 2.0)         # one body: no density, used == 0 — the centre of mass instead
    with f64(nb, 1) as e:
        e.set_state(lone, np.zeros((1, 4)))
        g = e.lagrange_f64((0.5,))
        assert g.centre.tolist() == [3.0, 4.0, 0.0] and g.count.tolist() == [1] and g.r2.tolist() == [0.0] and g.mass.tolist() == [2.0]


def test_command_line_lagrange_every(nb):
    """--lagrange-every 2 over four frames prints two lines, and their values are lagrange_f64()'s on the same state."""
    n = 512
    cmd = [sys.executable, "-m", "parallelnbody_amd", "--precision", "f64", "--plummer", "--n", str(n), "--steps", "4", "--lagrange-every", "2",
           "--lagrange-fractions", "0.1,0.5,0.9", "--core-k", "5"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines()]
    lag = [ln for ln in lines if "lagrange" in ln]
    assert [ln["frame"] for ln in lag] == [2, 4] and len(lines) == 3
    posm, vel = nb.ic_plummer(n, G=1.0e4, seed=1)
    with nb.NBodyEngine(n, precision="f64", G=1.0e4) as e:
        e.set_state(posm, vel)
        for ln in lag:
            e.step(0.01, 2)
            g = e.lagrange_f64((0.1, 0.5, 0.9), k=5)
            assert ln["lagrange"] == {"centre": [float(x) for x in g.centre], "total_mass": g.total_mass, "fractions": [0.1, 0.5, 0.9],
                                      "radii": [float(r) for r in g.radius], "bodies": [int(b) for b in g.body],
                                      "counts": [int(c) for c in g.count]}
            assert g.count[0] > 0 and g.radius[0] < g.radius[1] < g.radius[2]
    bad = subprocess.run([sys.executable, "-m", "parallelnbody_amd", "--n", "64", "--steps", "1", "--lagrange-every", "1"], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert bad.returncode == 2 and "--lagrange-every needs --precision f64" in bad.stderr
