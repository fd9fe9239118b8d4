"""The fp64 group census — nbody_get_radius_counts_f64, nbody_radius_counts_at_f64, nbody_get_groups_f64 — on the device.

The yardstick is tests/groups_f64_ref.py: include/nbody.h's definitions in numpy, float64 — the linked pairs and a union-find, nothing of
the device's rounds.  d2 is formed without contraction, so numpy forms the same bits and every link is decided alike: degree, label,
members and every summary field but `rounds` are compared BYTE FOR BYTE at every size.  Nothing here is held to a tolerance.  `rounds`
is bounded where the issue of plain label propagation is at stake (the chains), and otherwise only tied to the pass counter."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import census_f64_ref as C
import groups_f64_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1e-3


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
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a != b).sum())} entries differ"


def loaded(nb, posm, **kw):
    e = f64(nb, len(posm), **kw)
    e.set_state(np.array(posm), np.zeros((len(posm), 4)))
    return e


def held(what, got, want):
    """a GroupsResult against the mirror's case, byte for byte; rounds is the device's own"""
    eq(got.degree, want["degree"], f"{what}: degree")
    eq(got.label, want["label"], f"{what}: label")
    eq(got.members, want["members"], f"{what}: members")
    s = got.summary
    assert R.Summary(s.groups, s.multiples, s.largest, s.largest_members, s.links) == want["summary"], (what, s, want["summary"])
    assert 1 <= s.rounds <= len(got.label)


# ---- 1: every size, byte for byte ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.GAUSS_SIZES)
def test_degree_label_members_and_summary_byte_for_byte(nb, n):
    posm = R.scene(f"gauss{n}")
    with loaded(nb, posm) as e:
        for radius in R.gauss_radii(n):
            want = R.case(f"gauss{n}", radius)
            got = e.groups_f64(radius)
            print(f"N = {n}, b = {radius}: {got.summary}")
            held(f"N = {n}, b = {radius}", got, want)
            again = e.groups_f64(radius)                            # the same bytes from a second call
            for a, b, name in zip(got[:3], again[:3], ("label", "members", "degree")):
                eq(a, b, f"N = {n}, b = {radius}: {name} of a second call")
            assert again.summary == got.summary
            eq(e.radius_counts_f64(radius), got.degree, f"N = {n}, b = {radius}: radius_counts_f64 against the degree")
            if n <= 4097:                                           # a point on a body counts that body
                eq(e.radius_counts_at_f64(posm[:, :3], radius), got.degree + 1, f"N = {n}, b = {radius}: counts at the bodies' own positions")


@pytest.mark.parametrize("m", R.POINT_COUNTS)
def test_counts_at_points_one_and_two_rows_per_lane(nb, m):
    n = 4097
    posm = R.scene(f"gauss{n}")
    points = np.random.default_rng(100 + m).normal(0.0, 1.0, (m, 3))
    points[0] = posm[n - 1, :3]                                     # on the one body of the last chunk
    with loaded(nb, posm) as e:
        for radius in (0.0, 0.2, 0.4, 50.0):
            want = R.counts_at(points, posm, radius)
            eq(e.radius_counts_at_f64(points, radius), want, f"M = {m}, b = {radius}")
            assert want[0] >= 1 and (radius < 50.0 or (want == n).all())
        assert e.radius_counts_at_f64(np.zeros((0, 3)), 0.2).shape == (0,)   # n == 0: NBODY_OK


def test_one_point_counts_what_mass_within_counts(nb):
    n = 1000
    posm = R.scene(f"gauss{n}")
    with loaded(nb, posm) as e:
        for c in (np.zeros(3), posm[17, :3], np.array([0.3, -0.2, 1.1])):
            radii = np.array([0.0, 0.05, 0.2, 0.4, 1.0, 2.5, 100.0])
            _, count = e.mass_within(c, radii)
            got = [int(e.radius_counts_at_f64(c[None, :], r)[0]) for r in radii]
            assert got == count.tolist() == [int(R.counts_at(c[None, :], posm, r)[0]) for r in radii]
            assert got[-1] == n and got[0] == int((c == posm[17, :3]).all())      # radius 0: the body the point sits on


# ---- 2: structure --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("permuted", "bitrev"))
def test_a_chain_of_4096_is_one_group_within_32_rounds(nb, kind):
    posm = R.scene(f"chain_{kind}")
    with loaded(nb, posm) as e:
        got = e.groups_f64(1.5)
        print(f"the {kind} chain: {got.summary.rounds} rounds on the device")
        held(f"chain {kind}", got, R.case(f"chain_{kind}", 1.5))
        assert (got.label == 0).all() and got.summary.groups == 1 and got.summary.largest == 0
        assert got.summary.rounds <= 32                             # twice the mirror's bound: plain propagation needs thousands


def test_a_lattice_at_and_just_below_its_spacing(nb):
    posm = R.scene("lattice")
    with loaded(nb, posm) as e:
        got = e.groups_f64(1.0)
        held("lattice, b = 1", got, R.case("lattice", 1.0))
        assert got.degree.max() == 6 and got.degree.min() == 3 and got.summary.groups == 1 and got.summary.links == 3 * 9 * 9 * 8
        got = e.groups_f64(0.99)
        held("lattice, b = 0.99", got, R.case("lattice", 0.99))
        assert got.summary.groups == 729 and got.summary.links == 0 and got.summary.rounds == 1 and (got.members == 1).all()


def test_all_bodies_on_one_point_at_radius_zero(nb):
    posm = R.scene("coincident")
    n = len(posm)
    with loaded(nb, posm) as e:
        got = e.groups_f64(0.0)
        held("coincident", got, R.case("coincident", 0.0))
        assert (got.degree == n - 1).all() and (got.label == 0).all() and got.summary.links == n * (n - 1) // 2


def test_nan_and_infinite_positions_are_alone_and_link_nothing(nb):
    posm = R.scene("nonfinite")
    with loaded(nb, posm) as e:
        got = e.groups_f64(0.4)
        held("nonfinite", got, R.case("nonfinite", 0.4))
        for b in R.NONFINITE_BODIES:
            assert got.degree[b] == 0 and got.label[b] == b and got.members[b] == 1
        clean = np.array(R.gauss_scene(300)); clean[list(R.NONFINITE_BODIES), :3] = 1e6 + 1e3 * np.arange(6)[:, None]
        with loaded(nb, clean) as f:                                # ... and nobody else's links moved: the same bodies far away
            far = f.groups_f64(0.4)
        eq(got.degree, far.degree, "degree with the six far away"); eq(got.label, far.label, "label with the six far away")
        eq(e.radius_counts_at_f64(posm[:, :3], 0.4), got.degree + np.isfinite(posm[:, :3]).all(1).astype(np.int32), "points that are not finite")


def test_two_clusters_whose_indices_interleave(nb):
    posm = R.scene("interleaved")
    with loaded(nb, posm) as e:
        got = e.groups_f64(1.0)
        held("interleaved", got, R.case("interleaved", 1.0))
        assert got.label.tolist() == [0, 1] * 300 and (got.members == 300).all() and got.summary.largest == 0
        t = e.group_table_f64(1.0)
        assert t["label"].tolist() == [0, 1] and t["count"].tolist() == [300, 300]
        assert abs(t["com"][1, 0] - t["com"][0, 0] - 100.0) < 0.05 and (t["r_rms"] < 0.2).all() and (t["sigma"] == 0.0).all()


# ---- 3: nothing else moves -----------------------------------------------------------------------------------------------------------------

def linking_length(posm):
    """twice the median distance to the nearest body: singles, multiples and a large group at once"""
    d2 = R.d2_block(posm[:, :3], posm[:, :3])
    np.fill_diagonal(d2, np.inf)
    return 2.0 * float(np.sqrt(np.median(d2.min(1))))


def passes(nb, e):
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]


def fourth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite_state() + e.hermite_tracers_state()


def sixth(e):
    return e.state(np.float64) + e.tracers_f64() + e.hermite6_state() + e.hermite6_tracers_state()


def test_the_pass_counters_the_state_the_caches_and_the_tracers(nb):
    n, m = 257, 300
    posm, vel, tpos, tvel = C.scene(nb, n, m)
    with f64(nb, n, eps=0.05, time_kernels=True) as e, f64(nb, n, eps=0.05, time_kernels=True) as twin:
        for x in (e, twin):
            x.set_state(posm, vel); x.set_tracers_f64(tpos, tvel)
            x.hermite6_step(DT, 2); x.hermite_timescale(); x.hermite_tracers_timescale()   # both orders' caches, bodies and tracers
        before = fourth(e) + sixth(e)
        live = e.state(np.float64)[0]
        b = linking_length(live)
        f0, u0 = passes(nb, e)
        eq(e.radius_counts_f64(b), R.groups(live, b)["degree"], "degree of the live state")
        assert passes(nb, e) == (f0 + 1, u0)                        # one pass
        e.radius_counts_at_f64(tpos, b)
        assert passes(nb, e) == (f0 + 2, u0)
        got = e.groups_f64(b)
        held("the live state", got, R.groups(live, b))
        assert got.summary.rounds >= 2 and passes(nb, e) == (f0 + 2 + got.summary.rounds, u0)   # summary.rounds passes
        assert e.groups_f64(0.0).summary.rounds == 1 and passes(nb, e) == (f0 + 3 + got.summary.rounds, u0)
        for k, (a, c) in enumerate(zip(fourth(e) + sixth(e), before)):
            eq(a, c, f"array {k} behind the calls")
        for k, (a, c) in enumerate(zip(fourth(e) + sixth(e), fourth(twin) + sixth(twin))):
            eq(a, c, f"array {k} against the twin")
        e.hermite6_step(DT, 1); twin.hermite6_step(DT, 1)          # and the steps behind them go on as the twin's
        for k, (a, c) in enumerate(zip(sixth(e), sixth(twin))):
            eq(a, c, f"array {k} a sixth-order step later, against the twin")
        e.hermite_step(DT, 1); twin.hermite_step(DT, 1)
        for k, (a, c) in enumerate(zip(fourth(e), fourth(twin))):
            eq(a, c, f"array {k} a fourth-order step later, against the twin")


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
        live = e.state(np.float64)[0]                              # the groups describe each body where it is: the live state's
        b = linking_length(live)
        got = e.groups_f64(b)
        e.radius_counts_f64(b); e.radius_counts_at_f64(tpos, b)
        for k, (a, c) in enumerate(zip(session(e), before)):
            eq(a, c, f"array {k} behind the calls, in mid-frame")
        held("mid-frame", got, R.groups(live, b))
        se, sw = advance(e), advance(twin)
        assert se == sw and se["synchronised"]
        for k, (a, c) in enumerate(zip(session(e), session(twin))):
            eq(a, c, f"array {k} at the frame end, against the twin")


# ---- 4: the contract -----------------------------------------------------------------------------------------------------------------------

NAMES = ("nbody_get_radius_counts_f64", "nbody_radius_counts_at_f64", "nbody_get_groups_f64")


def lambdas(e, radius=0.4):
    return (lambda: e.radius_counts_f64(radius)), (lambda: e.radius_counts_at_f64(np.zeros((3, 3)), radius)), (lambda: e.groups_f64(radius))


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
            for name, call in zip(NAMES, lambdas(e, 50.0)):
                msg = raises(nb, E.ERR_UNSUPPORTED, call)
                assert name in msg and why in msg, (kw, msg)
    n = 257
    posm = R.scene(f"gauss{n}")
    with f64(nb, n) as e:
        for call in lambdas(e):                                    # no particles set
            raises(nb, E.ERR_STATE, call)
        e.set_state(np.array(posm), np.zeros((n, 4)))
        L, h = e._L, e._h
        A, P, G = L.nbody_get_radius_counts_f64, L.nbody_radius_counts_at_f64, L.nbody_get_groups_f64
        label, members, degree, count = (np.full(n, -7, np.int32) for _ in range(4))
        s = E.Groups(-7, -7, -7, -7, -7, -7, -7)
        pts = np.ascontiguousarray(posm[:, :3])
        for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf, 1e200):  # negative, NaN, infinite, a square that overflows
            assert A(h, bad, count.ctypes.data) == E.ERR_INVALID, bad
            assert P(h, pts.ctypes.data, 24, n, bad, count.ctypes.data) == E.ERR_INVALID, bad
            assert G(h, bad, label.ctypes.data, members.ctypes.data, degree.ctypes.data, ctypes.byref(s)) == E.ERR_INVALID, bad
            assert "nbody_get_groups_f64" in raises(nb, E.ERR_INVALID, lambda: e.groups_f64(bad))
        assert G(h, 0.4, None, None, None, None) == E.ERR_INVALID                                   # every output null
        assert A(h, 0.4, None) == E.ERR_INVALID
        assert P(h, None, 24, n, 0.4, count.ctypes.data) == E.ERR_INVALID                            # null points,
        assert P(h, pts.ctypes.data, 24, n, 0.4, None) == E.ERR_INVALID                              # null output,
        assert P(h, pts.ctypes.data, 16, n, 0.4, count.ctypes.data) == E.ERR_INVALID                 # a stride < 24,
        assert P(h, pts.ctypes.data, 24, -1, 0.4, count.ctypes.data) == E.ERR_INVALID                # n < 0
        e.step_begin()                                             # a step is open
        for name, call in zip(NAMES, lambdas(e)):
            assert name in raises(nb, E.ERR_STATE, call)
        assert G(h, 0.4, label.ctypes.data, members.ctypes.data, degree.ctypes.data, ctypes.byref(s)) == E.ERR_STATE
        e.step_end(0.0)
        for a in (label, members, degree, count):                  # nothing written by any refusal
            assert (a == -7).all()
        assert [getattr(s, f) for f, _ in E.Groups._fields_] == [-7] * 7
        want = R.case(f"gauss{n}", 0.4)
        assert P(h, pts.ctypes.data, 24, 0, 0.4, count.ctypes.data) == 0 and (count == -7).all()     # n == 0: NBODY_OK, nothing written
        assert G(h, 0.4, label.ctypes.data, None, None, None) == 0 and (members == -7).all(); eq(label, want["label"], "the label alone")
        assert G(h, 0.4, None, members.ctypes.data, None, None) == 0 and (degree == -7).all(); eq(members, want["members"], "members alone")
        assert G(h, 0.4, None, None, degree.ctypes.data, None) == 0 and s.groups == -7; eq(degree, want["degree"], "the degree alone")
        assert G(h, 0.4, None, None, None, ctypes.byref(s)) == 0 and s.reserved == 0
        assert R.Summary(s.groups, s.multiples, s.largest, s.largest_members, s.links) == want["summary"]
        assert G(h, -0.0, None, None, degree.ctypes.data, None) == 0 and (degree == 0).all()        # -0.0 is >= 0


def test_command_line_groups_every(nb):
    """--groups-every 2 over four frames prints two lines, and their values are groups_f64()'s on the same state."""
    n, b = 512, 2.0
    cmd = [sys.executable, "-m", "parallelnbody_amd", "--precision", "f64", "--plummer", "--n", str(n), "--steps", "4", "--groups-every", "2",
           "--linking-length", str(b)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines()]
    grp = [ln for ln in lines if "groups" in ln]
    assert [ln["frame"] for ln in grp] == [2, 4] and len(lines) == 3
    posm, vel = nb.ic_plummer(n, G=1.0e4, seed=1)
    with nb.NBodyEngine(n, precision="f64", G=1.0e4) as e:
        e.set_state(posm, vel)
        for ln in grp:
            e.step(0.01, 2)
            s = e.groups_f64(b).summary
            assert ln["groups"] == {"linking_length": b, "groups": s.groups, "multiples": s.multiples, "largest": s.largest,
                                    "largest_members": s.largest_members, "links": s.links}
            assert 1 <= s.groups <= n and s.links == int(e.radius_counts_f64(b).sum()) // 2
    bad = subprocess.run([sys.executable, "-m", "parallelnbody_amd", "--n", "64", "--steps", "1", "--groups-every", "1", "--linking-length", "1"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert bad.returncode == 2 and "--groups-every needs --precision f64" in bad.stderr
