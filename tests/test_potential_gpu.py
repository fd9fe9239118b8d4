"""The gravitational potential: nbody_potential_at (at caller-given points), nbody_get_potentials (at the bodies, self excluded) and
nbody_energy_fast (1/2 sum m phi from them).

theta = 0 against numpy fp64 direct sums at the project's all-pairs tolerance; theta > 0 against tests/cpp/bh_pot_ref.c — the
reference's octree walked from arbitrary points with the potential's term, pinned by tests/test_bh_pot_ref.py — in every byte."""
import os

import numpy as np
import pytest

from bh_pot_ref import PotRef, direct_potential
from probe_scenes import GOLDEN, N_PROBES, TOL_ACC, bodies, probes_for

pytestmark = pytest.mark.gpu

G = 1.0e4
SLAB = 211968            # points per slab of partial rows at N = 20000 (probe_slab_points: 256 MiB / (79 chunks * 16 B), in whole 1024s)


@pytest.fixture(scope="module")
def pot_ref(tmp_path_factory):
    return PotRef(tmp_path_factory.mktemp("bh_pot_ref"))


_direct = {}


def direct_ref(n, pos, mass, pts, eps=0.0, skip_self=False):
    key = (n, pts.shape[0], eps, skip_self, pts.tobytes()[:64])
    if key not in _direct:
        ref = direct_potential(pos, mass, pts, eps=eps, skip_self=skip_self)
        ref.setflags(write=False)
        _direct[key] = ref
    return _direct[key]


def rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.where(ref != 0.0, np.abs(ref), 1.0)


# ---- theta = 0: potential_at --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,eps", [(2000, 777, 0.0), (2000, 1, 0.0), (2000, 64, 0.0), (2000, 65, 0.0), (257, 5000, 0.0), (1, 64, 0.0),
                                     (20000, 100, 0.0), (2000, 777, 0.05)])
def test_direct_sum_at_every_probe(nb, n, m, eps):
    posm, vel = bodies(nb, n)
    pos, mass = posm[:, :3], posm[:, 3]
    pts = probes_for(pos, m)
    ref = direct_ref(n, pos, mass, pts, eps=eps)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.potential_at(pts)
    assert got.shape == (m,) and got.dtype == np.float32 and np.isfinite(got).all() and np.isfinite(ref).all()
    err = rel(got, ref)
    print(f"potential_at theta=0 N={n} M={m} eps={eps}: max rel err {err.max():.3e}")
    assert err.max() < TOL_ACC, (n, m, int(err.argmax()), err.max())
    if m >= 60 and n >= 110:
        # probes 0-49 sit ON bodies: at eps == 0 the d == 0 pair is dropped (finite, and the bound above holds against a sum without it);
        # at eps > 0 they feel that body's -G m / eps
        if eps > 0.0:
            without = direct_potential(pos[1:], mass[1:], pts[:1], eps=eps)[0]
            assert got[0] - without == pytest.approx(-G * float(mass[0]) / eps, rel=1e-4)     # (body 0: the scene's heaviest)


def test_every_zero_mode_gives_the_default_contexts_bytes(nb):
    n, m = 2000, N_PROBES
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], m)
    out = []
    for zm in (nb._lib.ZERO_EXACT, nb._lib.ZERO_FLOOR, nb._lib.ZERO_SELECT):
        with nb.NBodyEngine(n, zero_mode=zm) as e:
            e.set_state(posm, vel)
            out.append((e.potential_at(pts).tobytes(), e.potentials().tobytes()))
    assert out[1] == out[0] and out[2] == out[0]


def test_bit_level_properties(nb):
    n, m = 2000, N_PROBES
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], m)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        e.step(0.01, 2)
        before = (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done())
        a = e.potential_at(pts)
        assert e.potential_at(pts).tobytes() == a.tobytes()                       # two calls
        h = m // 2
        assert np.concatenate([e.potential_at(pts[:h]), e.potential_at(pts[h:])]).tobytes() == a.tobytes()   # a point does not see the others
        p4 = np.zeros((m, 4), np.float32); p4[:, :3] = pts; p4[:, 3] = 123.0
        v16 = p4[:, :3]
        assert v16.strides == (16, 4) and e.potential_at(v16).tobytes() == a.tobytes()
        rec = np.zeros(m, nb.PARTICLE_DTYPE)
        rec["Mass"] = 7.0; rec["Velocity"] = 9.0; rec["Position"] = pts
        v40 = rec["Position"]
        assert v40.strides == (40, 4) and e.potential_at(v40).tobytes() == a.tobytes()
        # ... and on the output side: stride 40 into the records' Mass field, through the C entry point itself
        f = e._L.nbody_potential_at
        assert f(e._h, rec["Position"].ctypes.data, 40, m, rec["Mass"].ctypes.data, 40) == 0
        assert np.ascontiguousarray(rec["Mass"]).tobytes() == a.tobytes()
        assert (rec["Velocity"] == 9.0).all() and np.ascontiguousarray(rec["Position"]).tobytes() == pts.tobytes()
        out4 = np.full(m, 5.0, np.float32)
        assert f(e._h, p4.ctypes.data, 16, m, out4.ctypes.data, 4) == 0 and out4.tobytes() == a.tobytes()
        out4[:] = 5.0
        assert f(e._h, p4.ctypes.data, 16, 0, out4.ctypes.data, 4) == 0 and (out4 == 5.0).all()            # n == 0: a no-op
        assert (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done()) == before
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        e.step(0.01, 2)
        before = (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done(), str(e.bh_stats()))
        a = e.potential_at(pts)
        assert e.potential_at(pts).tobytes() == a.tobytes()
        assert np.concatenate([e.potential_at(pts[:h]), e.potential_at(pts[h:])]).tobytes() == a.tobytes()
        assert (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done(), str(e.bh_stats())) == before


# Many points: from ceil(M / 1024) * chunks >= 1024 on a workgroup takes 1024 points instead of 512, and points beyond what the staging
# area of partial rows holds go in a second slab.  N = 2000 (8 chunks): M = 135000 crosses the first threshold.  N = 20000 (79 chunks, slabs
# of 211968 points): M = 220000 crosses both.  Every sub-range asked for alone gives the bytes of the whole call.
@pytest.mark.parametrize("n,m,eps", [(2000, 135000, 0.0), (20000, 220000, 0.0), (20000, 220000, 0.05)])
def test_many_points_across_the_workgroup_shapes_and_the_slab_boundary(nb, n, m, eps):
    posm, vel = bodies(nb, n)
    pos, mass = posm[:, :3], posm[:, 3]
    pts = probes_for(pos, m)
    if m > SLAB:                                                  # on bodies and beside bodies on either side of the slab boundary
        pts[SLAB - 25:SLAB - 15] = pos[200:210]
        pts[SLAB + 15:SLAB + 25] = pos[210:220] + np.float32(1e-3)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.potential_at(pts)
        assert np.isfinite(got).all()
        ranges = [(0, 777), (1024 - 3, 1024 + 300), (131072 - 100, 131072 + 100), (m - 500, m), (m - 1, m)]
        if m > SLAB:
            ranges += [(SLAB - 300, SLAB + 300), (SLAB, SLAB + 1), (SLAB - 1, SLAB)]
        for a, b in ranges:
            assert e.potential_at(pts[a:b]).tobytes() == got[a:b].tobytes(), (a, b)
    sample = np.unique(np.concatenate([np.arange(0, 64), np.arange(SLAB - 40, SLAB + 40) % m, np.arange(m - 64, m),
                                       np.random.default_rng(9).integers(0, m, 300)]))
    err = rel(got[sample], direct_potential(pos, mass, pts[sample], eps=eps))
    print(f"potential_at theta=0 N={n} M={m} eps={eps}: max rel err on {sample.size} sampled points {err.max():.3e}")
    assert err.max() < TOL_ACC, (int(sample[err.argmax()]), err.max())


# ---- theta > 0: potential_at --------------------------------------------------------------------------------------------------------

def tree_probes(pos, root_com):
    """tests/test_field_gpu.py's point set: the 777 probes plus the root's CoM, a far point, a point on a body, one 1e-3 beside a body."""
    extra = np.array([root_com, (1e6, 1e6, 1e6), pos[123], pos[321] + np.float32(1e-3)], np.float32)
    return np.concatenate([probes_for(pos, N_PROBES), extra])


@pytest.mark.parametrize("n,eps,div_mode", [(2000, 0.0, 0), (3000, 0.0, 0), (5000, 0.0, 0), (20000, 0.0, 0),
                                            (2000, 0.05, 0), (20000, 0.05, 0), (2000, 0.0, 1)])
def test_walk_of_the_last_tree(nb, pot_ref, n, eps, div_mode):
    # the four build / walk families: LDS build, small system on the global walk, windows, lane walk with hop words
    posm, vel = bodies(nb, n)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    with nb.NBodyEngine(n, theta=1.0, eps=eps, bh_div_mode=div_mode) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        own = e.accelerations()
        stats = e.bh_stats()
        pts = tree_probes(pos, stats["root_com"])
        got = e.potential_at(pts)
        assert e.accelerations().tobytes() == own.tobytes() and e.bh_stats()["nodes"] == stats["nodes"]
    ref = pot_ref.walk(pos, mass, pts, 1.0, eps=eps, div_mode=div_mode)
    assert ref["root_com"].tobytes() == stats["root_com"].tobytes() and ref["nodes"] == stats["nodes"]
    assert got[N_PROBES] == 0.0 and ref["phi"][N_PROBES] == 0.0   # d == 0 at the root ends the walk there
    assert got.tobytes() == ref["phi"].tobytes(), (n, eps, div_mode, int((got != ref["phi"]).sum()))



def test_after_a_step_the_last_tree_is_that_of_the_positions_before_its_update(nb, pot_ref):
    n = 5000
    posm, vel = bodies(nb, n)
    with nb.NBodyEngine(n, theta=1.0) as twin:
        twin.set_state(posm, vel)
        twin.step(0.01, 1)
        x1 = twin.state()[0]
        root = twin.bh_stats()["root_com"]                        # the first tree's CoM: where the reference roots the second
    pts = tree_probes(np.ascontiguousarray(x1[:, :3]), root)
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        e.step(0.01, 2)
        got = e.potential_at(pts)
    ref = pot_ref.walk(x1[:, :3], x1[:, 3], pts, 1.0, root_origin=root)
    assert got.tobytes() == ref["phi"].tobytes()


# ---- potentials() -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("n", [1, 2, 257, 1000, 2000, 5000])
def test_potentials_are_the_direct_sum_without_the_body_itself(nb, n, eps):
    # (the sizes put the workgroup's own bodies against the tiles of 256 in every position: inside one tile, across two, a ragged last one)
    posm, vel = bodies(nb, n)
    pos, mass = posm[:, :3], posm[:, 3]
    ref = direct_ref(n, pos, mass, pos, eps=eps, skip_self=True)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.potentials()
        at = e.potential_at(pos)
    assert got.shape == (n,) and got.dtype == np.float32 and np.isfinite(got).all()
    if n == 1:
        assert got[0] == 0.0
        return
    err = rel(got, ref)
    print(f"potentials theta=0 N={n} eps={eps}: max rel err {err.max():.3e}")
    assert err.max() < TOL_ACC, (n, int(err.argmax()), err.max())
    if eps > 0.0:
        # the two modes differ where they must: a point ON body i feels body i, the body itself does not
        d = at.astype(np.float64) - got.astype(np.float64)
        want = -G * mass.astype(np.float64) / eps
        assert np.abs(d - want).max() <= 2 * TOL_ACC * np.abs(at).max()     # (both are within TOL_ACC of their own direct sums)
    else:
        assert at.tobytes() == got.tobytes()                      # eps == 0: d == 0 drops the same pair the index drops


def test_two_coincident_bodies_skip_each_other(nb):
    n = 1000
    posm, vel = bodies(nb, n)
    posm = posm.copy()
    posm[700, :3] = posm[3, :3]
    pos, mass = posm[:, :3], posm[:, 3]
    ref = direct_potential(pos, mass, pos, skip_self=True)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        got = e.potentials()
    assert np.isfinite(got).all() and rel(got, ref).max() < TOL_ACC
    assert rel(got[[3, 700]], ref[[3, 700]]).max() < TOL_ACC


@pytest.mark.parametrize("n", [2000, 5000, 20000])
def test_potentials_at_theta_1_are_the_walk_from_every_body(nb, pot_ref, n):
    posm, vel = bodies(nb, n)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    with nb.NBodyEngine(n, theta=1.0) as twin:
        twin.set_state(posm, vel)
        twin.step(0.01, 1)
        twin.compute_forces()
        want_acc, want_stats, want_state = twin.accelerations(), twin.bh_stats(), twin.state()
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        e.step(0.01, 1)
        x1 = e.state()[0]
        root = e.bh_stats()["root_com"]                           # the first tree's CoM roots the diagnostic tree too
        got = e.potentials()
        # the side effects are those of compute_forces(): the stored accelerations, the diagnostic tree; nothing else
        assert e.accelerations().tobytes() == want_acc.tobytes()
        st = e.bh_stats()
        assert st["root_com"].tobytes() == want_stats["root_com"].tobytes() and st["nodes"] == want_stats["nodes"]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e.state()[:2], want_state[:2])) and e.steps_done() == 1
        assert e.potentials().tobytes() == got.tobytes()
    ref = pot_ref.walk(x1[:, :3], x1[:, 3], x1[:, :3], 1.0, root_origin=root)
    assert ref["root_com"].tobytes() == st["root_com"].tobytes()
    assert got.tobytes() == ref["phi"].tobytes(), (n, int((got != ref["phi"]).sum()))


@pytest.mark.parametrize("theta,n", [(0.0, 2000), (1.0, 5000)])
@pytest.mark.parametrize("tracers", [False, True])
def test_calls_between_steps_change_no_trajectory(nb, theta, n, tracers):
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], N_PROBES)
    tr = pts[60:] if tracers else None
    out = []
    for ask in (False, True):
        with nb.NBodyEngine(n, theta=theta) as e:
            e.set_state(posm, vel)
            if tracers:
                e.set_tracers(tr)
            for _ in range(5):
                e.step(0.01, 1)
                if ask:
                    e.potentials(); e.energy_fast(); e.potential_at(pts)
            out.append((e.particles().tobytes() if theta == 0.0 else b"".join(a.tobytes() for a in e.state()[:2]), e.steps_done(),
                        b"".join(a.tobytes() for a in e.tracers()[:2]) if tracers else b""))
    assert out[0] == out[1]


# ---- energy_fast() ------------------------------------------------------------------------------------------------------------------

def _golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return np.ascontiguousarray(g["posm"], np.float32), np.ascontiguousarray(g["vel"], np.float32)


@pytest.mark.parametrize("name,eps,theta", [("refbox_n2000_seed1", 0.0, 0.0), ("plummer_n1024_seed1", 1.0, 0.0),
                                            ("refbox_n2000_seed1", 0.0, 1e-30)])
def test_energy_fast_against_the_oracle(nb, oracle, name, eps, theta):
    posm, vel = _golden(name)
    n = posm.shape[0]
    ke0, pe0 = oracle.energy_f64(posm[:, :3], vel[:, :3], posm[:, 3], eps=eps)
    with nb.NBodyEngine(n, eps=eps, theta=theta) as e:
        e.set_state(posm, vel)
        ke1, pe1 = e.energy()
        ke, pe = e.energy_fast()
        assert e.energy_fast() == (ke, pe)                        # identical bits every run
    print(f"energy_fast {name} eps={eps} theta={theta}: pe rel err {abs(pe - pe0) / abs(pe0):.3e}, ke rel diff {abs(ke - ke1) / abs(ke1):.3e}")
    assert abs(ke - ke1) <= 1e-12 * abs(ke1) and abs(ke - ke0) <= 1e-12 * abs(ke0)
    assert abs(pe1 - pe0) <= 1e-10 * abs(pe0)                     # the yardstick itself: energy()'s all-pairs potential
    assert abs(pe - pe0) < 2e-5 * abs(pe0)


def test_energy_fast_at_theta_1_is_half_the_sum_of_m_phi(nb, pot_ref):
    n = 5000
    posm, vel = bodies(nb, n)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        ke, pe = e.energy_fast()
        assert e.energy_fast() == (ke, pe)
        ke1, _ = e.energy()
    ref = pot_ref.walk(pos, mass, pos, 1.0)
    want = 0.5 * float(np.sum(mass.astype(np.float64) * ref["phi64"]))
    print(f"energy_fast theta=1 N={n}: pe {pe:.17g}, from bh_pot_ref {want:.17g}, rel diff {abs(pe - want) / abs(want):.3e}")
    assert abs(pe - want) <= 1e-12 * abs(want)                    # only the order of the final reduction differs
    assert abs(ke - ke1) <= 1e-12 * abs(ke1)


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def _three_calls(e, pts):
    return (lambda: e.potential_at(pts)), e.potentials, e.energy_fast


def test_errors(nb):
    n = 2000
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], 16)
    E = nb._lib
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError) as err:                 # no tree yet
            e.potential_at(pts)
        assert err.value.code == E.ERR_STATE and "nbody_compute_forces" in str(err.value)
        e.compute_forces()
        e.potential_at(pts)
        e.set_theta(0.5)
        with pytest.raises(nb.NBodyError) as err:                 # the tree is another angle's
            e.potential_at(pts)
        assert err.value.code == E.ERR_STATE
        e.potentials()                                            # builds its own tree ...
        e.potential_at(pts)                                       # ... which a query may walk
        out = np.zeros(16, np.float32)
        f = e._L.nbody_potential_at
        assert f(e._h, pts.ctypes.data, 8, 16, out.ctypes.data, 4) == E.ERR_INVALID
        assert f(e._h, pts.ctypes.data, 12, 16, out.ctypes.data, 3) == E.ERR_INVALID
        assert f(e._h, None, 12, 16, out.ctypes.data, 4) == E.ERR_INVALID
        assert f(e._h, pts.ctypes.data, 12, 16, None, 4) == E.ERR_INVALID
        assert f(e._h, pts.ctypes.data, 12, -1, out.ctypes.data, 4) == E.ERR_INVALID
        big = np.zeros(n, np.float32)
        assert e._L.nbody_get_potentials(e._h, None, 4) == E.ERR_INVALID
        assert e._L.nbody_get_potentials(e._h, big.ctypes.data, 3) == E.ERR_INVALID
        assert e._L.nbody_energy_fast(e._h, None, None) == 0      # either output may be NULL
    for kw in ({"precision": "f64"}, {"precision": "f32_kahan"}, {"i_begin": 0, "i_count": 1000}, {"devices": [0]}):
        with nb.NBodyEngine(n, **kw) as e:
            e.set_state(posm, vel)
            for call in _three_calls(e, pts):
                with pytest.raises(nb.NBodyError) as err:
                    call()
                assert err.value.code == E.ERR_UNSUPPORTED, kw


def test_a_last_tree_deeper_than_42_levels_answers_no_potential(nb):
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
            with pytest.raises(nb.NBodyError) as err:
                call()
            assert err.value.code == E.ERR_UNSUPPORTED and "deeper than 42 levels" in str(err.value)


# ---- command line -------------------------------------------------------------------------------------------------------------------

def test_fast_energy_flag_on_the_command_line(nb, tmp_path, capsys):
    import json
    from parallelnbody_amd.__main__ import main
    common = ["--n", "2000", "--size", "1000", "--dt", "0.01", "--steps", "4", "--energy-every", "2"]
    out = {}
    for flag in ("", "--fast-energy"):
        for theta in ("0", "1.0"):
            dump = str(tmp_path / f"p{flag}{theta}.npy")
            main(common + ["--theta", theta, "--dump-positions", dump] + ([flag] if flag else []))
            lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
            out[flag, theta] = ([l for l in lines if "potential" in l], np.load(dump))
    for theta in ("0", "1.0"):
        slow, fast = out["", theta], out["--fast-energy", theta]
        assert fast[1].tobytes() == slow[1].tobytes()             # the same trajectory with and without the flag
        assert [l["frame"] for l in fast[0]] == [2, 4] == [l["frame"] for l in slow[0]]
        for a, b in zip(slow[0], fast[0]):
            assert abs(b["kinetic"] - a["kinetic"]) <= 1e-12 * abs(a["kinetic"])
            if theta == "0":
                assert abs(b["potential"] - a["potential"]) <= 2e-5 * abs(a["potential"])
            else:                                                 # the energy of the opening rule's monopoles: another number
                assert np.isfinite(b["potential"]) and b["potential"] < 0.0 and b["potential"] != a["potential"]
