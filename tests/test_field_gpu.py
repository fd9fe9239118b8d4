"""nbody_field_at: the acceleration the bodies exert on massless points the caller names.

theta = 0 against the oracle's direct sum with the points appended as zero-mass rows (they change no body's row, and a point's row is
the direct sum over the bodies) at the project's all-pairs tolerance; theta > 0 against tests/cpp/bh_probe_ref.c — the reference's
octree walked from arbitrary points, pinned to the oracle by tests/test_bh_probe_ref.py — in every bit."""
import numpy as np
import pytest

from bh_probe_ref import ProbeRef
from conftest import rel_err
from probe_scenes import N_PROBES, TOL_ACC, bodies, direct_at, probes_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_ref(tmp_path_factory):
    return ProbeRef(tmp_path_factory.mktemp("bh_probe_ref"))


_direct = {}


def direct_ref(oracle, n, pos, mass, pts, eps=0.0):
    key = (n, pts.shape[0], eps, pts.tobytes()[:64])
    if key not in _direct:
        ref = direct_at(oracle, pos, mass, pts, eps=eps)
        ref.setflags(write=False)
        _direct[key] = ref
    return _direct[key]


# ---- theta = 0 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(2000, 777), (2000, 1), (2000, 63), (2000, 64), (2000, 65), (257, 5000), (1, 64), (20000, 100)])
def test_direct_sum_at_every_probe(nb, oracle, n, m):
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], m)
    ref = direct_ref(oracle, n, posm[:, :3], posm[:, 3], pts)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        got = e.field_at(pts)
    assert got.shape == (m, 3) and np.isfinite(got).all() and np.isfinite(ref).all()
    err = rel_err(got, ref)
    print(f"field_at theta=0 N={n} M={m}: max rel err {err.max():.3e}")
    assert err.max() < TOL_ACC, (n, m, int(err.argmax()), err.max())


def test_direct_sum_softened(nb, oracle):
    n, m, eps = 2000, N_PROBES, 0.05
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], m)
    ref = direct_ref(oracle, n, posm[:, :3], posm[:, 3], pts, eps=eps)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.field_at(pts)
    err = rel_err(got, ref)
    print(f"field_at theta=0 eps={eps}: max rel err {err.max():.3e}")
    assert err.max() < TOL_ACC
    assert rel_err(got, direct_ref(oracle, n, posm[:, :3], posm[:, 3], pts)).max() > 1e-3     # (the near-body probes feel the softening)


# Many points: from ceil(M / 1024) * chunks >= 1024 on a workgroup takes 1024 points instead of 512 (two register pairs per lane), and
# points beyond what 256 MB of partial rows hold go in a second slab.  N = 2000 (8 chunks): M = 135000 crosses the first threshold.
# N = 20000 (79 chunks, slabs of 211968 points): M = 220000 crosses both.  A point's bits depend on neither: every sub-range asked for
# alone — a few hundred points, one slab, 512 points per workgroup — gives the bytes of the whole call.
@pytest.mark.parametrize("n,m,eps", [(2000, 135000, 0.0), (20000, 220000, 0.0), (20000, 220000, 0.05)])
def test_many_points_across_the_workgroup_shapes_and_the_slab_boundary(nb, oracle, n, m, eps):
    posm, vel = bodies(nb, n)
    pos, mass = posm[:, :3], posm[:, 3]
    pts = probes_for(pos, m)
    slab = 211968
    if m > slab:                                                  # on bodies and beside bodies on either side of the slab boundary
        pts[slab - 25:slab - 15] = pos[200:210]
        pts[slab + 15:slab + 25] = pos[210:220] + np.float32(1e-3)
    with nb.NBodyEngine(n, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.field_at(pts)
        assert np.isfinite(got).all()
        ranges = [(0, 777), (1024 - 3, 1024 + 300), (131072 - 100, 131072 + 100), (m - 500, m), (m - 1, m)]
        if m > slab:
            ranges += [(slab - 300, slab + 300), (slab, slab + 1), (slab - 1, slab)]
        for a, b in ranges:
            assert e.field_at(pts[a:b]).tobytes() == got[a:b].tobytes(), (a, b)
    if eps > 0.0:
        # The softened case is here for the bits of the softened instantiations across the shapes and the slabs.  For accuracy the
        # oracle's softened fp32 sum is no yardstick at 2e-5 in this scene: at point 56, 1e-3 beside body 106, it is 1.2e-4 off its
        # own fp64 sum (worked out on the CPU from the oracle alone).  test_direct_sum_softened holds the softened law to the bound.
        return
    sample = np.unique(np.concatenate([np.arange(0, 64), np.arange(slab - 40, slab + 40) % m, np.arange(m - 64, m),
                                       np.random.default_rng(9).integers(0, m, 600)]))
    err = rel_err(got[sample], direct_at(oracle, pos, mass, pts[sample], eps=eps))
    print(f"field_at theta=0 N={n} M={m} eps={eps}: max rel err on {sample.size} sampled points {err.max():.3e}")
    assert err.max() < TOL_ACC, (int(sample[err.argmax()]), err.max())


def test_bit_level_properties(nb):
    n, m = 2000, N_PROBES
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], m)
    with nb.NBodyEngine(n) as e:
        e.set_state(posm, vel)
        e.step(0.01, 2)
        before = (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done())
        a = e.field_at(pts)
        assert e.field_at(pts).tobytes() == a.tobytes()                       # two calls
        h = m // 2
        assert np.concatenate([e.field_at(pts[:h]), e.field_at(pts[h:])]).tobytes() == a.tobytes()   # a point does not see the others
        p4 = np.zeros((m, 4), np.float32); p4[:, :3] = pts; p4[:, 3] = 123.0
        v16 = p4[:, :3]
        assert v16.strides == (16, 4) and e.field_at(v16).tobytes() == a.tobytes()
        rec = np.zeros(m, nb.PARTICLE_DTYPE)
        rec["Mass"] = 7.0; rec["Velocity"] = 9.0; rec["Position"] = pts
        v40 = rec["Position"]
        assert v40.strides == (40, 4) and e.field_at(v40).tobytes() == a.tobytes()
        # ... and on the output side: stride 40 into the records' Acceleration field, through the C entry point itself
        rc = e._L.nbody_field_at(e._h, rec["Position"].ctypes.data, 40, m, rec["Acceleration"].ctypes.data, 40)
        assert rc == 0 and rec["Acceleration"].tobytes() == a.tobytes()
        assert (rec["Mass"] == 7.0).all() and (rec["Velocity"] == 9.0).all()
        assert e._L.nbody_field_at(e._h, rec["Position"].ctypes.data, 40, 0, rec["Acceleration"].ctypes.data, 40) == 0   # n == 0: a no-op
        assert (e.particles().tobytes(), e.accelerations().tobytes(), e.steps_done()) == before


# ---- theta > 0 -------------------------------------------------------------------------------------------------------------------

def tree_probes(pos, root_com):
    """The 777 points of the theta = 0 tests plus: one exactly at the root's CoM, one far outside, one on a body, one 1e-3 beside one."""
    extra = np.array([root_com, (1e6, 1e6, 1e6), pos[123], pos[321] + np.float32(1e-3)], np.float32)
    return np.concatenate([probes_for(pos, N_PROBES), extra])


@pytest.mark.parametrize("n,eps,div_mode", [(2000, 0.0, 0), (3000, 0.0, 0), (5000, 0.0, 0), (20000, 0.0, 0),
                                            (2000, 0.05, 0), (20000, 0.05, 0), (2000, 0.0, 1)])
def test_walk_of_the_last_tree(nb, probe_ref, n, eps, div_mode):
    # the four build / walk families: LDS build, small system on the global walk, windows, lane walk with hop words
    posm, vel = bodies(nb, n)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    with nb.NBodyEngine(n, theta=1.0, eps=eps, bh_div_mode=div_mode) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        own = e.accelerations()
        stats = e.bh_stats()
        assert e.field_at(pos).tobytes() == np.ascontiguousarray(own).tobytes()     # at a body's position: that body's own walk
        pts = tree_probes(pos, stats["root_com"])
        got = e.field_at(pts)
        assert e.accelerations().tobytes() == own.tobytes() and e.bh_stats()["nodes"] == stats["nodes"]
    ref, com, nodes = probe_ref.field(pos, mass, pts, 1.0, eps=eps, div_mode=div_mode)
    assert com.tobytes() == stats["root_com"].tobytes() and nodes == stats["nodes"]
    assert not ref[N_PROBES].any()                                # d == 0 at the root ends the walk there
    assert got.tobytes() == ref.tobytes(), (n, eps, div_mode, int((got != ref).any(axis=1).sum()))


def test_walk_that_opens_every_cell_is_the_direct_sum(nb, oracle):
    n = 2000
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], N_PROBES)
    ref = direct_ref(oracle, n, posm[:, :3], posm[:, 3], pts)
    with nb.NBodyEngine(n, theta=1e-30) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        got = e.field_at(pts)
    err = rel_err(got, ref)
    print(f"field_at theta=1e-30: max rel err {err.max():.3e}")
    assert err.max() < TOL_ACC


def test_after_a_step_the_last_tree_is_that_of_the_positions_before_its_update(nb, probe_ref):
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
        got = e.field_at(pts)
    ref, _, _ = probe_ref.field(x1[:, :3], x1[:, 3], pts, 1.0, root_origin=root)
    assert got.tobytes() == ref.tobytes()


# ---- the frame's records and the queries share one staging pair ------------------------------------------------------------------

@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("theta", [0.0, 1.0])
def test_queries_between_frames_disturb_neither(nb, theta, pinned):
    """nbody_tick's FParticle records (theta = 0: the one-launch step's mirror; theta = 1: written by the walk through a mapped pointer)
    and the point queries go through the same staging pair.  Twin A asks between its frames — 8 points first, then 8192, whose
    8192 x 56 bytes (jerk_at) outgrow the 80 KB the records need, so the pair is reallocated between two frames —, twin B only after
    them: every frame's records and Size are the same bytes, and each of A's answers is that of a fresh context stepped to the same
    state with step() alone."""
    n, dt = 2000, 0.01
    posm, vel = bodies(nb, n)
    few, many = probes_for(posm[:, :3], 8), probes_for(posm[:, :3], 8192)
    pvel = np.random.default_rng(11).uniform(-50, 50, many.shape).astype(np.float32)
    queries = [lambda e: [e.potential_at(few)], lambda e: list(e.jerk_at(many, pvel)), lambda e: [e.field_at(many)]]

    def run(ask_between):
        frames, answers = [], []
        with nb.NBodyEngine(n, theta=theta) as e:
            e.set_state(posm, vel)
            out = np.zeros(n, nb.PARTICLE_DTYPE)
            if pinned:
                e.pin(out)
            for q in queries:
                size, rec = e.tick(dt, out=out)
                assert rec is out
                frames.append((np.float32(size).tobytes(), out.tobytes()))
                if ask_between:
                    answers.append([a.tobytes() for a in q(e)])
            if not ask_between:
                answers = [[a.tobytes() for a in q(e)] for q in queries]
        return frames, answers

    frames_a, answers_a = run(True)
    frames_b, answers_b = run(False)
    for k, (fa, fb) in enumerate(zip(frames_a, frames_b)):
        assert fa[0] == fb[0], f"frame {k}: Size differs between the twins"
        assert fa[1] == fb[1], f"frame {k}: the records differ between the twins"
    assert answers_a[2] == answers_b[2]                            # (the one query both twins ask at the same state)
    for k, q in enumerate(queries):
        with nb.NBodyEngine(n, theta=theta) as e:
            e.set_state(posm, vel)
            for _ in range(k + 1):
                e.step(dt, 1)
            assert [a.tobytes() for a in q(e)] == answers_a[k], f"query {k}: not what a fresh context at the same state answers"


# ---- errors ----------------------------------------------------------------------------------------------------------------------

def test_errors(nb):
    n = 2000
    posm, vel = bodies(nb, n)
    pts = probes_for(posm[:, :3], 16)
    E = nb._lib
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError) as err:                 # no tree yet
            e.field_at(pts)
        assert err.value.code == E.ERR_STATE and "nbody_compute_forces" in str(err.value)
        e.compute_forces()
        e.field_at(pts)
        e.set_theta(0.5)
        with pytest.raises(nb.NBodyError) as err:                 # the tree is another angle's
            e.field_at(pts)
        assert err.value.code == E.ERR_STATE
        e.compute_forces()
        e.field_at(pts)
        out = np.zeros((16, 3), np.float32)
        f = e._L.nbody_field_at
        assert f(e._h, pts.ctypes.data, 8, 16, out.ctypes.data, 12) == E.ERR_INVALID
        assert f(e._h, pts.ctypes.data, 12, 16, out.ctypes.data, 11) == E.ERR_INVALID
        assert f(e._h, None, 12, 16, out.ctypes.data, 12) == E.ERR_INVALID
        assert f(e._h, pts.ctypes.data, 12, 16, None, 12) == E.ERR_INVALID
        assert f(e._h, pts.ctypes.data, 12, -1, out.ctypes.data, 12) == E.ERR_INVALID
    for precision in ("f64", "f32_kahan"):
        with nb.NBodyEngine(n, precision=precision) as e:
            e.set_state(posm, vel)
            with pytest.raises(nb.NBodyError) as err:
                e.field_at(pts)
            assert err.value.code == E.ERR_UNSUPPORTED
    with nb.NBodyEngine(n, i_begin=0, i_count=1000) as e:         # a slice context
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError) as err:
            e.field_at(pts)
        assert err.value.code == E.ERR_UNSUPPORTED
        with pytest.raises(nb.NBodyError) as err:
            e.set_tracers(pts)
        assert err.value.code == E.ERR_UNSUPPORTED
