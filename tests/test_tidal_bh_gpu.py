"""The tidal tensor at theta > 0: nbody_tidal_at, nbody_get_tidal and nbody_tidal_time walk the last tree built, and every byte they
return is that of tests/cpp/bh_tidal_ref.c — the reference's octree walked from arbitrary points with the tensor's term in plain C,
pinned by tests/test_bh_tidal_ref.py."""
import numpy as np
import pytest

from bh_tidal_ref import TidalRef, n2_of
from probe_scenes import N_PROBES, bodies, probes_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tidal_ref(tmp_path_factory):
    return TidalRef(tmp_path_factory.mktemp("bh_tidal_ref"))


def tree_probes(pos, root_com):
    """The 777 probes (0-49 ON bodies, 50-59 1e-3 beside bodies where there is room), the root's CoM and a point far outside."""
    extra = np.array([root_com, (1e6, 0.0, 0.0)], np.float32)
    return np.concatenate([probes_for(pos, N_PROBES), extra])


def split(posm):
    return np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])


# N <= 2000: the one-workgroup build, no hop words; N = 6000, 20000: the larger systems' build with hop words
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("theta", [0.5, 1.0])
@pytest.mark.parametrize("n", [2, 64, 257, 2000, 6000, 20000])
def test_walk_of_the_last_tree(nb, tidal_ref, n, theta, eps):
    posm, vel = bodies(nb, n)
    pos, mass = split(posm)
    with nb.NBodyEngine(n, theta=theta, eps=eps) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        own = e.accelerations()
        stats = e.bh_stats()
        pts = tree_probes(pos, stats["root_com"])
        got = e.tidal_at(pts)
        assert e.tidal_at(pts).tobytes() == got.tobytes()
        assert e.tidal_at(pts[300:]).tobytes() == got[300:].tobytes()            # a point does not see the others
        assert e.accelerations().tobytes() == own.tobytes() and e.bh_stats()["nodes"] == stats["nodes"]
    ref = tidal_ref.walk(pos, mass, pts, theta, eps=eps)
    assert ref["root_com"].tobytes() == stats["root_com"].tobytes() and ref["nodes"] == stats["nodes"]
    assert got.shape == (N_PROBES + 2, 6) and np.isfinite(got).all()
    assert not got[N_PROBES].any() and not ref["t"][N_PROBES].any()              # d == 0 at the root ends the walk there
    assert got[N_PROBES + 1].any()                                               # far outside: the root's single term
    assert got.tobytes() == ref["t"].tobytes(), (n, theta, eps, int((got != ref["t"]).any(1).sum()))


@pytest.mark.parametrize("n", [2000, 6000])
def test_after_a_step_the_last_tree_is_that_of_the_positions_before_its_update(nb, tidal_ref, n):
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
        got = e.tidal_at(pts)
    ref = tidal_ref.walk(x1[:, :3], x1[:, 3], pts, 1.0, root_origin=root)
    assert got.tobytes() == ref["t"].tobytes()


@pytest.mark.parametrize("n,eps", [(2000, 0.0), (6000, 0.0), (2000, 0.05), (6000, 0.05)])
def test_tidal_and_tidal_time_are_the_walk_from_every_body(nb, tidal_ref, n, eps):
    posm, vel = bodies(nb, n)
    with nb.NBodyEngine(n, theta=1.0, eps=eps) as twin:
        twin.set_state(posm, vel)
        twin.step(0.01, 1)
        twin.compute_forces()
        want = (twin.accelerations().tobytes(), str(twin.bh_stats()), [a.tobytes() for a in twin.state()[:2]], twin.steps_done())
    with nb.NBodyEngine(n, theta=1.0, eps=eps) as e:
        e.set_state(posm, vel)
        e.step(0.01, 1)
        x1 = e.state()[0]
        root = e.bh_stats()["root_com"]                           # the first tree's CoM roots the diagnostic tree too
        got = e.tidal()
        # the side effects are those of compute_forces(): the stored accelerations, the diagnostic tree; nothing else
        after = lambda: (e.accelerations().tobytes(), str(e.bh_stats()), [a.tobytes() for a in e.state()[:2]], e.steps_done())
        assert after() == want
        assert e.tidal().tobytes() == got.tobytes()
        t, body = e.tidal_time()
        assert e.tidal_time() == (t, body)                        # identical bits, the same body, every run
        assert after() == want
    ref = tidal_ref.walk(x1[:, :3], x1[:, 3], x1[:, :3], 1.0, eps=eps, root_origin=root)
    assert got.tobytes() == ref["t"].tobytes(), (n, int((got != ref["t"]).any(1).sum()))
    n2 = n2_of(ref["t64"])                                        # the reference's unrounded fp64 sums
    print(f"tidal_time theta=1 N={n} eps={eps}: t_min {t!r} at body {body}")
    assert body == int(n2.argmax()) and t == float(1.0 / np.sqrt(np.sqrt(n2.max())))


def test_a_refused_frame_returns_its_error_and_no_tensors(nb):
    # a scene past 42 levels on a context of the default depth: the frame tidal() and tidal_time() run first is refused
    n = 2000
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=1)
    posm[0, :3] = (1.0e9, -2.0e8, 3.0e8)
    posm[0, 3] = np.float32(1e-6)
    posm[1, :3] = (500.25, 300.5, -200.75)
    posm[2, :3] = posm[1, :3] + np.float32(1e-4)
    vel[:7, :3] = 0.0
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        for call in (e.tidal, e.tidal_time):
            with pytest.raises(nb.NBodyError, match="deeper than 42 levels"):
                call()
        with pytest.raises(nb.NBodyError) as er:                  # ... and it left no tree a query may walk
            e.tidal_at(posm[:4, :3])
        assert er.value.code == nb._lib.ERR_STATE
