"""Plummer softening at theta > 0: every walk, the deep path, several devices, checkpoints and the actor apply nbody_params.eps to the
term of every accepted node (ds2 = d2 + (float)(eps * eps), include/nbody.h), and every bit and byte of the answer equals the CPU
restatement's (tests/cpp/bh_softened_ref.c, pinned to the oracle at eps = 0 by tests/test_bh_softening.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bh_softened_ref import SoftenedRef
from conftest import particles_from, rel_err

pytestmark = pytest.mark.gpu
THETA = 1.0                  # OctreeSearch.cpp:85
EPS = (0.5, 30.0, 3000.0)    # below, about and far above the scenes' nearest-neighbour distances (~16 and ~42)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return SoftenedRef(tmp_path_factory.mktemp("bh_softened_ref"))


def _scene(nb, n, kind):
    return nb.ic_reference_box(n, 1000.0, seed=n % 97 + 1) if kind == "box" else nb.ic_plummer(n, seed=n % 89 + 1)


def _cold_and_ticks(nb, soft, posm, vel, eps, ticks=3, theta=THETA, div_mode=0, what=""):
    """A cold force pass (records, root CoM, node count), then `ticks` Ticks (the later ones from the previous frame's order): every
    byte of the records, Size and the root CoM equal the restatement's."""
    n = posm.shape[0]
    pos = np.ascontiguousarray(posm[:, :3]); m = np.ascontiguousarray(posm[:, 3])
    ref, com0, nodes = soft.forces(pos, m, theta, eps=eps, div_mode=div_mode)
    q = particles_from(nb, posm, vel)
    com = None
    with nb.NBodyEngine(n, theta=theta, eps=eps, bh_div_mode=div_mode) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        assert e.accelerations().tobytes() == ref.tobytes(), what
        st = e.bh_stats()
        assert st["nodes"] == nodes and st["root_com"].tobytes() == com0.tobytes(), what
        for frame in range(ticks):
            size_dev, out = e.tick(0.01)
            com, size = soft.tick(q, 0.01, theta, eps=eps, root_com=com, div_mode=div_mode)
            assert size_dev == size, (what, frame)
            assert out.tobytes() == q.tobytes(), (what, frame)
        assert e.bh_stats()["root_com"].tobytes() == com.tobytes(), what


@pytest.mark.parametrize("n", [2000, 3000, 8192, 16384, 65536, 140000])
def test_every_walk_equals_the_restatement(nb, soft, n):
    # 2000: the small systems' walk on the tree in LDS; 3000: on the global tree; 8192: a wave per body; 16384 and 65536: a lane per
    # body; 140000: two steps to a turn, radix sort
    for kind in ("box", "plummer"):
        posm, vel = _scene(nb, n, kind)
        for eps in (EPS if n <= 16384 else EPS[1:] if kind == "box" else EPS[:1]):
            _cold_and_ticks(nb, soft, posm, vel, eps, what=f"n={n} {kind} eps={eps}")


@pytest.mark.parametrize("walk,rows_max,wave_max,n", [
    ("sixteen lanes per body", "1000000", "0", 9000),
    ("a lane per body", "0", "0", 4100),
    ("a wave per body", "1000000", "1000000", 15000),
])
def test_every_walk_at_the_boundaries_moved(nb, soft, monkeypatch, walk, rows_max, wave_max, n):
    monkeypatch.setenv("NBODY_BH_ROWS_MAX_N", rows_max)
    monkeypatch.setenv("NBODY_BH_WAVE_MAX_N", wave_max)
    for kind in ("box", "plummer"):
        posm, vel = _scene(nb, n, kind)
        _cold_and_ticks(nb, soft, posm, vel, 30.0, ticks=2, what=f"{walk} n={n} {kind}")


_ROWS_CHILD = r"""
import sys, tempfile
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import parallelnbody_amd as nb
from bh_softened_ref import SoftenedRef
from test_bh_softening_gpu import _cold_and_ticks, _scene
soft = SoftenedRef(tempfile.mkdtemp())
for n in (2000, 3000, 9000):
    for kind in ("box", "plummer"):
        posm, vel = _scene(nb, n, kind)
        _cold_and_ticks(nb, soft, posm, vel, 30.0, ticks=2, what=f"NBODY_BH_WALK=rows n={n} {kind}")
print("rows walks ok")
"""


def test_the_sixteen_lanes_walks_of_every_size(nb):
    # NBODY_BH_WALK=rows (read once per process) puts the small systems on bh_walk_compact_kernel and the larger ones on
    # bh_walk_rows_kernel: a child process of its own
    env = dict(os.environ, NBODY_BH_WALK="rows")
    r = subprocess.run([sys.executable, "-c", _ROWS_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rows walks ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_softening_changes_the_answer_of_the_shipped_scene(nb):
    posm, vel = nb.ic_reference_box(2000, 1000.0, seed=1)
    acc = {}
    for eps in (0.0, 5.0):
        with nb.NBodyEngine(2000, theta=THETA, eps=eps) as e:
            e.set_state(posm, vel)
            e.compute_forces()
            acc[eps] = e.accelerations()
    changed = np.any(acc[0.0] != acc[5.0], axis=1)
    assert changed.mean() > 0.5, changed.mean()


@pytest.mark.parametrize("precision", ["f32", "f32_kahan"])
@pytest.mark.parametrize("eps", [1.0, 30.0])
def test_theta_to_zero_is_the_softened_all_pairs_law(nb, precision, eps):
    n = 2000
    for posm, vel in (nb.ic_reference_box(n, 1000.0, seed=1), nb.ic_plummer(n, seed=1)):
        with nb.NBodyEngine(n, theta=1e-30, eps=eps) as t, nb.NBodyEngine(n, eps=eps, precision=precision) as d:
            for e in (t, d):
                e.set_state(posm, vel)
                e.compute_forces()
            a, ref = t.accelerations(), d.accelerations(np.float64)
        assert np.linalg.norm(a - ref) / np.linalg.norm(ref) < 2e-5
        assert rel_err(a, ref).max() < 1e-4                     # (a body whose terms nearly cancel loses a few more digits)


def _deep_scene(nb, n, where):
    """tests/test_bh_deep_gpu.py's scenes (duplicated: that file stays as it is): a runaway body holds Size at 1e9; "far" a pair 1e-4
    apart at |x| ~ 500, "run_far" six bodies a few ulps apart in one cell of level 42, split at levels 43 .. 46."""
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=1)
    posm[0, :3] = (1.0e9, -2.0e8, 3.0e8)
    posm[0, 3] = np.float32(1e-6)
    if where == "far":
        posm[1, :3] = (500.25, 300.5, -200.75)
        posm[2, :3] = posm[1, :3] + np.float32(1e-4)
    else:
        base = np.array([500.2500915527344, 300.5, -200.75], np.float32)
        for k, (dx, dy) in enumerate(((4, 3), (0, 0), (3, 1), (1, 0), (4, 0), (2, 2))):
            posm[1 + k, :3] = base + np.array([dx, dy, 0], np.float32) * np.float32(2.0 ** -15)
    vel[:7, :3] = 0.0
    return posm, vel


@pytest.mark.parametrize("n,where", [(2000, "far"), (2000, "run_far"), (65536, "far"), (65536, "run_far")])
def test_deep_context_softened_cold_and_warm(nb, oracle, soft, n, where):
    posm, vel = _deep_scene(nb, n, where)
    eps = 1e-3                                                  # (comparable to the pair's distance, small against the box's)
    pos = np.ascontiguousarray(posm[:, :3]); m = np.ascontiguousarray(posm[:, 3])
    assert oracle.octree_depth_f32(pos) > 42
    ref, com0, nodes = soft.forces(pos, m, THETA, eps=eps)
    q = particles_from(nb, posm, vel)
    com = None
    with nb.NBodyEngine(n, theta=THETA, eps=eps) as e:
        e.set_bh_max_depth(200)
        e.set_state(posm, vel)
        e.compute_forces()
        assert e.accelerations().tobytes() == ref.tobytes()
        assert e.bh_stats()["nodes"] == nodes and e.bh_stats()["levels"] > 42
        for frame in range(3):
            size_dev, out = e.tick(0.01)
            com, size = soft.tick(q, 0.01, THETA, eps=eps, root_com=com)
            assert size_dev == size and out.tobytes() == q.tobytes(), frame
        e.step(0.01, 2)                                          # queued together: a deep frame, a warm one behind it
        for _ in range(2):
            com, size = soft.tick(q, 0.01, THETA, eps=eps, root_com=com)
        assert e.particles().tobytes() == q.tobytes()
        assert e.bh_stats()["root_com"].tobytes() == com.tobytes()


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    # the stand-in for RCCL tests/test_multi_parts_gpu.py builds: several parts of one context on the one GPU of the test box
    so = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "fake_rccl.c"), "-o", so, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return so


@pytest.mark.parametrize("n", [2000, 65536])
def test_four_parts_equal_one_device_and_the_restatement(nb, soft, fake_rccl, monkeypatch, n):
    monkeypatch.setenv("NBODY_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("NBODY_MULTI_SHARE_DEVICE", "1")
    posm, vel = _scene(nb, n, "box")
    eps = 30.0
    q = particles_from(nb, posm, vel)
    com = None
    with nb.NBodyEngine(n, theta=THETA, eps=eps) as one, nb.NBodyEngine(n, theta=THETA, eps=eps, devices=[0] * 4) as many:
        for e in (one, many):
            e.set_state(posm, vel)
            e.step(0.01, 3)
        for _ in range(3):
            com, _ = soft.tick(q, 0.01, THETA, eps=eps, root_com=com)
        p1, v1, a1 = one.state()
        p4, v4, a4 = many.state()
        assert p1.tobytes() == p4.tobytes() and v1.tobytes() == v4.tobytes() and a1.tobytes() == a4.tobytes()
        assert p1[:, :3].tobytes() == np.ascontiguousarray(q["Position"]).tobytes()
        assert v1[:, :3].tobytes() == np.ascontiguousarray(q["Velocity"]).tobytes()
        assert a1[:, :3].tobytes() == np.ascontiguousarray(q["Acceleration"]).tobytes()


@pytest.mark.parametrize("n", [2000, 65536])
def test_checkpoint_resume_equals_straight_frames(nb, tmp_path, n):
    posm, vel = _scene(nb, n, "plummer")
    eps = 30.0
    path = str(tmp_path / "soft.ckpt")
    with nb.NBodyEngine(n, theta=THETA, eps=eps) as a:
        a.set_state(posm, vel)
        a.step(0.01, 6)
        straight = a.state()
    with nb.NBodyEngine(n, theta=THETA, eps=eps) as b:
        b.set_state(posm, vel)
        b.step(0.01, 3)
        b.save_checkpoint(path)
    with nb.NBodyEngine(n, theta=THETA, eps=eps) as c:
        c.load_checkpoint(path)
        c.step(0.01, 3)
        resumed = c.state()
    for x, y in zip(straight, resumed):
        assert x.tobytes() == y.tobytes()


def test_the_actor_softens_at_its_default_theta(nb, soft):
    posm, vel = nb.ic_reference_box(2000, 1000.0, seed=1)
    p = particles_from(nb, posm, vel)
    eps = 30.0
    a = nb.OctreeSearch(eps=eps)                                 # Theta = 1, the actor's default
    a.SetParticles(p)
    q = p.copy()
    com = None
    for frame in range(4):
        a.Tick(0.0)
        assert a.LastStatus == 0
        com, _ = soft.tick(q, 0.01, THETA, eps=eps, root_com=com)
        assert a.Particles.tobytes() == q.tobytes(), frame


def test_softened_fuzz_every_bit_and_byte(nb, oracle, soft):
    """Random systems of 2 .. 20000 bodies, random eps (0 among them, one whose square is subnormal in fp32, one far above the box):
    the force pass in every bit, two Ticks in every byte.  NBODY_FUZZ_SEED / NBODY_FUZZ_TRIALS run it longer."""
    rng = np.random.default_rng(int(os.environ.get("NBODY_FUZZ_SEED", "2718")))
    trials = int(os.environ.get("NBODY_FUZZ_TRIALS", "16"))
    ran = 0
    for trial in range(trials):
        n = int(rng.integers(2, 4097)) if rng.random() < 0.5 else int(rng.integers(4097, 20001))
        eps = float(rng.choice([0.0, 1e-22, 1e6, 10.0 ** rng.uniform(-3, 3)]))
        assert eps != 1e-22 or 0.0 < np.float32(eps * eps) < np.finfo(np.float32).tiny
        theta = float(rng.choice([1.0, 0.5, 1.7]))
        div_mode = int(rng.integers(0, 2))
        if rng.random() < 0.5:
            posm = np.concatenate([rng.uniform(-1000, 1000, (n, 3)), 10.0 ** rng.uniform(0, 3, (n, 1))], 1).astype(np.float32)
        else:
            k = int(rng.integers(1, 6))
            centres = rng.uniform(-800, 800, (k, 3))
            widths = 10.0 ** rng.uniform(-1, 2.5, k)
            which = rng.integers(0, k, n)
            pos = centres[which] + rng.normal(0, 1, (n, 3)) * widths[which, None]
            posm = np.concatenate([pos, 10.0 ** rng.uniform(0, 3, (n, 1))], 1).astype(np.float32)
        posm[:, 3] *= np.float32(1e-4)
        if oracle.octree_depth_f32(posm[:, :3]) > 42:
            continue                                             # (a default context refuses such a scene: tests/test_bh_deep_gpu.py)
        vel = np.concatenate([rng.normal(0, 10.0, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
        _cold_and_ticks(nb, soft, posm, vel, eps, ticks=2, theta=theta, div_mode=div_mode,
                        what=f"trial {trial}: n={n} eps={eps} theta={theta} div_mode={div_mode}")
        ran += 1
    assert ran >= trials // 2, ran
