"""Barnes-Hut trees deeper than the path keys' 42 levels (nbody_set_bh_max_depth): a deep context answers every frame whose
Octree::Add (OctreeSearch.h:60-81) stops at depth <= its limit, and every byte of the answer equals the oracle's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import particles_from

pytestmark = pytest.mark.gpu
THETA = 1.0                  # OctreeSearch.cpp:85
LIMIT = 200                  # the deepest limit a context takes: the oracle's insertion is cut off (201) past it


def _deep_scene(nb, n, where="far", seed=1):
    """The reference's box scene with a runaway body that holds Size at 1e9, and bodies that Add splits below level 42:
      far      a pair 1e-4 apart at |x| ~ 500 (the later body the farther one along every axis)
      far_neg  the same pair with the indices swapped: the pair's order below level 42 is not the order of the bodies' indices
               (the order a stable sort leaves equal keys in)
      near     a pair 1e-26 apart next to the origin (deeper than 100 levels)
      run      six bodies next to the origin in one cell of level 42, in no particular index order, that Add splits at different
               levels (cells of the run end inside it; their forces overflow, so for the force pass only)
      run_far  six bodies a few ulps apart at |x| ~ 500 in one cell of level 42, in no particular index order, split at levels
               43 .. 46 (whole frames: the bodies stay finite and apart)"""
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=seed)
    posm[0, :3] = (1.0e9, -2.0e8, 3.0e8)
    posm[0, 3] = np.float32(1e-6)
    if where in ("far", "far_neg"):
        posm[1, :3] = (500.25, 300.5, -200.75)
        posm[2, :3] = posm[1, :3] + np.float32(1e-4)
        if where == "far_neg":
            posm[[1, 2]] = posm[[2, 1]]
    elif where == "run_far":
        base = np.array([500.2500915527344, 300.5, -200.75], np.float32)
        for k, (dx, dy) in enumerate(((4, 3), (0, 0), (3, 1), (1, 0), (4, 0), (2, 2))):
            posm[1 + k, :3] = base + np.array([dx, dy, 0], np.float32) * np.float32(2.0 ** -15)   # (ulps of |x| in [256, 512))
    elif where == "near":
        posm[1, :3] = (1.0e-20, 2.0e-20, -3.0e-20)
        posm[2, :3] = posm[1, :3] + np.float32(1e-26)
    else:
        for k, x in enumerate((7.0, 1.0, 3.0, 1.5, 7.5, 1.25)):
            posm[1 + k, :3] = (x * 1e-20, 2.0e-20, 1.0e-20)
    vel[:7, :3] = 0.0
    return posm, vel


def _check_tree(e, oracle, posm, limit):
    pos = np.ascontiguousarray(posm[:, :3]); m = np.ascontiguousarray(posm[:, 3])
    ref, com, nodes = oracle.octree_forces_f32(pos, m, THETA, pow_mode=3)
    depth = oracle.last_max_depth()
    boxes, order = oracle.octree_leaves_f32(pos, m)
    assert 42 < depth <= limit, depth
    e.compute_forces()
    st = e.bh_stats()
    np.testing.assert_array_equal(e.accelerations(), ref)
    assert st["nodes"] == nodes and st["levels"] == depth, (st, nodes, depth)
    np.testing.assert_array_equal(st["root_com"], com)
    np.testing.assert_array_equal(e.bh_leaf_order(), order)
    np.testing.assert_array_equal(e.bh_leaf_boxes()[order], boxes)
    return depth


def test_the_targeted_scenes_are_what_they_claim(nb, oracle):
    # (the premises of the scenes below, on the oracle alone: the run's bodies share the cell of level 42 and split at different levels)
    for where in ("run", "run_far"):
        posm, _ = _deep_scene(nb, 2000, where)
        size = oracle.bounds_f32(posm[:, :3])
        run = posm[1:7, :3]
        depths = {oracle.octree_depth_f32(np.stack([run[a], run[b]]), root_size=size) for a in range(6) for b in range(a + 1, 6)}
        assert min(depths) >= 43 and len(depths) >= 3, (where, depths)   # all in one cell of level 42, split at different levels


@pytest.mark.parametrize("where", ["far", "far_neg", "near", "run", "run_far"])
@pytest.mark.parametrize("n", [2000, 65536])
def test_deep_pair_force_pass_and_tree_equal_the_oracle(nb, oracle, n, where):
    posm, vel = _deep_scene(nb, n, where)
    with nb.NBodyEngine(n, theta=THETA) as e:
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError, match="deeper than 42 levels"):   # the default context refuses it, as before
            e.compute_forces()
        e.set_bh_max_depth(200)
        assert e.bh_max_depth() == 200
        depth = _check_tree(e, oracle, posm, 200)
        if where == "near":
            assert depth > 100, depth


def test_deep_pair_force_pass_of_a_million_bodies(nb, oracle):
    posm, vel = _deep_scene(nb, 1 << 20, "far_neg")
    with nb.NBodyEngine(1 << 20, theta=THETA) as e:
        e.set_bh_max_depth(200)
        e.set_state(posm, vel)
        _check_tree(e, oracle, posm, 200)


@pytest.mark.parametrize("n,where,ticks", [(2000, "far", 3), (2000, "run_far", 3), (65536, "far_neg", 3), (65536, "run_far", 3),
                                           (1 << 20, "far_neg", 1)])
def test_deep_ticks_cold_and_warm_equal_the_oracle_in_every_byte(nb, oracle, n, where, ticks):
    posm, vel = _deep_scene(nb, n, where)
    q = particles_from(nb, posm, vel)
    com, size = None, 0.0
    with nb.NBodyEngine(n, theta=THETA) as e:
        e.set_bh_max_depth(200)
        e.set_state(posm, vel)
        for frame in range(ticks):                                  # one frame a call
            size_dev, out = e.tick(0.01)
            com, size = oracle.tick_aos_f32(q, 0.01, theta=THETA, root_com=com, size=size, pow_mode=3)
            assert size_dev == size, frame
            assert out.tobytes() == q.tobytes(), frame
        e.step(0.01, 3)                                              # three frames queued at once: deep ones, warm ones behind them
        for _ in range(3):
            com, size = oracle.tick_aos_f32(q, 0.01, theta=THETA, root_com=com, size=size, pow_mode=3)
        p, v, _ = e.state()
        np.testing.assert_array_equal(p[:, :3], q["Position"])
        np.testing.assert_array_equal(v[:, :3], q["Velocity"])
        np.testing.assert_array_equal(e.bh_stats()["root_com"], com)
        assert e.steps_done() == ticks + 3


def test_the_limit_is_the_oracle_depth(nb, oracle):
    n = 2000
    posm, vel = _deep_scene(nb, n, "far")
    depth = oracle.octree_depth_f32(posm[:, :3])
    assert 42 < depth < 200
    with nb.NBodyEngine(n, theta=THETA) as e:
        e.set_state(posm, vel)
        e.set_bh_max_depth(depth - 1)
        with pytest.raises(nb.NBodyError, match=f"deeper than {depth - 1} levels"):
            e.step(0.01, 2)
        assert e.steps_done() == 0
        p, v, _ = e.state()
        np.testing.assert_array_equal(p, posm); np.testing.assert_array_equal(v, vel)
        e.set_bh_max_depth(depth)
        e.step(0.01, 1)
        assert e.steps_done() == 1
        e.set_bh_max_depth(42)                                       # explicitly 42: today's rule and message
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError, match="deeper than 42 levels: two bodies closer than Size/2"):
            e.step(0.01, 1)


def test_coincident_bodies_are_refused_at_any_limit(nb):
    n = 2000
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=3)
    posm[5, :3] = posm[4, :3]
    with nb.NBodyEngine(n, theta=THETA) as e:
        e.set_bh_max_depth(200)
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError, match="deeper than 200 levels"):
            e.step(0.01, 1)
        assert e.steps_done() == 0
        e.set_theta(0.0)
        e.step(0.01, 1)
        assert e.steps_done() == 1


def test_a_cell_of_level_42_with_more_than_64_bodies_is_refused(nb, oracle):
    # the device orders at most 64 bodies of one cell of level 42 (bh_deep_runs_kernel): 70 distinct bodies next to the origin are
    # refused with a message of their own, and the state stays what it was — though the reference would answer the scene
    n = 2000
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=2)
    posm[0, :3] = (1.0e9, -2.0e8, 3.0e8)
    for k in range(70):
        posm[1 + k, :3] = ((1.0 + k) * 1e-20, 2.0e-20, 1.0e-20)
    assert 42 < oracle.octree_depth_f32(posm[:, :3]) <= 200
    with nb.NBodyEngine(n, theta=THETA) as e:
        e.set_bh_max_depth(200)
        e.set_state(posm, vel)
        with pytest.raises(nb.NBodyError, match="more than 64 bodies share one cell of level 42"):
            e.step(0.01, 2)
        assert e.steps_done() == 0
        p, v, _ = e.state()
        np.testing.assert_array_equal(p, posm); np.testing.assert_array_equal(v, vel)


def test_argument_errors(nb):
    with nb.NBodyEngine(64, theta=THETA) as e:
        assert e.bh_max_depth() == 42
        for bad in (41, 201, -1):
            with pytest.raises(nb.NBodyError):
                e.set_bh_max_depth(bad)
        assert e.bh_max_depth() == 42
    with nb.NBodyEngine(64) as e:                                    # theta == 0: taken, in force once theta > 0
        e.set_bh_max_depth(120)
        assert e.bh_max_depth() == 120
    with nb.NBodyEngine(64, precision="f64") as e:
        with pytest.raises(nb.NBodyError, match="fp32"):
            e.set_bh_max_depth(100)


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    # the same stand-in for RCCL tests/test_multi_parts_gpu.py builds: several parts of one context on the one GPU of the test box
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(root, "tests", "cpp", "fake_rccl.c"), "-o", so, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return so


@pytest.mark.parametrize("n", [2000, 65536])
def test_deep_frames_over_four_parts_equal_one_device(nb, fake_rccl, monkeypatch, n):
    monkeypatch.setenv("NBODY_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("NBODY_MULTI_SHARE_DEVICE", "1")
    posm, vel = _deep_scene(nb, n, "far")
    with nb.NBodyEngine(n, theta=THETA) as one, nb.NBodyEngine(n, theta=THETA, devices=[0] * 4) as many:
        for e in (one, many):
            e.set_bh_max_depth(200)
            e.set_state(posm, vel)
            e.step(0.01, 1)                                          # the first frame's tree goes below level 42
        assert one.bh_stats()["levels"] > 42
        assert one.bh_stats()["levels"] == many.bh_stats()["levels"] and one.bh_stats()["nodes"] == many.bh_stats()["nodes"]
        np.testing.assert_array_equal(one.bh_stats()["root_com"], many.bh_stats()["root_com"])
        for e in (one, many):
            e.step(0.01, 2)
        p1, v1, a1 = one.state()
        p4, v4, a4 = many.state()
        assert p1.tobytes() == p4.tobytes() and v1.tobytes() == v4.tobytes() and a1.tobytes() == a4.tobytes()
        assert one.steps_done() == many.steps_done() == 3


def test_an_actor_with_the_limit_set_keeps_ticking_a_deep_scene(nb, oracle):
    posm, vel = _deep_scene(nb, 2000, "far")
    p = particles_from(nb, posm, vel)
    a = nb.OctreeSearch()
    a.SetParticles(p)
    a.set_theta(THETA)
    a.set_bh_max_depth(200)
    q = p.copy()
    com, size = None, 0.0
    for _ in range(3):
        a.Tick(0.0)
        assert a.LastStatus == 0
        com, size = oracle.tick_aos_f32(q, 0.01, theta=THETA, root_com=com, size=size, pow_mode=3)
    assert a.Particles.tobytes() == q.tobytes()


def _fuzz_scene(rng, n):
    """tests/test_bh_gpu.py's generator of the two fuzzes (duplicated: that file stays as it is): a few clumps of very different
    widths, a uniform background, masses over three decades — the scenes that reach past depth 42 in 10-21 of 150 per seed."""
    kind = rng.integers(0, 3)
    if kind == 0:
        pos = rng.uniform(-1000, 1000, (n, 3))
    else:
        k = int(rng.integers(1, 6))
        centres = rng.uniform(-800, 800, (k, 3))
        widths = 10.0 ** rng.uniform(-3, 2.5, k)
        which = rng.integers(0, k, n)
        pos = centres[which] + rng.normal(0, 1, (n, 3)) * widths[which, None]
        if kind == 2:
            back = rng.random(n) < 0.3
            pos[back] = rng.uniform(-1000, 1000, (int(back.sum()), 3))
    posm = np.concatenate([pos, 10.0 ** rng.uniform(0, 3, (n, 1))], 1).astype(np.float32)
    if n > 3:
        posm[0, :3] = 0.0
    return posm


def _runaway(rng, posm):
    """In half the scenes one body has run away to ~1e9, as in the reference's box scene: Size follows it, and a clump's bodies then
    share cells down to level 42 and below (the scenes this feature is for)."""
    if posm.shape[0] > 3 and rng.random() < 0.5:
        posm[1, :3] = rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(7, 9)
        posm[1, 3] = np.float32(1e-3)


def test_deep_fuzz_every_bit_of_the_force_pass(nb, oracle):
    """The force-pass fuzz of tests/test_bh_gpu.py at limit 200: a scene is refused only where the oracle's insertion goes past
    depth 200 (coincident bodies), and every other scene — those past depth 42 included — equals the oracle's tree in every bit.
    NBODY_FUZZ_SEED / NBODY_FUZZ_TRIALS run it longer."""
    rng = np.random.default_rng(int(os.environ.get("NBODY_FUZZ_SEED", "77")))
    trials = int(os.environ.get("NBODY_FUZZ_TRIALS", "24"))
    ran = refused = deep = 0
    for trial in range(trials):
        u = rng.random()
        n = (int(rng.integers(2, 4097)) if u < 0.35 else int(rng.integers(4097, 21000)) if u < 0.7 else
             int(rng.integers(21000, 140000)) if u < 0.92 else int(rng.integers(262145, 400000)))
        theta = float(rng.choice([1.0, 1.0, 0.5, 0.3, 1.7]))
        div_mode = int(rng.integers(0, 2))
        posm = _fuzz_scene(rng, n)
        _runaway(rng, posm)
        vel = np.zeros((n, 4), np.float32)
        pos = np.ascontiguousarray(posm[:, :3]); m = np.ascontiguousarray(posm[:, 3])
        with nb.NBodyEngine(n, theta=theta, bh_div_mode=div_mode) as e:
            e.set_bh_max_depth(LIMIT)
            e.set_state(posm, vel)
            try:
                e.compute_forces()
            except nb.NBodyError as err:
                depth = oracle.octree_depth_f32(pos)
                assert depth > LIMIT, f"trial {trial}: n={n} refused ({err}), but Octree::Add of the scene stops at depth {depth}"
                refused += 1
                continue
            a = e.accelerations()
            st = e.bh_stats()
        ref, com, nodes = oracle.octree_forces_f32(pos, m, theta, pow_mode=3, div_mode=div_mode)
        depth = oracle.last_max_depth()
        assert depth <= LIMIT, (trial, n, depth)                        # (a frame that should have been refused and was not)
        np.testing.assert_array_equal(a, ref, err_msg=f"trial {trial}: n={n} theta={theta} div_mode={div_mode} depth={depth}")
        np.testing.assert_array_equal(st["root_com"], com)
        assert st["nodes"] == nodes and st["levels"] == depth, (trial, n, st["levels"], depth)
        deep += depth > 42
        ran += 1
    print(f"deep force-pass fuzz: {ran} of {trials} scenes compared in every bit, {deep} of them past depth 42; {refused} refused "
          f"and confirmed (the oracle's insertion passes depth {LIMIT})")
    assert ran >= trials * 2 // 3, ran


def test_deep_fuzz_every_byte_of_the_frames(nb, oracle):
    """The frames fuzz of tests/test_bh_gpu.py at limit 200 (frames queued several at a time, one by one with the mirror, or as force
    pass + update; records replaced and the opening angle changed between calls): a call is refused only where the oracle's insertion of
    one of its frames goes past depth 200, the refused frame leaves the records alone, and after every other call every byte of the
    records equals the oracle's.  NBODY_FUZZ_SEED / NBODY_FUZZ_TRIALS run it longer."""
    rng = np.random.default_rng(int(os.environ.get("NBODY_FUZZ_SEED", "404")))
    trials = int(os.environ.get("NBODY_FUZZ_TRIALS", "24"))
    ran = refused = deep = 0
    for trial in range(trials):
        u = rng.random()
        n = (int(rng.integers(2, 4097)) if u < 0.3 else int(rng.integers(4097, 21000)) if u < 0.72 else
             int(rng.integers(21000, 70000)) if u < 0.96 else int(rng.integers(70000, 300000)))
        theta = float(rng.choice([1.0, 1.0, 0.5, 1.7]))
        div_mode = int(rng.integers(0, 2))
        posm = _fuzz_scene(rng, n)
        _runaway(rng, posm)
        posm[:, 3] *= np.float32(10.0 ** rng.uniform(-7, -2))
        speed = 10.0 ** rng.uniform(-1, 4.5)
        vel = np.concatenate([rng.normal(0, speed, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
        dt = float(rng.choice([0.01, 0.002, 0.05]))
        q = particles_from(nb, posm, vel)
        com, size = None, 0.0
        went_deep = False
        what = f"trial {trial}: n={n} theta={theta} div_mode={div_mode} speed={speed:.3g} dt={dt}"
        with nb.NBodyEngine(n, theta=theta, bh_div_mode=div_mode) as e:
            e.set_bh_max_depth(LIMIT)
            e.set_state(posm, vel)
            try:
                for call in range(int(rng.integers(2, 6))):
                    size_dev = None
                    how = rng.random()
                    if how < 0.4:
                        k = int(rng.integers(1, 4))
                        e.step(dt, k)
                        out = e.particles()
                    elif how < 0.8:
                        k = 1
                        size_dev, out = e.tick(dt)
                    else:
                        k = 1
                        e.step_begin(); e.step_end(dt)
                        out = e.particles()
                    for _ in range(k):
                        com, size = oracle.tick_aos_f32(q, dt, theta=theta, root_com=com, size=size, pow_mode=3, div_mode=div_mode)
                        assert oracle.last_max_depth() <= LIMIT, (what, call)   # (a frame that should have been refused)
                        went_deep |= oracle.last_max_depth() > 42
                    assert out.tobytes() == q.tobytes(), (what, call)
                    if size_dev is not None:
                        assert size_dev == size, (what, call)
                    between = rng.random()
                    if between < 0.15:
                        some = rng.random(n) < rng.choice([0.001, 0.05, 0.9])
                        q["Position"][some] = (q["Position"][some] * np.float32(rng.choice([0.5, 1.0, 3.0])) +
                                               rng.normal(0, 1.0, (int(some.sum()), 3)).astype(np.float32))
                        e.push_particles(q)
                    elif between < 0.25:
                        theta = float(rng.choice([1.0, 0.5, 0.7, 1.7]))
                        e.set_theta(theta)
            except nb.NBodyError as err:
                confirmed = False
                for _ in range(k):
                    root = np.zeros(3, np.float32) if com is None else com
                    if oracle.octree_depth_f32(q["Position"], root_origin=root) > LIMIT:
                        confirmed = True
                        break
                    com, size = oracle.tick_aos_f32(q, dt, theta=theta, root_com=com, size=size, pow_mode=3, div_mode=div_mode)
                assert confirmed, f"{what}, call {call} ({k} frames): refused ({err}), but Octree::Add of no frame passes depth {LIMIT}"
                got = e.particles()
                for f in ("Position", "Velocity", "Mass"):
                    np.testing.assert_array_equal(got[f], q[f], err_msg=f"{what}: {f} after the refused frame")
                refused += 1
                continue
            np.testing.assert_array_equal(e.bh_stats()["root_com"], com, err_msg=what)
        deep += went_deep
        ran += 1
    assert ran >= trials // 2, ran
    print(f"deep frames fuzz: {ran} of {trials} scenes ran to the end, {deep} of them with frames past depth 42; {refused} refused "
          f"and confirmed (the oracle's insertion of the refused frame passes depth {LIMIT})")
