"""The oracle against the reference's own compiled code (oracle/_ref/nbody_ref: Source/NBody/OctreeSearch.cpp of the reference,
unchanged, under g++ against the stand-in engine headers of oracle/ue4_standin/, driven by oracle/ref_driver.cpp).

Everything the suite calls "bit for bit" rests on oracle/nbody_oracle.c, a restatement by reading.  Here the restatement meets what
it restates: frames, Size, root centre of mass, forces at several opening angles and roots, and the draw sequence — every byte.
No GPU.  The tests skip in one case only: no binary and no reference sources to build one from (oracle/reference.py)."""
import os

import numpy as np
import pytest

from oracle import reference as R
import reference_scenes as S

pytestmark = pytest.mark.skipif(not R.available(), reason="no oracle/_ref/nbody_ref and no reference sources to build it from")

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FAMILIES = ("box", "gauss", "clump", "lattice", "boundary", "massless", "tiny", "huge", "negzero")
SIZES = (1, 2, 3, 5, 9, 64, 300, 1000, 2500)
DRAWS_PER_FAMILY = 45           # 405 draws: each family meets each N five times, with 1 to 4 frames


@pytest.fixture(scope="module")
def ref():
    assert R.build() is not None
    return R


def _scene(family, n, rng):
    pos = rng.uniform(-500, 500, (n, 3))
    m = rng.uniform(1, 5000, n)
    if family == "gauss":
        pos = rng.normal(0, 100, (n, 3))
    if family == "clump":                                   # a tight clump far from the origin, one body at the origin
        pos = rng.normal(0, 1e-3, (n, 3)) + 400.0
        pos[0] = 0
    if family == "lattice":
        pos = rng.integers(-8, 9, (n, 3)).astype(float) * 62.5
    if family == "boundary":                                # every body ON an octant boundary of the first root
        pos[:, rng.integers(0, 3)] = 0.0
    if family == "massless":
        m[rng.random(n) < 0.7] = 0.0
    if family == "tiny":
        pos *= 1e-20
        m *= 1e-30
    if family == "huge":
        pos *= 1e10
    if family == "negzero":
        pos[rng.random((n, 3)) < 0.3] = -0.0
    return R.particles(pos.astype(np.float32), m, rng.normal(0, 10, (n, 3)))


def _oracle_frames(O, q0, dt, frames, pow_mode, div_mode=0):
    """`frames` oracle Ticks: [(records, size, com)], or None as soon as a frame's insertion goes deeper than the reference may be
    sent (or the oracle refuses it: coincident bodies)."""
    q = q0.copy()
    com, size, out = None, 0.0, []
    for _ in range(frames):
        try:
            com, size = O.tick_aos_f32(q, dt, theta=1.0, root_com=com, size=size, pow_mode=pow_mode, div_mode=div_mode)
        except RuntimeError:
            return None
        if O.last_max_depth() > R.MAX_DEPTH:
            return None
        out.append((q.copy(), np.float32(size), com.copy()))
    return out


def _same_frames(got, want):
    return all(g["records"].tobytes() == w[0].tobytes() and g["size"].tobytes() == w[1].tobytes() and g["com"].tobytes() == w[2].tobytes()
               for g, w in zip(got, want))


@pytest.fixture(scope="module")
def fuzz(oracle, ref):
    """The whole fuzz, once: per family the draws made, dropped and run, and every scene on which a reading differs."""
    made = {f: 0 for f in FAMILIES}
    ran = {f: 0 for f in FAMILIES}
    differs = {0: [], 3: []}
    draws_wrong = []
    for family in FAMILIES:
        rng = np.random.default_rng([2015, FAMILIES.index(family)])
        for draw in range(DRAWS_PER_FAMILY):
            n = SIZES[draw % len(SIZES)]
            frames = int(rng.integers(1, 5))
            q0 = _scene(family, n, rng)
            made[family] += 1
            dt = 1e-3 if family == "huge" else 0.01
            if len(np.unique(q0["Position"], axis=0)) != n or oracle.octree_depth_f32(q0["Position"]) > R.MAX_DEPTH:
                continue
            want = _oracle_frames(oracle, q0, dt, frames, pow_mode=0)
            if want is None:
                continue
            got = ref.run(q0, [ref.ticks_command(dt, frames, True)])[0]
            ran[family] += 1
            tag = (family, n, frames, draw)
            if not _same_frames(got, want):
                differs[0].append(tag)
            want3 = _oracle_frames(oracle, q0, dt, frames, pow_mode=3)
            if want3 is None or not _same_frames(got, want3):
                differs[3].append(tag)
            # the last frame's draw calls against the oracle's leaves of that frame's tree: the positions before the frame's update,
            # rooted at the previous frame's centre of mass
            before = q0["Position"] if frames == 1 else want[-2][0]["Position"]
            origin = (0.0, 0.0, 0.0) if frames == 1 else want[-2][2]
            boxes, order = oracle.octree_leaves_f32(before, q0["Mass"], root_origin=origin, root_size=want[-1][1])
            got_boxes, got_points = ref.draw_sequence(got[-1]["calls"])
            if not (got_boxes.tobytes() == boxes.tobytes() and got_points.tobytes() == got[-1]["records"]["Position"][order].tobytes()):
                draws_wrong.append(tag)
    return {"made": made, "ran": ran, "differs": differs, "draws_wrong": draws_wrong}


def test_fuzz_covers_every_family_and_drops_few(fuzz):
    made, ran = sum(fuzz["made"].values()), sum(fuzz["ran"].values())
    print()
    for f in FAMILIES:
        print(f"  {f:9s} draws {fuzz['made'][f]:3d}  run {fuzz['ran'][f]:3d}  dropped {fuzz['made'][f] - fuzz['ran'][f]:3d}")
    print(f"  total     draws {made:3d}  run {ran:3d}  dropped {made - ran:3d} = {100.0 * (made - ran) / made:.1f} % (depth > {R.MAX_DEPTH} or coincident bodies)")
    print(f"  scenes on which pow_mode 3, the device's reading, differs from the compiled reference: {len(fuzz['differs'][3])} {fuzz['differs'][3][:8]}")
    assert ran >= 300
    assert min(fuzz["ran"].values()) >= 20, fuzz["ran"]
    assert made - ran <= 0.15 * made, (made, ran)


def test_oracle_frames_equal_the_reference_on_every_fuzzed_scene(fuzz):
    # records, Size and root centre of mass of every frame, byte for byte, under the default reading (pow_mode 0, div_mode 0)
    assert fuzz["differs"][0] == []


def test_oracle_leaves_equal_the_reference_draw_calls_on_every_fuzzed_scene(fuzz):
    assert fuzz["draws_wrong"] == []


def test_the_devices_reading_of_the_cube_equals_the_reference_too(fuzz):
    # pow_mode 3 — the correctly rounded (d*d)*d in double, which the device computes — against glibc's pow(d, 3) in the compiled
    # reference.  glibc's pow is not correctly rounded, so the two MAY differ; a scene on which they do is recorded here by failing.
    assert fuzz["differs"][3] == []


def _refbox():
    g = np.load(os.path.join(GOLDEN, "refbox_n2000_seed1.npz"))
    return g, R.particles(g["posm"][:, :3], g["posm"][:, 3], g["vel"])


@pytest.mark.parametrize("pow_mode,div_mode", [(0, 1), (1, 0), (2, 0)])
def test_the_check_can_fail(oracle, ref, pow_mode, div_mode):
    # one Tick of the shipped scene under each OTHER reading the oracle carries: more than 1000 of 2000 acceleration rows differ
    _, q0 = _refbox()
    got = ref.run(q0, [ref.ticks_command(0.01, 1, False)])[0][0]["records"]
    other = _oracle_frames(oracle, q0, 0.01, 1, pow_mode=pow_mode, div_mode=div_mode)[0][0]
    rows = int((other["Acceleration"].view(np.uint32) != got["Acceleration"].view(np.uint32)).any(axis=1).sum())
    print(f"pow_mode {pow_mode} div_mode {div_mode}: {rows} of {len(q0)} rows differ")
    assert rows > 1000
    same = _oracle_frames(oracle, q0, 0.01, 1, pow_mode=0, div_mode=0)[0][0]
    assert same.tobytes() == got.tobytes()


THETAS = (0.0, 0.25, 0.5, 1.0, 1.7)


@pytest.mark.parametrize("fixture", ["refbox_n2000_seed1", "plummer_n1024_seed1"])
def test_forces_at_other_opening_angles_and_roots(oracle, ref, fixture):
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    q0 = R.particles(g["posm"][:, :3], g["posm"][:, 3], g["vel"])
    pos, mass = q0["Position"].copy(), q0["Mass"].copy()
    size = oracle.bounds_f32(pos)
    # a nonzero root: the previous frame's centre of mass, as CreateOctree takes it (OctreeSearch.cpp:77-79)
    frame1 = ref.run(q0, [ref.ticks_command(0.01, 1, False)])[0][0]
    assert np.any(frame1["com"] != 0)
    for origin in ((0.0, 0.0, 0.0), tuple(frame1["com"])):
        assert oracle.octree_depth_f32(pos, root_origin=origin, root_size=size) <= R.MAX_DEPTH
        got = ref.run(q0, [ref.forces_command(theta, origin, size) for theta in THETAS])
        for theta, r in zip(THETAS, got):
            acc, com, _ = oracle.octree_forces_f32(pos, mass, theta, root_origin=origin, root_size=size)
            assert r["acc"].tobytes() == acc.tobytes(), (theta, origin)
            assert r["com"].tobytes() == com.tobytes(), (theta, origin)
        if origin == (0.0, 0.0, 0.0):
            assert got[0]["acc"].tobytes() == np.ascontiguousarray(g["acc_tree0"]).tobytes()    # the reference's own all-pairs order
        accs = [r["acc"] for r in got]
        assert all(not np.array_equal(accs[i], accs[i + 1]) for i in range(len(accs) - 1))      # (the angle is really in force)


def test_draw_sequence_of_the_shipped_scene(oracle, ref):
    _, q0 = _refbox()
    n = len(q0)
    on, off = ref.run(q0, [ref.ticks_command(0.01, 2, True), ref.ticks_command(0.01, 2, False)])
    want = _oracle_frames(oracle, q0, 0.01, 2, pow_mode=0)
    before, origin = q0["Position"], (0.0, 0.0, 0.0)
    for f in range(2):
        boxes, order = oracle.octree_leaves_f32(before, q0["Mass"], root_origin=origin, root_size=want[f][1])
        got_boxes, got_points = ref.draw_sequence(on[f]["calls"])
        assert len(got_points) == n and len(got_boxes) == n
        assert got_boxes.tobytes() == boxes.tobytes()                                           # origin, size and order
        assert got_points.tobytes() == on[f]["records"]["Position"][order].tobytes()            # the bodies in that order, where they are NOW
        no_boxes, points = ref.draw_sequence(off[f]["calls"])                                   # ShowOctree off: the points alone
        assert len(no_boxes) == 0 and points.tobytes() == got_points.tobytes()
        before, origin = want[f][0]["Position"], want[f][2]


@pytest.mark.parametrize("name", S.NAMES)
def test_fixtures_are_current(oracle, ref, name):
    # the committed reference_*.npz are what the binary writes today, byte for byte, and stay within the device's depth limit;
    # the oracle — under the default reading and under the device's — gives the same bytes on them
    stored = dict(np.load(os.path.join(GOLDEN, S.file_name(name))))
    fresh = S.record(name, ref, oracle)
    assert sorted(stored) == sorted(fresh)
    for key in sorted(fresh):
        assert stored[key].dtype == fresh[key].dtype and stored[key].shape == fresh[key].shape, key
        assert stored[key].tobytes() == fresh[key].tobytes(), key
    assert os.path.getsize(os.path.join(GOLDEN, S.file_name(name))) <= 191589
