"""Tracers: massless bodies the engine advances with the bodies (nbody_set_tracers).

In every step a tracer at y_n gets the field of the bodies at x_n — theta = 0: the direct sum at the project's all-pairs tolerance;
theta > 0: the walk of that frame's tree, every bit of tests/cpp/bh_probe_ref.c — and then the bodies' own fp32 kick-drift, every bit of
the oracle's.  The bodies never notice: every byte of their records equals a twin context's without tracers."""

import numpy as np
import pytest

from bh_probe_ref import ProbeRef
from conftest import particles_from, rel_err
from probe_scenes import N_PROBES, TOL_ACC, bodies, direct_at, fuzz_scene, probes_for, sort_counts

pytestmark = pytest.mark.gpu
DT = 0.01


@pytest.fixture(scope="module")
def probe_ref(tmp_path_factory):
    return ProbeRef(tmp_path_factory.mktemp("bh_probe_ref"))


def tracer_start(pos, m=N_PROBES):
    """The probe set of tests/test_field_gpu.py (some ON bodies, some 1e-3 beside one) with velocities from default_rng(8), uniform in
    +-3000 per axis: a tracer that starts ON a body (bodies move 2.5 - 5 units a step) leaves that body's neighbourhood with its first
    step.  One that stays within a unit or two of it feels one term of ~3e7 there, and the yardstick the accelerations are held to — the
    oracle's fp32 sum in body order, that term (body 26 of 20000) first and the other 20000 added underneath it — is then itself off by
    2.9e-5 from its own fp64 sum, more than the 2e-5 it is the yardstick of (worked out on the CPU from the oracle alone, velocities in
    +-300, second step; with +-3000 the oracle's fp32 and fp64 sums agree to 8.4e-6 at worst over the three steps at N = 20000)."""
    y = probes_for(pos, m)
    v = np.random.default_rng(8).uniform(-3000, 3000, (m, 3)).astype(np.float32)
    return y, v


def direct(oracle, x, mass, y):
    return direct_at(oracle, np.ascontiguousarray(x), np.ascontiguousarray(mass), np.ascontiguousarray(y))


# ---- theta = 0 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2000, 20000])                      # the one-launch step; the symmetric pass and its update
def test_all_pairs_steps(nb, oracle, n):
    posm, vel = bodies(nb, n)
    y0, v0 = tracer_start(posm[:, :3])
    with nb.NBodyEngine(n) as e, nb.NBodyEngine(n) as twin, nb.NBodyEngine(n) as e3, nb.NBodyEngine(n) as et:
        assert e.launch_config()["kernel"] == ("forces_block_pk_kernel" if n == 2000 else "forces_sym_pk_kernel")
        for x in (e, twin, e3, et):
            x.set_state(posm, vel)
        for x in (e, e3, et):
            x.set_tracers(y0, v0)
        assert e.tracer_count == N_PROBES and twin.tracer_count == 0
        t0 = e.tracers()
        assert t0[0][:, :3].tobytes() == y0.tobytes() and t0[1][:, :3].tobytes() == v0.tobytes() and not t0[2].any()

        e.compute_forces()                                        # fills the tracers' accelerations, moves nothing
        y, v, a = e.tracers()
        assert y.tobytes() == t0[0].tobytes() and v.tobytes() == t0[1].tobytes()
        assert rel_err(a[:, :3], direct(oracle, posm[:, :3], posm[:, 3], y0)).max() < TOL_ACC
        e.step(0.0, 1)                                            # dt <= 0 freezes everything
        assert [q.tobytes() for q in e.tracers()] == [y.tobytes(), v.tobytes(), a.tobytes()]
        twin.compute_forces()

        for step in range(3):
            x_n = e.state()[0]
            y_n, v_n, _ = e.tracers()
            e.step(DT, 1)
            twin.step(DT, 1)
            y1, v1, a1 = e.tracers()
            ref = direct(oracle, x_n[:, :3], x_n[:, 3], y_n[:, :3])
            err = rel_err(a1[:, :3], ref)
            print(f"tracers theta=0 N={n} step {step}: max rel acc err {err.max():.3e}")
            assert err.max() < TOL_ACC, (step, int(err.argmax()))
            ry, rv = oracle.kick_drift_f32(y_n[:, :3], v_n[:, :3], a1[:, :3], DT)
            assert y1[:, :3].tobytes() == ry.tobytes() and v1[:, :3].tobytes() == rv.tobytes(), step
        assert e.particles().tobytes() == twin.particles().tobytes()        # the bodies never notice
        assert e.steps_done() == twin.steps_done() == 3

        e3.step(DT, 3)                                            # three steps in one call
        assert [q.tobytes() for q in e3.tracers()] == [q.tobytes() for q in e.tracers()]
        assert e3.particles().tobytes() == e.particles().tobytes()
        for _ in range(3):                                        # ... and as three frames of the actor
            _, rec = et.tick(DT)
        assert [q.tobytes() for q in et.tracers()] == [q.tobytes() for q in e.tracers()]
        assert rec.tobytes() == e.particles().tobytes()

        e.set_tracers(np.zeros((0, 3), np.float32))               # removed: the next step is the twin's
        assert e.tracer_count == 0 and e.tracers()[0].shape == (0, 4)
        e.step(DT, 1); twin.step(DT, 1)
        assert e.particles().tobytes() == twin.particles().tobytes()


def test_many_tracers_across_the_slab_boundary(nb, oracle):
    # 220000 tracers against 20000 bodies: 1024 points per workgroup and two slabs of partial rows (tests/test_field_gpu.py has the
    # thresholds).  The accelerations a step stores are the bytes nbody_field_at gives for the same points and bodies — slab by slab, on
    # either side of the boundary —, every tracer gets the oracle's kick-drift of them in every bit, and the bodies never notice.
    n, m, slab = 20000, 220000, 211968
    posm, vel = bodies(nb, n)
    y0, v0 = tracer_start(posm[:, :3], m)
    with nb.NBodyEngine(n) as e, nb.NBodyEngine(n) as twin:
        e.set_state(posm, vel); twin.set_state(posm, vel)
        e.set_tracers(y0, v0)
        for step in range(2):
            y_n, v_n, _ = e.tracers()
            want = e.field_at(y_n[:, :3])
            e.step(DT, 1); twin.step(DT, 1)
            y1, v1, a1 = e.tracers()
            assert a1[:, :3].tobytes() == want.tobytes(), (step, int((a1[:, :3] != want).any(axis=1).sum()))
            ry, rv = oracle.kick_drift_f32(y_n[:, :3], v_n[:, :3], a1[:, :3], DT)
            bad = (y1[:, :3] != ry).any(axis=1) | (v1[:, :3] != rv).any(axis=1)
            assert not bad.any(), (step, int(bad.sum()), int(np.flatnonzero(bad)[0]))
            assert (y1[slab - 5:slab + 5, :3] != y_n[slab - 5:slab + 5, :3]).any(axis=1).all()      # both sides of the boundary moved
        assert e.particles().tobytes() == twin.particles().tobytes()
        x = e.state()[0]
        y, _, _ = e.tracers()
        e.compute_forces()
        a = e.tracers()[2]
        sample = np.concatenate([np.arange(slab - 30, slab + 30), np.random.default_rng(9).integers(0, m, 300)])
        err = rel_err(a[sample, :3], direct(oracle, x[:, :3], x[:, 3], y[sample, :3]))
        print(f"tracers theta=0 N={n} M={m}: max rel acc err on {sample.size} sampled tracers {err.max():.3e}")
        assert err.max() < TOL_ACC


def test_tracers_survive_uploads_and_restore_bit_for_bit(nb):
    n = 2000
    posm, vel = bodies(nb, n)
    y0, v0 = tracer_start(posm[:, :3])
    with nb.NBodyEngine(n) as e, nb.NBodyEngine(n) as r:
        e.set_state(posm, vel); e.set_tracers(y0, v0); e.step(DT, 2)
        y, v, _ = e.tracers()
        p = e.particles()
        r.set_tracers(y, v)                                        # before any state: tracers do not need one
        r.set_particles(p)                                         # ... and an upload keeps them
        assert r.tracer_count == N_PROBES
        e.step(DT, 2); r.step(DT, 2)
        assert [q.tobytes() for q in r.tracers()] == [q.tobytes() for q in e.tracers()]
        assert r.particles().tobytes() == e.particles().tobytes()
        e.set_tracers(y0)                                          # vel None: at rest; replaces the earlier set
        assert not e.tracers()[1].any() and e.tracers()[0][:, :3].tobytes() == y0.tobytes()


# ---- theta = 1 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2000, 5000, 20000])
def test_barnes_hut_frames(nb, oracle, probe_ref, n):
    posm, vel = bodies(nb, n)
    y0, v0 = tracer_start(posm[:, :3])
    with nb.NBodyEngine(n, theta=1.0) as e, nb.NBodyEngine(n, theta=1.0) as twin:
        for x in (e, twin):
            x.set_state(posm, vel)
        e.set_tracers(y0, v0)
        root = np.zeros(3, np.float32)                             # FVector t = ZeroVector, OctreeSearch.cpp:77
        for frame in range(3):
            x_n = e.state()[0]
            y_n, v_n, _ = e.tracers()
            if frame == 1:
                e.tick(DT)                                         # (the actor's frame carries them as well)
            else:
                e.step(DT, 1)
            twin.step(DT, 1)
            y1, v1, a1 = e.tracers()
            ref, root, _ = probe_ref.field(x_n[:, :3], x_n[:, 3], y_n[:, :3], 1.0, root_origin=root)
            assert a1[:, :3].tobytes() == ref.tobytes(), (frame, int((a1[:, :3] != ref).any(axis=1).sum()))
            ry, rv = oracle.kick_drift_f32(y_n[:, :3], v_n[:, :3], a1[:, :3], DT)
            assert y1[:, :3].tobytes() == ry.tobytes() and v1[:, :3].tobytes() == rv.tobytes(), frame
            assert e.bh_stats()["root_com"].tobytes() == root.tobytes()
        assert e.particles().tobytes() == twin.particles().tobytes()
        x_n = e.state()[0]
        before = [q.tobytes() for q in e.tracers()]
        e.compute_forces()                                         # accelerations only, on a tree that belongs to no frame
        y, v, a = e.tracers()
        assert [y.tobytes(), v.tobytes()] == before[:2]
        ref, _, _ = probe_ref.field(x_n[:, :3], x_n[:, 3], y[:, :3], 1.0, root_origin=root)
        assert a[:, :3].tobytes() == ref.tobytes()


def test_frames_queued_behind_a_frame_the_warm_sort_gives_up(nb, oracle, probe_ref):
    # the scenario of tests/test_bh_gpu.py's test of the same name, with tracers: seven Ticks in three calls, the records replaced by a
    # clump in between, so that the first frame of the second call is given up and all three are queued again.  No tracer may be
    # advanced twice, or skipped, by a frame that is queued again.
    n = 8192
    rng = np.random.default_rng(77)
    posm = fuzz_scene(rng, n)
    vel = np.concatenate([rng.uniform(-20, 20, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
    q = particles_from(nb, posm, vel)
    y, v = tracer_start(posm[:, :3])
    state = {"com": None, "size": 0.0}

    def frames(k):                                                 # the same calls made frame by frame with the yardstick
        nonlocal y, v
        for _ in range(k):
            root = np.zeros(3, np.float32) if state["com"] is None else state["com"]
            a, _, _ = probe_ref.field(q["Position"], q["Mass"], y, 1.0, root_origin=root)
            y, v = oracle.kick_drift_f32(y, v, a, DT)
            state["com"], state["size"] = oracle.tick_aos_f32(q, DT, theta=1.0, root_com=state["com"], size=state["size"], pow_mode=3)

    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        e.set_tracers(y, v)
        e.step(DT, 2); frames(2)
        assert e.particles().tobytes() == q.tobytes()
        clump = (rng.uniform(-30, 30, (n - 1, 3)) + 500.0).astype(np.float32)
        assert len(np.unique(clump, axis=0)) == n - 1
        q["Position"][1:] = clump
        q["Mass"] *= np.float32(1e-4)
        e.push_particles(q)                                        # (an upload keeps the tracers)
        e.step(DT, 3); frames(3)
        assert e.particles().tobytes() == q.tobytes()
        e.step(DT, 2); frames(2)
        assert e.particles().tobytes() == q.tobytes()
        warm, retries = sort_counts(e)
        assert retries >= 1, (warm, retries)
        ty, tv, _ = e.tracers()
        assert ty[:, :3].tobytes() == y.tobytes() and tv[:, :3].tobytes() == v.tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_tracers_and_trees_deeper_than_42_levels_exclude_each_other(nb):
    n = 2000
    posm, vel = bodies(nb, n)
    y0, _ = tracer_start(posm[:, :3])
    U = nb._lib.ERR_UNSUPPORTED
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        e.set_tracers(y0)
        with pytest.raises(nb.NBodyError) as err:
            e.set_bh_max_depth(60)
        assert err.value.code == U and "tracers" in str(err.value)
        assert e.bh_max_depth() == 42
        e.set_bh_max_depth(42)                                     # (the default is no refusal)
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_state(posm, vel)
        e.set_bh_max_depth(60)
        with pytest.raises(nb.NBodyError) as err:
            e.set_tracers(y0)
        assert err.value.code == U and e.tracer_count == 0
        e.set_tracers(np.zeros((0, 3), np.float32))                # removing none is allowed
    for precision in ("f64", "f32_kahan"):
        with nb.NBodyEngine(n, precision=precision) as e:
            with pytest.raises(nb.NBodyError) as err:
                e.set_tracers(y0)
            assert err.value.code == U
