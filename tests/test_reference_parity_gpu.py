"""The device against what the REFERENCE's own compiled code wrote (tests/golden/reference_*.npz, recorded from oracle/_ref/nbody_ref by
tests/golden/make_reference_golden.py; tests/test_reference_build.py keeps the files current).  The other Barnes-Hut tests compare with
the oracle, a restatement by reading; these compare with recorded results of the thing restated.  They read the fixtures only — never the
reference, never oracle/_ref/.

And integration/ue4/OctreeSearch.cpp — the drop-in this project ships — compiled, linked against libnbody_amd and run: the same
driver that produced the fixtures (oracle/ref_driver.cpp) around the adapter's AOctreeSearch instead of the reference's."""
import os
import subprocess

import numpy as np
import pytest

import reference_scenes as S
from conftest import rel_err
from test_parity_gpu import TOL_ACC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _stored(fx, frames_key, key, frame):
    at = np.flatnonzero(fx[frames_key] == frame)
    return fx[key][at[0]] if len(at) else None


@pytest.mark.parametrize("name", list(S.SCENES))
def test_tick_frames_equal_the_reference(nb, name):
    fx, q0 = S.load(name), S.inputs(name)
    n = len(q0)
    with nb.NBodyEngine(n, theta=1.0) as e:
        e.set_particles(q0)
        for frame in range(1, S.SCENES[name] + 1):
            size, out = e.tick(float(fx["dt"]))
            assert _same(np.float32(size), fx["size"][frame - 1]), frame
            assert _same(e.bh_stats()["root_com"], fx["com"][frame - 1]), frame
            want = _stored(fx, "record_frames", "records", frame)
            if want is not None:
                assert out.tobytes() == want.tobytes(), frame               # every byte of the FParticle records
            order = _stored(fx, "draw_frames", "order", frame)
            if order is not None:                                           # what DrawOctreeBoxes drew, and in which order
                assert _same(e.bh_leaf_order(), order), frame
                assert _same(e.bh_leaf_boxes()[order], _stored(fx, "draw_frames", "boxes", frame)), frame
    assert len(fx["record_frames"]) and len(fx["draw_frames"])


@pytest.mark.parametrize("name", list(S.SCENES))
def test_step_frames_equal_the_reference(nb, name):
    # the same frames through the calls a host makes that wants no record per frame: bounds / step / particles()
    fx, q0 = S.load(name), S.inputs(name)
    with nb.NBodyEngine(len(q0), theta=1.0) as e:
        e.set_particles(q0)
        for frame in range(1, S.SCENES[name] + 1):
            assert _same(np.float32(e.bounds()), fx["size"][frame - 1]), frame   # ComputeCubeSize of the positions the frame starts from
            e.step(float(fx["dt"]), 1)
            assert _same(e.bh_stats()["root_com"], fx["com"][frame - 1]), frame
            want = _stored(fx, "record_frames", "records", frame)
            if want is not None:
                assert e.particles().tobytes() == want.tobytes(), frame


@pytest.mark.parametrize("name", S.FORCES)
def test_all_pairs_kernels_against_the_reference_at_theta_0(nb, name):
    # the reference's own Octree at theta = 0 visits every leaf: its all-pairs answer in ITS summation order.  The all-pairs kernels add
    # in another order, so no byte equality: the project's tolerance per body.
    want = S.load("forces_theta0")["acc_" + name]
    q0 = S.inputs(name)
    with nb.NBodyEngine(len(q0), theta=0.0) as e:
        e.set_particles(q0)
        e.compute_forces()
        a = e.accelerations()
    err = rel_err(a, want)
    print(f"{name}: max per-body relative error against the reference's theta = 0 accelerations {err.max():.3e}")
    assert np.all(np.linalg.norm(want, axis=1) > 0)
    assert err.max() < TOL_ACC


@pytest.fixture(scope="module")
def adapter_program(nb, tmp_path_factory):
    """oracle/ref_driver.cpp + integration/ue4/OctreeSearch.cpp against the stand-in engine headers and include/, linked with
    libnbody_amd as tests/test_cpp_actor_gpu.py links its program."""
    from oracle import reference as R
    standin = os.path.join(ROOT, "oracle", "ue4_standin")
    lib_dir = os.path.join(ROOT, "parallelnbody_amd")
    exe = str(tmp_path_factory.mktemp("adapter") / "nbody_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-DNBODY_DRIVER_ADAPTER",
                           "-I", os.path.join(standin, "module"), "-I", standin, "-I", os.path.join(ROOT, "integration", "ue4"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "oracle", "ref_driver.cpp"), os.path.join(ROOT, "integration", "ue4", "OctreeSearch.cpp"),
                           "-o", exe, "-L", lib_dir, "-lnbody_amd", "-Wl,-rpath," + lib_dir])
    return R, exe


@pytest.mark.parametrize("name", ["refbox_n2000", "n300"])
def test_the_ue4_adapter_compiled_and_run_equals_the_reference(adapter_program, name):
    R, exe = adapter_program
    fx, q0 = S.load(name), S.inputs(name)
    n, frames = len(q0), S.SCENES[name]
    with_boxes, points_only = R.run(q0, [R.ticks_command(float(fx["dt"]), frames, True), R.ticks_command(float(fx["dt"]), frames, False)],
                                    binary=exe)             # (a child process under reference.TIME_LIMIT; non-zero status raises)
    for frame in range(1, frames + 1):
        got = with_boxes[frame - 1]
        assert _same(got["size"], fx["size"][frame - 1]), frame
        want = _stored(fx, "record_frames", "records", frame)
        boxes, points = R.draw_sequence(got["calls"])       # (asserts the interleaving: box, point, box, point ...)
        assert len(points) == n and len(boxes) == n
        if want is not None:
            assert got["records"].tobytes() == want.tobytes(), frame
            assert points_only[frame - 1]["records"].tobytes() == want.tobytes(), frame
        order = _stored(fx, "draw_frames", "order", frame)
        if order is not None:
            assert _same(boxes, _stored(fx, "draw_frames", "boxes", frame)), frame
            assert _same(points, got["records"]["Position"][order]), frame
            no_boxes, same_points = R.draw_sequence(points_only[frame - 1]["calls"])
            assert len(no_boxes) == 0 and _same(same_points, points), frame
