"""The yardstick of the Hermite block time steps pinned on the CPU (tests/hermite_block_ref.py; tests/test_hermite_block_gpu.py holds the
device to it), and the level rule the library exports for exactly this purpose (nbody_hermite_block_level: host only).

The scene: ic_plummer N = 257 through the scene() recipe of tests/test_hermite_gpu.py, bodies 0 and 1 replaced by
hermite_ref.kepler(0.5, a = 1) of their own masses, the pair's centre of mass at (30, 20, 10) — a binary of period 0.0225 in a cluster
whose median |a| / |j| is 0.58.  One frame of dt_max = 0.01 with 12 levels and eta = 0.02, fp64 direct sums:

    block scheme    67 block steps, active sets of 1 .. 257 bodies, 2.2e5 pair evaluations, levels 0 .. 4 occupied at the frame end
                    (0 .. 10 at begin: eta_start = 0.01), no floor hits, relative energy error 1.31e-8
    shared steps    hermite_ref.Hermite.advance at the same eta: 46 steps, 3.0e6 pair evaluations, relative energy error 3.73e-8

The energy bound of test_energy_error_of_a_frame is the measured shared-step error times 4: levels round steps down by up to a factor of
2, which pushes the error down; the inactive bodies' predictions push it up."""
import ctypes

import numpy as np
import pytest

import hermite_block_ref as B
import hermite_ref as H
from test_hermite_gpu import scene

N, DT_MAX, LEVELS, ETA = 257, 0.01, 12, 0.02
_runs = {}


def binary_scene(nb, n=N):
    posm, vel = scene(nb, n)
    p, v, _ = B.binary_in_cluster(posm, vel)
    p.setflags(write=False); v.setflags(write=False)
    return p, v


def frame(nb):
    """One frame of the scene by block steps and by shared steps, computed once: (block session, its levels and times after every block
    step, the shared-step Hermite, its step count)."""
    if "frame" not in _runs:
        p, v = binary_scene(nb)
        b = B.HermiteBlock(p, v, DT_MAX, LEVELS, eta=ETA)
        begin_levels = b.level.copy()
        trace = []
        while b.ticks < 1 << LEVELS:
            b.block_step()
            trace.append((b.ticks, b.T.copy(), b.level.copy()))
        h = H.Hermite(p, v)
        t_done, steps, _ = h.advance(DT_MAX, eta=ETA, dt_max=DT_MAX)
        assert t_done == DT_MAX
        _runs["frame"] = (b, begin_levels, trace, h, steps)
    return _runs["frame"]


def test_levels_zero_is_the_shared_step(nb):
    p, v = binary_scene(nb)
    b = B.HermiteBlock(p, v, DT_MAX, 0)
    h = H.Hermite(p, v)
    for k in range(1, 4):
        act = b.block_step()
        h.step(DT_MAX, 1)
        assert len(act) == N and b.ticks == k
        for name, got, want in (("posm", b.posm, h.posm), ("vel", b.vel, h.vel), ("a0", b.a0, h.a0), ("j0", b.j0, h.j0), ("a2", b.a2, h.a2),
                                ("a3", b.a3, h.a3)):
            assert got.tobytes() == want.tobytes(), (k, name)
    assert b.evaluations == h.evaluations == 4 and b.stats()["pairs"] == 3 * N * N


def test_times_stay_aligned_and_meet_at_the_frame_end(nb):
    b, _, trace, _, _ = frame(nb)
    for ticks, T, level in trace:
        step = np.int64(1) << (LEVELS - level).astype(np.int64)
        assert (T % step == 0).all() and (T <= ticks).all() and (ticks < T + step).all()
    ticks, T, _ = trace[-1]
    assert ticks == 1 << LEVELS and (T == ticks).all() and b.stats()["synchronised"]
    assert not any((T == t).all() for t, T, _ in trace[:-1])       # ragged everywhere else


def test_the_scene_exercises_the_scheme(nb):
    """Conditions, not measurements: a one-level scene cannot hide a failure."""
    b, begin_levels, trace, _, shared_steps = frame(nb)
    seen = set(begin_levels.tolist())
    for _, _, level in trace:
        seen |= set(level.tolist())
    print(f"block steps {b.block_steps}, sizes {min(b.sizes)} .. {max(b.sizes)}, levels seen {sorted(seen)}, pairs {b.pairs} against "
          f"{shared_steps * N * N} in {shared_steps} shared steps")
    assert len(seen) >= 4 and len(set(trace[-1][2].tolist())) >= 4
    assert min(b.sizes) <= 2 and max(b.sizes) == N
    assert b.floor_hits == 0
    assert b.pairs == sum(b.sizes) * N < shared_steps * N * N


def test_energy_error_of_a_frame(nb):
    """Measured: block 1.31e-8, shared 3.73e-8 (relative, one frame)."""
    p, v = binary_scene(nb)
    b, _, _, h, _ = frame(nb)
    e0 = B.energy(p, v)
    block = abs(B.energy(b.posm, b.vel) - e0) / abs(e0)
    shared = abs(B.energy(h.posm, h.vel) - e0) / abs(e0)
    print(f"relative energy error over one frame: block {block:.3e}, shared {shared:.3e}")
    assert block <= 4 * shared


def test_max_block_steps_and_frames(nb):
    p, v = binary_scene(nb)
    b, _, trace, _, _ = frame(nb)
    c = B.HermiteBlock(p, v, DT_MAX, LEVELS, eta=ETA)
    assert c.advance(0)["block_steps"] == 0
    st = c.advance(1, max_block_steps=5)
    assert st["block_steps"] == 5 and not st["synchronised"] and st["ticks"] == trace[4][0]
    st = c.advance(1)                                              # finishes the frame it is in
    assert st["synchronised"] and st["frames_done"] == 1 and st["block_steps"] == b.block_steps
    assert c.posm.tobytes() == b.posm.tobytes() and c.level.tobytes() == b.level.tobytes()


def lib_level(nb, dt_c, dt_max, levels):
    hit = ctypes.c_int32(-1)
    k = nb.lib().nbody_hermite_block_level(float(dt_c), float(dt_max), int(levels), ctypes.byref(hit))
    return k, bool(hit.value)


@pytest.mark.parametrize("levels", [0, 1, 12, 40])
def test_the_level_rule_against_the_numpy_loop(nb, levels):
    dt_max = np.float64(0.01)
    points = [np.inf, 0.0, -0.0, np.nan, -1.0, 5e-324, 2.2250738585072014e-308 / 4, 2.2250738585072014e-308, 1e300, dt_max * 3, dt_max * 0.75]
    for k in range(0, 44):
        e = np.ldexp(dt_max, -k)                                   # an exact power of two times dt_max, and one ulp either side
        points += [e, np.nextafter(e, 0.0), np.nextafter(e, np.inf)]
    for dt_c in points:
        want = B.level_of(np.float64(dt_c), dt_max, levels)
        assert lib_level(nb, dt_c, dt_max, levels) == want, (dt_c, levels)
    assert lib_level(nb, dt_max, dt_max, levels) == (0, False)
    assert lib_level(nb, np.ldexp(dt_max, -levels), dt_max, levels) == (levels, False)
    assert lib_level(nb, np.nextafter(np.ldexp(dt_max, -levels), 0.0), dt_max, levels) == (levels, True)
    if levels >= 1:
        assert lib_level(nb, np.nextafter(dt_max, 0.0), dt_max, levels) == (1, False)
    for dt_c in (0.0, np.nan, 5e-324):
        assert lib_level(nb, dt_c, dt_max, levels) == (levels, True)
    assert lib_level(nb, np.inf, dt_max, levels) == (0, False)


def test_the_level_rule_refuses_levels_out_of_range(nb):
    L = nb.lib()
    assert L.nbody_hermite_block_level(1.0, 1.0, -1, None) == -1 and L.nbody_hermite_block_level(1.0, 1.0, 41, None) == -1
    assert L.nbody_hermite_block_level(1.0, 1.0, 40, None) == 0    # floor_hit may be NULL
    tiny = 2.2250738585072014e-308                                  # dt_max itself the smallest normal number: deeper steps are denormals
    for dt_c in (tiny, tiny / 2, tiny / 8, 5e-324):
        assert lib_level(nb, dt_c, tiny, 40) == B.level_of(np.float64(dt_c), tiny, 40)


def test_command_line_usage_errors():
    from parallelnbody_amd.__main__ import main
    for argv in (["--integrator", "hermite-block"], ["--integrator", "hermite-block", "--precision", "f32"],
                 ["--integrator", "hermite-block", "--precision", "f64", "--levels", "41"],
                 ["--integrator", "hermite-block", "--precision", "f64", "--levels", "-1"],
                 ["--integrator", "hermite-block", "--precision", "f64", "--theta", "1.0"],
                 ["--integrator", "hermite", "--precision", "f64", "--levels", "4"], ["--levels", "4"]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2, argv
