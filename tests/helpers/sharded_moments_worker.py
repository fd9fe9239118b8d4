"""Child process of tests/test_moments_gpu.py: ShardedSimulation.moments() / .mass_within() on the HIP engine at world size 1, in a
process of its own as every other ShardedSimulation run on the GPU (torch brings its HIP runtime up first there)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import diagnostics_ref as R  # noqa: E402
import moments_ref as M  # noqa: E402
import parallelnbody_amd as nb  # noqa: E402

n = 4096
posm, vel = R.scene(n, n + 251)
sim = nb.ShardedSimulation(posm, vel, device="cuda:0")
try:
    sim.step(0.01, 3)
    m = sim.moments()
    p, v, a = sim.engine.state()
    assert np.abs(a[:, :3]).max() > 0.0 and not np.array_equal(p, posm)
    M.assert_moments(M.flat(m), p, v, a, f"ShardedSimulation N={n}")
    assert m.count == n and M.flat(m).tobytes() == M.flat(sim.engine.moments()).tobytes()
    centre = (12.345678901234567, -7.1122334455667788, 3.3000000000000003)
    radii = np.linspace(0.0, 900.0, 70)
    mass, count = sim.mass_within(centre, radii)
    m0, c0, big = M.mass_within(p, centre, radii)
    np.testing.assert_array_equal(count, c0)
    assert (np.abs(mass - m0) <= M.gamma(n) * big).all()
finally:
    sim.close()
print("sharded moments at world size 1: ok")
