"""Scenes and point sets the field-query and tracer tests share (tests/test_field_gpu.py, tests/test_tracers_gpu.py).  TEST
INFRASTRUCTURE ONLY."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_ACC = 2e-5               # tests/test_parity_gpu.py: all-pairs parity
N_PROBES = 777

_scenes = {}


def bodies(nb, n):
    """(posm, vel): the golden shipped scene at N = 2000, else ic_reference_box(n, 1000, seed=n)."""
    if n not in _scenes:
        if n == 2000:
            g = np.load(os.path.join(GOLDEN, "refbox_n2000_seed1.npz"))
            _scenes[n] = (np.ascontiguousarray(g["posm"], np.float32), np.ascontiguousarray(g["vel"], np.float32))
        else:
            _scenes[n] = nb.ic_reference_box(n, 1000.0, seed=n)
    return _scenes[n]


def probes_for(pos, m):
    """m points from default_rng(7): x, y uniform +-1500, z uniform +-300; where there is room, points 0-49 ON bodies 0-49 and
    points 50-59 1e-3 beside bodies 100-109 (fewer points: point 0 on body 0 when there are two or more)."""
    rng = np.random.default_rng(7)
    p = np.stack([rng.uniform(-1500, 1500, m), rng.uniform(-1500, 1500, m), rng.uniform(-300, 300, m)], 1).astype(np.float32)
    if m >= 60 and pos.shape[0] >= 110:
        p[:50] = pos[:50]
        p[50:60] = pos[100:110] + np.float32(1e-3)
    elif m >= 2:
        p[0] = pos[0]
    return p


def direct_at(oracle, pos, mass, pts, eps=0.0):
    """The oracle's fp32 direct sum at `pts`: the points appended to the bodies as zero-mass rows (they change no body's row, and a
    point's row is the direct sum over the bodies)."""
    n, m = pos.shape[0], pts.shape[0]
    return oracle.forces_direct_f32(np.concatenate([pos, pts]), np.concatenate([mass, np.zeros(m, np.float32)]), eps=eps, i0=n, i1=n + m)


# (the scene generator and the sort counters of tests/test_bh_gpu.py, restated: the give-up scenario is replayed with tracers)
def fuzz_scene(rng, n):
    """A scene with structure at every scale: a few clumps of very different widths (deep, narrow subtrees: chains of
    single-child cells, cells that reach across many 256-body chunks), a uniform background, masses over three decades."""
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


def sort_counts(e):
    import ctypes
    warm, retries = ctypes.c_longlong(), ctypes.c_longlong()
    assert e._L.nbody_debug_bh_sort_counts(e._h, ctypes.byref(warm), ctypes.byref(retries)) == 0
    return warm.value, retries.value
