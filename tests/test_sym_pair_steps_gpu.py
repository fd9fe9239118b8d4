"""The double steps of the guided plans' symmetric fp32 kernel (csrc/kernels_sym.hip, sym_subtile_double — every guided kernel but
the general form at sixteen bodies per lane, whose cases here hold the single steps to the same checks): a lane meets TWO bodies of
a subtile per step — entries k and k + 32 of the doubled image —, the travelling j-side pair holds the sums of two different
bodies, and every body's sum comes home in two copies that are added once per subtile.  A wrong pairing, a wrong half of the
travelling pair or a wrong combination of the copies shows at single bodies (subtile entries 0, 31, 32, 63), so EVERY body is
compared with the fp64 direct sum of the oracle — same pair law (OctreeSearch.h:101-104), same `d == 0` rule (.h:102) — at
the tolerances of the other all-pairs tests (tests/test_parity_gpu.py, tests/test_even_plan_gpu.py): 2e-5 plain, 2e-6
compensated, relative to the body's acceleration or to a twentieth of the scene's median where the pulls on a body nearly
cancel.

Sizes: sixteen bodies per lane (4096-body blocks) at 12288 (three blocks, an odd ring), 16384 (an even ring with antipodal block
pairs) and 12288 + 37 (pads at 1e30 inside double steps, ragged strips) — the smallest sizes where the own-block forms P0 = 0 .. 7
and symmetric strips of a subtile count that is no multiple of four all occur; eight, four and two bodies per lane at 4096 + 37
and 8192."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_ACC = 2e-5          # asserted;  stated contract 1e-4 (tests/test_parity_gpu.py)
TOL_KAHAN = 2e-6        # the compensated passes' own tolerance (tests/test_parity_gpu.py, tests/test_even_plan_gpu.py)

SIZES = [(12288, 16), (16384, 16), (12288 + 37, 16), (4096 + 37, 8), (8192, 8), (4096 + 37, 4), (8192, 4), (4096 + 37, 2), (8192, 2)]


class env:
    def __init__(self, **kw): self.kw = {k: str(v) for k, v in kw.items()}
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def guided(nb, n, ipt, **kw):
    with env(NBODY_SYM_EVEN=0):
        e = nb.NBodyEngine(n, algorithm=2, i_per_thread=ipt, **kw)
    cfg = e.launch_config()
    assert cfg["algorithm"] == "symmetric" and cfg["plan"] == "guided" and cfg["i_per_thread"] == ipt, cfg
    return e


_scenes = {}


def scene(oracle, n, equal, ipt=16, dup=None, eps=0.0):
    """(posm, vel, fp64 accelerations of every body), made once per scene and shared (never written to)."""
    key = (n, equal, ipt if dup is not None else 0, dup, eps)
    if key not in _scenes:
        rng = np.random.default_rng(1000 * n + 2 * (0 if dup is None else len(dup)) + equal)
        posm = np.concatenate([rng.uniform(-500, 500, (n, 3)),
                               np.full((n, 1), 37.5) if equal else rng.uniform(1, 5000, (n, 1))], 1).astype(np.float32)
        vel = np.concatenate([rng.uniform(-5, 5, (n, 3)), np.zeros((n, 1))], 1).astype(np.float32)
        if dup == "blocks":            # two bodies on one point in different blocks (a symmetric strip)
            for i, j in ((5, 256 * ipt + 5), (100, n - 1), (256 * ipt - 1, 2 * 256 * ipt + 31)):
                posm[j, :3] = posm[i, :3]
        elif dup == "pair":            # ... in the slots of one register pair (512 bodies): neighbours, and the two bodies of one lane
            for i, j in ((700, 701), (1030, 1030 + 256), (n - 40, n - 8)):
                posm[j, :3] = posm[i, :3]
        elif dup == "origin":          # one body on the origin (the pads sit far away, at 1e30) — and a pair, so that the guarded loops run
            posm[n // 3, :3] = 0.0
            posm[32, :3] = posm[n // 2 + 63, :3]
        p64 = posm.astype(np.float64)
        ref = oracle.forces_direct_f64(p64[:, :3], p64[:, 3], eps=eps, nthreads=8)
        for a in (posm, vel, ref):
            a.setflags(write=False)
        _scenes[key] = (posm, vel, ref)
    return _scenes[key]


def errors(a, ref):
    na = np.linalg.norm(ref, axis=1)
    return np.linalg.norm(np.asarray(a, np.float64)[:, :3] - ref, axis=1) / np.maximum(na, 0.05 * np.median(na))


def forces_twice(e, posm, vel):
    e.set_state(posm, vel)
    e.compute_forces()
    a = e.accelerations()
    e.compute_forces()
    assert e.accelerations().tobytes() == a.tobytes()             # two passes of one state: the same bytes
    assert np.isfinite(a).all()
    return a


@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("n,ipt", SIZES)
def test_every_body_against_the_fp64_sum(nb, oracle, n, ipt, equal):
    posm, vel, ref = scene(oracle, n, equal)
    with guided(nb, n, ipt) as e:
        a = forces_twice(e, posm, vel)
        assert e.equal_mass_form() == equal
    err = errors(a, ref)
    print(f"N={n} ipt={ipt} equal={equal}: every body vs fp64: max {err.max():.2e} at body {int(err.argmax())}, median {np.median(err):.2e}")
    assert err.max() < TOL_ACC


@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("dup", ["blocks", "pair", "origin"])
@pytest.mark.parametrize("n,ipt", [(12288 + 37, 16), (4096 + 37, 8), (4096 + 37, 4), (4096 + 37, 2)])
def test_coincident_bodies_take_the_guarded_double_steps(nb, oracle, n, ipt, dup, equal):
    posm, vel, ref = scene(oracle, n, equal, ipt, dup)
    with guided(nb, n, ipt) as e:
        a = forces_twice(e, posm, vel)
    err = errors(a, ref)
    print(f"N={n} ipt={ipt} equal={equal} dup={dup}: every body vs fp64: max {err.max():.2e} at body {int(err.argmax())}")
    assert err.max() < TOL_ACC


@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("n,ipt", [(12288 + 37, 16), (16384, 16), (4096 + 37, 8), (4096 + 37, 4), (4096 + 37, 2)])
def test_softened_double_steps(nb, oracle, n, ipt, equal):
    posm, vel, ref = scene(oracle, n, equal, eps=0.5)
    with guided(nb, n, ipt, eps=0.5) as e:
        a = forces_twice(e, posm, vel)
    err = errors(a, ref)
    print(f"N={n} ipt={ipt} equal={equal} eps=0.5: every body vs fp64: max {err.max():.2e} at body {int(err.argmax())}")
    assert err.max() < TOL_ACC


@pytest.mark.parametrize("eps", [0.0, 0.5])
@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("n", [4096 + 37, 8192])
def test_compensated_sums_at_eight_bodies_per_lane(nb, oracle, n, equal, eps):
    posm, vel, ref = scene(oracle, n, equal, eps=eps)
    with guided(nb, n, 8, precision="f32_kahan", eps=eps) as e:
        a = forces_twice(e, posm, vel)
    err = errors(a, ref)
    print(f"N={n} ipt=8 kahan equal={equal} eps={eps}: every body vs fp64: max {err.max():.2e} at body {int(err.argmax())}")
    assert err.max() < TOL_KAHAN


@pytest.mark.parametrize("equal,dup", [(False, "pair"), (True, "blocks"), (True, "pair"), (False, "blocks")])
def test_compensated_sums_with_coincident_bodies(nb, oracle, equal, dup):
    n = 4096 + 37
    posm, vel, ref = scene(oracle, n, equal, 8, dup)
    with guided(nb, n, 8, precision="f32_kahan") as e:
        a = forces_twice(e, posm, vel)
    assert errors(a, ref).max() < TOL_KAHAN


@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("n,ipt", [(16384, 16), (8192, 16), (8192, 4)])
def test_two_rank_geometry_on_one_device_agrees_with_the_single_context(nb, oracle, n, ipt, equal):
    """Two contexts that own half of the bodies each (the exchange staged through the host, as tests/test_parity_gpu.py does): the
    same pairs, cut into other strips — against the single context and against the fp64 sum, at the plain tolerance."""
    posm, vel, ref = scene(oracle, n, equal)
    with guided(nb, n, ipt) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        single = e.accelerations()
    cuts = [0, n // 2, n]
    with env(NBODY_SYM_EVEN=0):
        engs = [nb.NBodyEngine(n, i_begin=cuts[r], i_count=cuts[r + 1] - cuts[r], algorithm=2, i_per_thread=ipt) for r in range(2)]
    try:
        for e in engs:
            cfg = e.launch_config()
            assert cfg["algorithm"] == "symmetric" and cfg["plan"] == "guided" and e.exchange_ranks() == 2, cfg
            e.set_state(posm, vel)
            e.step_begin()
        sends = [e.exchange_read_send() for e in engs]
        for r, e in enumerate(engs):
            e.exchange_write_recv(np.concatenate([sd[cuts[r]:cuts[r + 1]] for sd in sends]))
            e.step_end(0.01)
        a = np.concatenate([e.state()[2] for e in engs])
    finally:
        for e in engs:
            e.close()
    assert np.isfinite(a).all()
    na = np.linalg.norm(ref, axis=1)
    diff = np.linalg.norm(a[:, :3].astype(np.float64) - single[:, :3], axis=1) / np.maximum(na, 0.05 * np.median(na))
    print(f"N={n} ipt={ipt} equal={equal}: two ranks vs fp64 {errors(a, ref).max():.2e}, vs the single context {diff.max():.2e}")
    assert errors(a, ref).max() < TOL_ACC and diff.max() < TOL_ACC
