"""nbody_get_moments and nbody_mass_within (csrc/kernels_moments.hip) against the fp64 references of tests/moments_ref.py: at every launch
geometry, in every precision, on slices, on the live buffers of every stepping path after odd step counts, on multi-device contexts, and
through the Python package and the command line.

Tolerance (derived in moments_ref.py, not measured): |S - S0| <= (n + 16) 2^-53 A for each of the 24 sums and for the masses of
nbody_mass_within, S0 = math.fsum of the fp64 terms formed from exactly the values the context holds (read back with state()), A the sum
of the absolute products.  Counts are compared for equality.  Every comparison prints its worst ratio (pytest -s)."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_ref as R
import moments_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

BLOCK_PK = "forces_block_pk_kernel"
BLOCK = "forces_block_kernel"
SYM_PK = "forces_sym_pk_kernel"
BH_SMALL = "bh_walk_compact_kernel (+ bh_small_build_kernel)"
BH_LANE = "bh_walk_lane_kernel (+ tree build)"
ABOVE_CAP = M.SLOT_CAP * M.K_BLOCK + 1              # 262145: the slots are capped, every workgroup makes a second trip


def np_dtype(prec):
    return np.float64 if prec == "f64" else np.float32


def moments_bytes(nb, e):
    """The struct as the C call fills it, byte for byte."""
    m = nb._lib.Moments()
    m.struct_size = ctypes.sizeof(m)
    assert e._L.nbody_get_moments(e._h, ctypes.byref(m)) == 0
    return bytes(m)


def mass_within_raw(nb, e, centre, radii, want_mass=True, want_count=True):
    """(rc, mass, count) of ONE nbody_mass_within call, whatever k is."""
    k = len(radii)
    c = (ctypes.c_double * 3)(*centre) if centre is not None else None
    r = (ctypes.c_double * max(k, 1))(*radii) if radii is not None else None
    mass, count = (ctypes.c_double * max(k, 1))(), (ctypes.c_int64 * max(k, 1))()
    rc = e._L.nbody_mass_within(e._h, c, r, k, mass if want_mass else None, count if want_count else None)
    return rc, np.array(mass[:k]), np.array(count[:k], np.int64)


def check_against_readback(e, prec, label):
    """moments() against the references of a readback taken at the same moment"""
    m = e.moments()
    p, v, a = e.state(np_dtype(prec))
    assert m.count == p.shape[0]
    M.assert_moments(M.flat(m), p, v, a, f"{label} {prec}")
    return m, (p, v, a)


# ---- 1. geometry ---------------------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2000, 100003, ABOVE_CAP]


@pytest.mark.parametrize("n,prec", [(n, p) for n in SIZES for p in ("f32", "f64")] + [(2049, "f32_kahan")])
def test_moments_match_the_fsum_reference_at_every_geometry(nb, n, prec):
    posm, vel = R.scene(n, n + 211, np_dtype(prec))
    with nb.NBodyEngine(n, precision=prec) as e:
        e.set_state(posm, vel)
        e.compute_forces()                                             # accelerations that are not zero
        m, (p, v, a) = check_against_readback(e, prec, f"N={n} slots x run = {M.geometry(n)}")
    np.testing.assert_array_equal(p, posm)
    assert n == 1 or np.abs(a[:, :3]).max() > 0.0
    assert m.mass > 0.0 and m.kinetic > 0.0


# ---- 2. a planted body ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [100003, ABOVE_CAP])
def test_momentum_shows_a_planted_body_wherever_it_sits(nb, n, prec):
    """One body carries 10^6 times the largest momentum any other body has (m = 5000, |v_a| = 5e6 against m <= 5000, |v_a| <= 5): at
    index 0, at the last index, and at the first and last index of a middle workgroup's run.  Losing it — or any ordinary body, whose
    momentum is far above the bound — cannot hide."""
    dt = np_dtype(prec)
    base_p, base_v = R.scene(n, n + 223, dt)
    slots, per = M.geometry(n)
    b = slots // 2
    with nb.NBodyEngine(n, precision=prec) as e:
        for i in (0, n - 1, b * per, (b + 1) * per - 1):
            posm, vel = base_p.copy(), base_v.copy()
            posm[i, 3] = 5000.0
            vel[i, :3] = (5.0e6, -5.0e6, 5.0e6)
            e.set_state(posm, vel)
            m = e.moments()
            p, v, _ = e.state(dt)
            mv = np.asarray(p, np.float64)[:, 3:4] * np.asarray(v, np.float64)[:, :3]
            s0 = np.array([math.fsum(mv[:, k].tolist()) for k in range(3)])
            big = np.array([math.fsum(np.abs(mv[:, k]).tolist()) for k in range(3)])
            print(f"moments N={n} {prec} planted at {i}: |p - p0| / (gamma A) = {(np.abs(m.p - s0) / (M.gamma(n) * big)).max():.3e}")
            assert np.all(np.abs(m.p) > 2.4e10) and np.all(np.abs(m.p - s0) <= M.gamma(n) * big)
            assert M.gamma(n) * big.max() < 1.0                        # the bound is far below one ordinary body's momentum


# ---- 3. slices -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,cuts", [(5000, (0, 1999, 4001, 5000)), (8193, (0, 4096, 8193))])
def test_moments_of_slices_are_the_owned_bodies_shares(nb, n, cuts, prec):
    dt = np_dtype(prec)
    posm, vel = R.scene(n, n + 227, dt)
    with nb.NBodyEngine(n, precision=prec) as e:
        e.set_state(posm, vel)
        e.compute_forces()
        whole, (p, v, a) = check_against_readback(e, prec, f"N={n} whole")
    _, big = M.reference(p, v, a)
    total = np.zeros(24)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        with nb.NBodyEngine(n, precision=prec, i_begin=lo, i_count=hi - lo) as e:
            e.set_state(posm, vel)
            e.compute_forces()
            share, (ps, vs, as_) = check_against_readback(e, prec, f"N={n} slice [{lo},{hi})")
            assert share.count == hi - lo
            np.testing.assert_array_equal(ps, posm[lo:hi])              # posm by the global index, vel and acc by the local one
            np.testing.assert_array_equal(vs, vel[lo:hi])
            total += M.flat(share)
    err = np.abs(total - M.flat(whole))
    print(f"moments N={n} {prec}: shares against the whole, worst |diff| / (gamma A) = {(err / (M.gamma(n) * big)).max():.3e}")
    assert (err <= M.gamma(n) * big).all()


# ---- 4. live buffers after odd step counts -------------------------------------------------------------------------------------------

def _moments_follow_the_steps(nb, e, prec, posm, vel, kernel, label, held=False):
    assert e.launch_config()["kernel"] == kernel
    e.set_state(posm, vel)
    if held:
        e.device_ptr(nb.BUF_POSM)                                      # the caller holds the buffer: two launches per step from here on
    last = posm
    for done, more in ((1, 1), (3, 2)):
        e.step(0.01, more)
        m, (p, v, a) = check_against_readback(e, prec, f"{label} after {done} steps")
        assert e.steps_done() == done and not np.array_equal(p, last) and np.abs(a[:, :3]).max() > 0.0
        last = p
        mass, count = e.mass_within((0.0, 0.0, 0.0), [250.0])
        m0, c0, big = M.mass_within(p, (0.0, 0.0, 0.0), [250.0])
        assert count[0] == c0[0] and abs(mass[0] - m0[0]) <= M.gamma(p.shape[0]) * big[0]


@pytest.mark.parametrize("held", [False, True])
def test_moments_after_odd_step_counts_one_launch_step(nb, held):
    n = 2560
    posm, vel = R.scene(n, n + 31)
    with nb.NBodyEngine(n) as e:
        _moments_follow_the_steps(nb, e, "f32", posm, vel, BLOCK_PK, f"N={n} one-launch step held={held}", held)


@pytest.mark.parametrize("prec", ["f32_kahan", "f64"])
def test_moments_after_odd_step_counts_block_kernel(nb, prec):
    n = 2001
    posm, vel = R.scene(n, n + 37, np_dtype(prec))
    with nb.NBodyEngine(n, precision=prec) as e:
        _moments_follow_the_steps(nb, e, prec, posm, vel, BLOCK, f"N={n} block kernel")


@pytest.mark.parametrize("equal", [True, False])
def test_moments_after_odd_step_counts_fused_symmetric_step(nb, equal):
    n = 24576
    posm, vel = R.scene(n, n + 41, equal=equal)
    with nb.NBodyEngine(n) as e:
        assert e.launch_config()["algorithm"] == "symmetric"
        _moments_follow_the_steps(nb, e, "f32", posm, vel, SYM_PK, f"N={n} symmetric step equal={equal}")


@pytest.mark.parametrize("n,kernel", [(2000, BH_SMALL), (5000, BH_LANE)])
def test_moments_after_odd_step_counts_barnes_hut(nb, n, kernel):
    posm, vel = R.scene(n, n + 43)
    with nb.NBodyEngine(n, theta=1.0) as e:
        _moments_follow_the_steps(nb, e, "f32", posm, vel, kernel, f"N={n} theta=1")


@pytest.mark.parametrize("n,lo,hi", [(2000, 700, 1500), (5000, 1999, 4001)])
def test_moments_of_a_barnes_hut_slice_follow_both_ways_of_stepping(nb, n, lo, hi):
    """A theta > 0 slice walks into a buffer of its own on the phased path (nbody_step_begin) and stores the accelerations with
    nbody_step_end; nbody_step's frame stores them itself.  Either way the moments are those of what the getters deliver."""
    posm, vel = R.scene(n, n + 47)
    with nb.NBodyEngine(n, theta=1.0, i_begin=lo, i_count=hi - lo) as e:
        e.set_state(posm, vel)
        e.step(0.01, 1)
        _, (_, _, a1) = check_against_readback(e, "f32", f"N={n} theta=1 slice [{lo},{hi}) after nbody_step")
        e.step_begin()
        check_against_readback(e, "f32", f"N={n} theta=1 slice between step_begin and step_end")   # still the stored ones
        e.step_end(0.01)
        _, (_, _, a2) = check_against_readback(e, "f32", f"N={n} theta=1 slice after step_begin / step_end")
        assert np.abs(a1[:, :3]).max() > 0.0 and not np.array_equal(a1, a2)
        e.compute_forces()
        check_against_readback(e, "f32", f"N={n} theta=1 slice after compute_forces")


# ---- 5. physics, from the project's own tolerance ------------------------------------------------------------------------------------

def test_net_force_and_virial_of_a_pair_sum_and_of_the_monopole_walk(nb):
    """theta = 0: the pair sum's net force vanishes and the Clausius virial is the potential energy, both to the 2e-5 per-body
    acceleration tolerance test_parity_gpu.py holds the kernels to.  theta = 1 is the reference's algorithm: its residuals are printed
    (and recorded in DESIGN.md), not asserted."""
    g = np.load(os.path.join(GOLDEN, "plummer_n1024_seed1.npz"))
    n = g["posm"].shape[0]
    for theta in (0.0, 1.0):
        with nb.NBodyEngine(n, eps=0.0, theta=theta) as e:
            e.set_state(g["posm"], g["vel"])
            e.compute_forces()
            m, (p, v, a) = check_against_readback(e, "f32", f"plummer N={n} theta={theta}")
            ke, pe = e.energy()
        p64, a64 = np.asarray(p, np.float64), np.asarray(a, np.float64)
        ma = float((p64[:, 3] * np.linalg.norm(a64[:, :3], axis=1)).sum())
        mxa = float((p64[:, 3] * np.linalg.norm(p64[:, :3], axis=1) * np.linalg.norm(a64[:, :3], axis=1)).sum())
        f, t = float(np.linalg.norm(m.force)), float(np.linalg.norm(m.torque))
        print(f"plummer N={n} theta={theta}: |force| / sum m|a| = {f / ma:.3e}, |torque| / sum m|x||a| = {t / mxa:.3e}, "
              f"|virial - pe| / sum m|x||a| = {abs(m.virial - pe) / mxa:.3e}, virial {m.virial:.9e}, pe {pe:.9e}")
        assert m.kinetic == pytest.approx(ke, rel=1e-12)
        if theta == 0.0:
            assert f <= 2e-5 * ma
            assert abs(m.virial - pe) <= 2e-5 * mxa


# ---- 6. nbody_mass_within ------------------------------------------------------------------------------------------------------------

CENTRES = [(0.0, 0.0, 0.0), (12.345678901234567, -7.1122334455667788, 3.3000000000000003)]


def radii_for(posm, centre):
    """64 radii from 0 to beyond the farthest body: 0 itself, a radius EQUAL to a body's fp64 distance whose square is that body's d2
    again (the body sits on the <= boundary) next to the double just below it, two equal radii, not sorted."""
    d2 = M.distances2(posm, centre)
    r = np.sqrt(d2)
    on = np.flatnonzero((r * r == d2) & (d2 > 0))
    assert on.size > 0
    j = int(on[on.size // 2])
    far = float(r.max())
    radii = list(np.linspace(0.0, 1.25 * far, 60)) + [float(r[j]), float(np.nextafter(r[j], 0.0)), 0.5 * far, 0.5 * far]
    radii = np.array(radii)[np.random.default_rng(3).permutation(64)]
    return radii, j, float(r[j])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [2000, 100003])
def test_mass_within_counts_are_numpys_and_masses_within_the_bound(nb, n, prec):
    posm, vel = R.scene(n, n + 229, np_dtype(prec))
    with nb.NBodyEngine(n, precision=prec) as e:
        e.set_state(posm, vel)
        for centre in CENTRES:
            radii, j, rj = radii_for(posm, centre)
            rc, mass, count = mass_within_raw(nb, e, centre, radii)                   # k = 64, one call
            assert rc == 0
            m0, c0, big = M.mass_within(posm, centre, radii)
            np.testing.assert_array_equal(count, c0)
            err = np.abs(mass - m0)
            print(f"mass_within N={n} {prec} centre {centre[0]:g}: worst |m - m0| / (gamma A) = "
                  f"{np.where(big > 0, err / np.maximum(M.gamma(n) * big, 1e-300), 0.0).max():.3e}")
            assert (err <= M.gamma(n) * big).all()
            assert count.max() == n and c0[radii == 0.0][0] == (1 if centre == CENTRES[0] and n > 3 else 0)
            at, below = int(np.flatnonzero(radii == rj)[0]), int(np.flatnonzero(radii == np.nextafter(rj, 0.0))[0])
            assert count[at] >= count[below] + 1                                       # the body on the boundary is inside
            twins = np.flatnonzero(radii == radii[np.argsort(radii)][np.flatnonzero(np.diff(np.sort(radii)) == 0)[0]])
            assert twins.size == 2 and mass[twins[0]] == mass[twins[1]] and count[twins[0]] == count[twins[1]]
            # independent of the order of the radii and of how many there are, bit for bit
            perm = np.random.default_rng(11).permutation(64)
            rc, mass_p, count_p = mass_within_raw(nb, e, centre, radii[perm])
            assert rc == 0 and mass_p.tobytes() == mass[perm].tobytes() and count_p.tobytes() == count[perm].tobytes()
            for q in (at, int(np.argmax(radii))):
                rc, m1, c1 = mass_within_raw(nb, e, centre, radii[q:q + 1])            # k = 1
                assert rc == 0 and m1.tobytes() == mass[q:q + 1].tobytes() and c1[0] == count[q]
            for k in (16, 17):                                                          # either side of the two register budgets
                rc, mk, ck = mass_within_raw(nb, e, centre, radii[:k])
                assert rc == 0 and mk.tobytes() == mass[:k].tobytes() and ck.tobytes() == count[:k].tobytes()
            # either output alone
            rc, only_m, _ = mass_within_raw(nb, e, centre, radii, want_count=False)
            assert rc == 0 and only_m.tobytes() == mass.tobytes()
            rc, _, only_c = mass_within_raw(nb, e, centre, radii, want_mass=False)
            assert rc == 0 and only_c.tobytes() == count.tobytes()
        if n != 2000:
            return
        # any number of radii through the package, in batches of 64
        many = np.linspace(0.0, 900.0, 150).reshape(3, 50)
        mass, count = e.mass_within(CENTRES[1], many)
        m0, c0, big = M.mass_within(posm, CENTRES[1], many)
        assert mass.shape == count.shape == (3, 50) and count.dtype == np.int64
        np.testing.assert_array_equal(count.reshape(-1), c0)
        assert (np.abs(mass.reshape(-1) - m0) <= M.gamma(n) * big).all()


def test_mass_within_refuses_bad_arguments(nb):
    n = 300
    posm, vel = R.scene(n, 17)
    INVALID, STATE = nb._lib.ERR_INVALID, nb._lib.ERR_STATE
    with nb.NBodyEngine(n) as e:
        assert mass_within_raw(nb, e, (0, 0, 0), [1.0])[0] == STATE                   # no particles set
        m = nb._lib.Moments()
        m.struct_size = ctypes.sizeof(m)
        assert e._L.nbody_get_moments(e._h, ctypes.byref(m)) == STATE
        e.set_state(posm, vel)
        assert mass_within_raw(nb, e, (0, 0, 0), [1.0] * 64)[0] == 0
        assert mass_within_raw(nb, e, (0, 0, 0), [])[0] == INVALID                    # k = 0
        assert mass_within_raw(nb, e, (0, 0, 0), [1.0] * 65)[0] == INVALID
        assert mass_within_raw(nb, e, (0, 0, 0), [1.0, -1e-300])[0] == INVALID
        assert mass_within_raw(nb, e, (0, 0, 0), [float("nan")])[0] == INVALID
        assert mass_within_raw(nb, e, (0, 0, 0), [1.0, float("inf")])[0] == INVALID
        assert mass_within_raw(nb, e, None, [1.0])[0] == INVALID
        assert mass_within_raw(nb, e, (0, 0, 0), [1.0], want_mass=False, want_count=False)[0] == INVALID
        assert e._L.nbody_mass_within(e._h, (ctypes.c_double * 3)(), None, 1, (ctypes.c_double * 1)(), None) == INVALID
        m.struct_size = 207
        assert e._L.nbody_get_moments(e._h, ctypes.byref(m)) == INVALID
        assert e._L.nbody_get_moments(e._h, None) == INVALID
        assert b"struct_size" in e._L.nbody_last_error(e._h)
        rc, mass, count = mass_within_raw(nb, e, (0, 0, 0), [0.0])                    # -0.0 and 0 are radii like any other
        assert rc == 0 and count[0] == 1 and mass[0] == float(posm[0, 3])
        assert mass_within_raw(nb, e, (0, 0, 0), [-0.0])[2][0] == 1


# ---- 7. determinism, no side effects, tracers ----------------------------------------------------------------------------------------

def getters(nb, e, theta):
    p, v, a = e.state()
    out = [p.tobytes(), v.tobytes(), a.tobytes(), e.particles().tobytes(), e.steps_done(), e.kernel_time(nb.KERNEL_FORCES),
           e.kernel_time(nb.KERNEL_UPDATE), e.tracers()[0].tobytes(), e.tracers()[2].tobytes()]
    if theta > 0.0:
        s = e.bh_stats()
        out += [s["nodes"], s["levels"], s["root_com"].tobytes(), e.bh_leaf_order().tobytes()]
    return out


@pytest.mark.parametrize("theta", [0.0, 1.0])
def test_two_calls_give_equal_bytes_and_change_nothing_and_tracers_are_not_summed(nb, theta):
    n = 2000
    posm, vel = R.scene(n, n + 233)
    rng = np.random.default_rng(5)
    tr_pos = rng.uniform(-450, 450, (777, 3)).astype(np.float32)
    tr_vel = rng.uniform(-5, 5, (777, 3)).astype(np.float32)
    radii = list(np.linspace(0.0, 900.0, 20))
    seen = []
    for tracers in (False, True):
        with nb.NBodyEngine(n, theta=theta, time_kernels=True) as e:
            e.set_state(posm, vel)
            if tracers:
                e.set_tracers(tr_pos, tr_vel)
                assert e.tracer_count == 777
            e.step(0.01, 3)
            before = getters(nb, e, theta)
            first = moments_bytes(nb, e)
            rc, mass, count = mass_within_raw(nb, e, CENTRES[1], radii)
            assert rc == 0
            assert moments_bytes(nb, e) == first
            again = mass_within_raw(nb, e, CENTRES[1], radii)
            assert again[0] == 0 and again[1].tobytes() == mass.tobytes() and again[2].tobytes() == count.tobytes()
            assert getters(nb, e, theta) == before                    # the timers too: neither call is a force pass or an update
            assert before[5][1] == 3
            seen.append((first, mass.tobytes(), count.tobytes(), before[:3]))
    assert seen[0] == seen[1]


# ---- 8. multi-device contexts --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "fake_rccl.c"), "-o", so, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib"])
    return so


@pytest.fixture
def parts_env(fake_rccl, monkeypatch):
    monkeypatch.setenv("NBODY_RCCL_LIB", fake_rccl)
    monkeypatch.setenv("NBODY_MULTI_SHARE_DEVICE", "1")


@pytest.mark.parametrize("theta", [0.0, 1.0])
@pytest.mark.parametrize("parts", [1, 2, 4])
def test_multi_device_moments_are_the_part_order_sum_of_the_shares(nb, parts_env, parts, theta):
    n = 4096
    posm, vel = R.scene(n, n + 239)
    radii = list(np.linspace(0.0, 2000.0, 33))
    with nb.NBodyEngine(n, theta=theta) as one, nb.NBodyEngine(n, theta=theta, devices=[0] * parts) as many:
        for e in (one, many):
            e.set_state(posm, vel)
            e.step(0.01, 3)
        m_many, (p, v, a) = check_against_readback(many, "f32", f"N={n} theta={theta} {parts} parts")
        assert np.abs(a[:, :3]).max() > 0.0
        got = moments_bytes(nb, many)
        rc, mass, count = mass_within_raw(nb, many, CENTRES[1], radii)
        assert rc == 0
        if parts == 1:                                                 # one part: nbody_create's result, bit for bit
            np.testing.assert_array_equal(one.particles(), many.particles())
            assert got == moments_bytes(nb, one)
            r1 = mass_within_raw(nb, one, CENTRES[1], radii)
            assert r1[1].tobytes() == mass.tobytes() and r1[2].tobytes() == count.tobytes()
            return
        records = many.particles()                                     # Mass, Position, Velocity and the stored Acceleration
        m_one = one.moments()
    # the same records in slice contexts: their shares, added in part order in fp64, are the multi-device result in every bit
    ic = n // parts
    total, mass_sum, count_sum = None, None, None
    for k in range(parts):
        with nb.NBodyEngine(n, theta=theta, i_begin=k * ic, i_count=ic) as e:
            e.set_particles(records)
            share = M.flat(e.moments())
            rc, ms, cs = mass_within_raw(nb, e, CENTRES[1], radii)
            assert rc == 0
        total = share if total is None else total + share
        mass_sum = ms if mass_sum is None else mass_sum + ms
        count_sum = cs if count_sum is None else count_sum + cs
    assert M.flat(m_many).tobytes() == total.tobytes()
    assert mass.tobytes() == mass_sum.tobytes() and count.tobytes() == count_sum.tobytes()
    np.testing.assert_array_equal(count, M.mass_within(p, CENTRES[1], radii)[1])   # (close encounters fling a few bodies out of any fixed radius)
    assert m_many.count == n
    # ... and the single context's within the bound (theta = 0: the parts' step is the same all-pairs sum; theta = 1: the same frames)
    _, big = M.reference(p, v, a)
    assert (np.abs(M.flat(m_many) - M.flat(m_one)) <= M.gamma(n) * big).all()


# ---- 9. the Python package and the command line --------------------------------------------------------------------------------------

def test_derived_fields_against_numpy(nb):
    n = 2000
    posm, vel = R.scene(n, n + 241, np.float64)
    vel[:, :3] += (3.0, -1.0, 0.5)                                     # a centre-of-mass motion worth the name
    with nb.NBodyEngine(n, precision="f64") as e:
        e.set_state(posm, vel)
        e.compute_forces()
        m = e.moments()
        p, v, a = e.state(np.float64)
    mass = p[:, 3]
    com = (mass[:, None] * p[:, :3]).sum(0) / mass.sum()
    vcom = (mass[:, None] * v[:, :3]).sum(0) / mass.sum()
    l_com = (mass[:, None] * np.cross(p[:, :3] - com, v[:, :3] - vcom)).sum(0)
    assert isinstance(m.mass, float) and m.mx.shape == m.p.shape == m.l.shape == m.force.shape == m.torque.shape == (3,)
    assert m.second.shape == (6,) and m.count == n
    np.testing.assert_allclose(m.com, com, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(m.com_velocity, vcom, rtol=1e-12)
    np.testing.assert_allclose(m.l_about_com, l_com, rtol=1e-9)
    np.testing.assert_array_equal(m.com, m.mx / m.mass)
    np.testing.assert_array_equal(m.l_about_com, m.l - np.cross(m.com, m.p))


TIMING_KEYS = ("wall_s", "frames_per_s", "pair_interactions_per_s")


def test_command_line_moments_every(nb):
    """--moments-every K prints one parsable line per mark; without the flag the run prints what it printed before — the same lines
    in the same order, every figure of the simulation equal (the closing line's wall-clock figures are the only ones a second run of
    the same command changes, and are left out of the comparison)."""
    base = [sys.executable, "-m", "parallelnbody_amd", "--n", "2000", "--steps", "6", "--energy-every", "3"]

    def run(extra):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines(), out.stderr

    plain, err0 = run([])
    with_m, err1 = run(["--moments-every", "2"])
    assert err0 == err1
    assert not any("moments" in ln for ln in plain)
    marks = [json.loads(ln) for ln in with_m if "moments" in ln]
    assert [r["frame"] for r in marks] == [2, 4, 6]
    for r in marks:
        mm = r["moments"]
        assert set(mm) == {"P", "L", "com", "net_force", "net_torque", "virial"} and len(mm["com"]) == 3
        assert all(math.isfinite(x) for x in [mm["P"], mm["L"], mm["net_force"], mm["net_torque"], mm["virial"], *mm["com"]])
        assert mm["P"] > 0 and mm["L"] > 0 and mm["net_force"] >= 0      # (the virial of a(x_n) beside x_(n+1) has either sign)
    rest = [ln for ln in with_m if "moments" not in ln]
    assert len(rest) == len(plain) == 3
    assert rest[:-1] == plain[:-1]                                     # the energy lines: byte for byte
    a, b = json.loads(rest[-1]), json.loads(plain[-1])
    assert list(a) == list(b)
    assert {k: x for k, x in a.items() if k not in TIMING_KEYS} == {k: x for k, x in b.items() if k not in TIMING_KEYS}


# ---- 10. ShardedSimulation -----------------------------------------------------------------------------------------------------------

def test_sharded_simulation_moments_at_world_size_one():
    """(two ranks: tests/test_moments_abi.py runs the all-reduce over gloo with a numpy stand-in for the engine.)  In a process of its
    own, as every ShardedSimulation run on the GPU: torch brings its HIP runtime up first there."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "sharded_moments_worker.py")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "sharded moments at world size 1: ok" in out.stdout
