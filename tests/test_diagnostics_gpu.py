"""nbody_energy and nbody_get_bounds (energy_kernel, energy_fold_kernel, bounds_kernel: csrc/kernels.hip) against fp64 references
at every geometry they launch with, in every precision, on slices, on Barnes-Hut contexts, and on the live buffers of every
stepping path after odd step counts.

The energy reference is the oracle's fp64 pair sum (oracle_energy_f64) — for slices the per-body shares of tests/diagnostics_ref.py,
themselves pinned to the oracle on the CPU below — evaluated on exactly the values the context holds (float32 widened to double
for the fp32 contexts).  Both sides add the same fp64 terms in different orders, the device's reciprocal square root is good to
the last bits: |ke - ke0| <= 1e-12 |ke0| and |pe - pe0| <= 1e-10 |pe0|, the bounds of test_energy_diagnostic.  Bounds are
compared for equality: the kernel casts every coordinate to float before it compares, and rounding is monotonic.

Every energy comparison prints its errors and the worst so far per precision (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest

import diagnostics_ref as R

gpu = pytest.mark.gpu          # every test that needs the device; the references' own test below runs anywhere

KE_TOL = 1e-12
PE_TOL = 1e-10
BLOCK_PK = "forces_block_pk_kernel"
BLOCK = "forces_block_kernel"
SYM_PK = "forces_sym_pk_kernel"
BH_SMALL = "bh_walk_compact_kernel (+ bh_small_build_kernel)"
BH_LANE = "bh_walk_lane_kernel (+ tree build)"

WORST = {}                     # precision -> [worst ke error, worst pe error] seen by check_energy


def np_dtype(prec):
    return np.float64 if prec == "f64" else np.float32


def oracle_energy(oracle, posm, vel, eps):
    p = np.asarray(posm, np.float64)
    v = np.asarray(vel, np.float64)
    return oracle.energy_f64(p[:, :3], v[:, :3], p[:, 3], eps=eps, nthreads=8)


def check_energy(label, prec, got, ref, ke_tol=KE_TOL, pe_tol=PE_TOL):
    (ke, pe), (ke0, pe0) = got, ref
    dk = abs(ke - ke0) / abs(ke0) if ke0 != 0.0 else abs(ke)
    dp = abs(pe - pe0) / abs(pe0) if pe0 != 0.0 else abs(pe)
    w = WORST.setdefault(prec, [0.0, 0.0])
    w[0], w[1] = max(w[0], dk), max(w[1], dp)
    print(f"energy {label} {prec}: ke rel err {dk:.3e}, pe rel err {dp:.3e}   (worst so far in {prec}: ke {w[0]:.3e}, pe {w[1]:.3e})")
    assert math.isfinite(ke) and math.isfinite(pe), (label, ke, pe)
    assert abs(ke - ke0) <= ke_tol * abs(ke0), (label, ke, ke0)
    assert abs(pe - pe0) <= pe_tol * abs(pe0), (label, pe, pe0)


def expected_bounds(oracle, pos, prec):
    if prec == "f64":
        return float(np.float32(np.abs(np.asarray(pos, np.float64)[:, :3]).max()))
    return oracle.bounds_f32(np.ascontiguousarray(np.asarray(pos)[:, :3], np.float32))


def hip_runtime():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


# ---- the references themselves (no GPU) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.7])
def test_numpy_energy_shares_add_up_to_the_oracle_pair(oracle, eps):
    n, cuts = 1500, [0, 499, 1001, 1500]
    posm, vel = R.scene(n, 1500 + 3)
    posm[700, :3] = posm[40, :3]                                       # a coincident pair: skipped at eps = 0, counted at eps > 0
    posm[90, 3] = 0.0
    shares = R.energy_shares(posm, vel, cuts, eps=eps)
    ke0, pe0 = oracle_energy(oracle, posm, vel, eps)
    ke, pe = sum(s[0] for s in shares), sum(s[1] for s in shares)
    print(f"numpy shares N={n} eps={eps}: ke rel diff {abs(ke - ke0) / abs(ke0):.3e}, pe rel diff {abs(pe - pe0) / abs(pe0):.3e}")
    assert all(s[0] > 0.0 and s[1] < 0.0 for s in shares)
    assert abs(ke - ke0) <= 1e-12 * abs(ke0)
    assert abs(pe - pe0) <= 1e-12 * abs(pe0)


def test_the_sizes_below_reach_the_cases_they_are_named_for():
    # the table of test_energy_matches_the_fp64_oracle, from the geometry restated in diagnostics_ref.energy_geometry
    for n in (1, 2, 255, 256, 257, 2047):
        assert R.energy_geometry(n)[1] == 1
    assert R.energy_geometry(2048) == (8, 2, 1024)
    assert R.energy_geometry(2049) == (9, 2, 1280) and 2049 - 1280 == 769 and 769 % 256 == 1
    assert R.energy_geometry(2561)[1:] == (2, 1536) and (2561 - 1536) % 256 == 1
    assert R.energy_geometry(4096) == (16, 4, 1024)
    assert R.energy_geometry(4097) == (17, 4, 1280) and 4097 - 3 * 1280 == 257
    assert R.energy_geometry(8193) == (33, 7, 1280)                   # the loop stops at 8 chunks, 7 are launched
    assert R.energy_geometry(12289)[1] > 1 and 12289 % R.energy_geometry(12289)[2] % 256 != 0
    assert R.energy_geometry(40000)[:2] == (157, 16) and 157 * 16 == 2512 and -(-2512 // 256) == 10
    assert R.energy_geometry(3001)[1] == 2
    assert R.energy_geometry(2047, 1023)[1] == 1 and R.energy_geometry(4096, 4096) == R.energy_geometry(4096)


def test_one_body_kinetic_candidates():
    m, v = np.float32(3.7), np.array([1.1, -2.3, 4.9], np.float32)
    assert len(R.one_body_kinetic(m, v)) == 1                          # float inputs: exact products, one value
    vd = np.array([1.1, -2.3, 4.9])
    assert 0.5 * 3.7 * (vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2]) in R.one_body_kinetic(3.7, vd)


# ---- 1. energy against the fp64 oracle across the split geometry ---------------------------------------------------------------------

SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 2561, 4096, 4097, 8193, 12289, 40000]
_ORACLE_CACHE = {}


def scene_and_oracle(oracle, n, prec, eps):
    """One scene per (n, width) and one oracle evaluation per (n, width, eps), shared by the precisions of that width."""
    dt = np_dtype(prec)
    key = (n, dt, eps)
    if key not in _ORACLE_CACHE:
        posm, vel = R.scene(n, n + 101, dt)
        _ORACLE_CACHE[key] = (posm, vel, oracle_energy(oracle, posm, vel, eps))
    return _ORACLE_CACHE[key]


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.7])
@pytest.mark.parametrize("n,prec", [(n, p) for n in SIZES for p in ("f32", "f64")] + [(2049, "f32_kahan"), (8193, "f32_kahan")])
def test_energy_matches_the_fp64_oracle(nb, oracle, n, prec, eps):
    posm, vel, ref = scene_and_oracle(oracle, n, prec, eps)
    with nb.NBodyEngine(n, precision=prec, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.energy()
        assert e.energy() == got                                       # one slot per workgroup, folded in a fixed order
    if n == 1:
        assert got[1] == 0.0
        assert got[0] in R.one_body_kinetic(posm[0, 3], vel[0]), (got[0], R.one_body_kinetic(posm[0, 3], vel[0]))
    check_energy(f"N={n} eps={eps} chunks={R.energy_geometry(n)[1]}", prec, got, ref)


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.7])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [2047, 4096])
def test_split_energy_against_the_same_bodies_in_slices(nb, oracle, n, prec, eps):
    """N = 4096 runs four chunks; a context created with i_begin = 0, i_count = 4096 has the same geometry and must give the same
    bits.  Two half slices add their halves of the i range over the same chunks: the whole within 1e-12, at N = 2047 (one chunk
    in the whole and in both halves) and at N = 4096 alike — a chunk dropped or counted twice on either side cannot hide."""
    posm, vel, ref = scene_and_oracle(oracle, n, prec, eps)
    with nb.NBodyEngine(n, precision=prec, eps=eps) as e:
        e.set_state(posm, vel)
        whole = e.energy()
    check_energy(f"N={n} eps={eps} whole", prec, whole, ref)
    if n == 4096:
        with nb.NBodyEngine(n, precision=prec, eps=eps, i_begin=0, i_count=n) as e:
            e.set_state(posm, vel)
            assert e.energy() == whole
    half = n // 2
    parts = []
    for lo, hi in ((0, half), (half, n)):
        with nb.NBodyEngine(n, precision=prec, eps=eps, i_begin=lo, i_count=hi - lo) as e:
            e.set_state(posm, vel)
            parts.append(e.energy())
    ke, pe = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    print(f"energy N={n} eps={eps} {prec}: two halves against the whole: ke {abs(ke - whole[0]) / abs(whole[0]):.3e}, "
          f"pe {abs(pe - whole[1]) / abs(whole[1]):.3e}")
    assert abs(ke - whole[0]) <= 1e-12 * abs(whole[0])
    assert abs(pe - whole[1]) <= 1e-12 * abs(whole[1])


# ---- 2. edges of the pair rule -------------------------------------------------------------------------------------------------------

def edge_scene(n, dt):
    posm, vel = R.scene(n, n + 29, dt)
    posm[17, :3] = posm[n - 400, :3]                                   # partners in different chunks of the j range
    posm[600, :3] = posm[601, :3]                                      # neighbours
    posm[1200, :3] = posm[0, :3]                                       # on the origin with body 0, where the tile padding sits
    posm[n - 1, :3] = posm[3, :3]                                      # the last body, in the ragged last tile
    for i in (5, 256, 257, 1023, 1535, 1536, 2000, 2815, 2816, n - 2):
        posm[i, 3] = 0.0                                               # zero-mass bodies, some on tile and chunk edges
    return posm, vel


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.7])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_energy_with_coincident_and_massless_bodies(nb, oracle, prec, eps):
    """d^2 + eps^2 == 0 skips a pair, anything else counts it (oracle_energy_f64's rule): coincident pairs vanish at eps = 0 and
    weigh -G m m / eps at eps > 0."""
    n, dt = 3001, np_dtype(prec)
    posm, vel = edge_scene(n, dt)
    with nb.NBodyEngine(n, precision=prec, eps=eps) as e:
        e.set_state(posm, vel)
        got = e.energy()
        ref = oracle_energy(oracle, posm, vel, eps)
        check_energy(f"N={n} eps={eps} coincident pairs", prec, got, ref)
        if eps > 0.0:
            moved = posm.copy()
            moved[601, 0] = moved[601, 0] + dt(1.0)
            shift = np.asarray(moved[601, :3], np.float64) - np.asarray(posm[601, :3], np.float64)
            e.set_state(moved, vel)
            got_m = e.energy()
            ref_m = oracle_energy(oracle, moved, vel, eps)
            check_energy(f"N={n} eps={eps} one partner moved", prec, got_m, ref_m)
            want, own = R.moved_partner_difference(posm, 601, 600, shift, eps=eps)
            diff = got[1] - got_m[1]
            print(f"energy N={n} eps={eps} {prec}: pair's own term {own:.17g}, pe difference {diff:.17g}, expected {want:.17g}, "
                  f"oracle's {ref[1] - ref_m[1]:.17g}; off by {abs(diff - want) / abs(got[1]):.3e} of |pe|")
            assert abs((ref[1] - ref_m[1]) - want) <= 1e-10 * abs(ref[1])
            assert abs(diff - want) <= 1e-10 * abs(got[1])
            assert abs(own) > 1e-6 * abs(got[1])                       # the term is far above the bound: dropping it fails


# ---- 3. slices -----------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("eps", [0.0, 0.7])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n,cuts", [(5000, (0, 1999, 4001, 5000)), (8193, (0, 4096, 8193))])
def test_energy_of_slices_is_the_owned_bodies_share(nb, n, cuts, prec, eps):
    """posm is read by the global index, vel by the local one; the potential is the owned bodies' 1/2 m_i phi_i with phi_i from all
    bodies.  After one step of every slice (its own velocities, all positions refreshed from the single context as a job's
    all-gather would) the same again, against shares of the single context's state."""
    hip = hip_runtime()
    dt = np_dtype(prec)
    posm, vel = R.scene(n, n + 7, dt)
    shares0 = R.energy_shares(posm, vel, cuts, eps=eps)
    with nb.NBodyEngine(n, precision=prec, eps=eps) as e:
        e.set_state(posm, vel)
        whole0 = e.energy()
        e.step(0.01, 1)
        p1, v1, _ = e.state(dt)
        whole1 = e.energy()
    shares1 = R.energy_shares(p1, v1, cuts, eps=eps)
    assert not np.array_equal(p1, posm)
    got0, got1 = [], []
    for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        with nb.NBodyEngine(n, precision=prec, eps=eps, i_begin=lo, i_count=hi - lo) as e:
            e.set_state(posm, vel)
            got0.append(e.energy())
            check_energy(f"N={n} eps={eps} slice [{lo},{hi})", prec, got0[-1], shares0[k])
            e.step(0.01, 1)
            ps, vs, _ = e.state(dt)
            np.testing.assert_array_equal(vs, v1[lo:hi])
            np.testing.assert_array_equal(ps, p1[lo:hi])
            ptr, nbytes = e.device_ptr(nb.BUF_POSM)
            assert nbytes == p1.nbytes
            e.synchronize()
            assert hip.hipMemcpy(ptr, p1.ctypes.data, nbytes, 1) == 0
            got1.append(e.energy())
            check_energy(f"N={n} eps={eps} slice [{lo},{hi}) after a step", prec, got1[-1], shares1[k])
    for label, got, whole in (("at the start", got0, whole0), ("after a step", got1, whole1)):
        ke, pe = sum(g[0] for g in got), sum(g[1] for g in got)
        print(f"energy N={n} eps={eps} {prec}: slices against the single context {label}: ke {abs(ke - whole[0]) / abs(whole[0]):.3e}, "
              f"pe {abs(pe - whole[1]) / abs(whole[1]):.3e}")
        assert abs(ke - whole[0]) <= 1e-12 * abs(whole[0])
        assert abs(pe - whole[1]) <= 1e-12 * abs(whole[1])


# ---- 4. theta > 0 contexts and tracers -----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n,kernel", [(2000, BH_SMALL), (5000, BH_LANE)])
def test_energy_of_a_barnes_hut_context_is_the_all_pairs_energy(nb, oracle, n, kernel):
    posm, vel = R.scene(n, n + 13)
    with nb.NBodyEngine(n, theta=1.0) as e:
        assert e.launch_config()["kernel"] == kernel
        e.set_state(posm, vel)
        check_energy(f"N={n} theta=1 after set_state", "f32", e.energy(), oracle_energy(oracle, posm, vel, 0.0))
        e.step(0.01, 3)
        p, v, _ = e.state()
        assert not np.array_equal(p, posm)
        check_energy(f"N={n} theta=1 after 3 steps", "f32", e.energy(), oracle_energy(oracle, p, v, 0.0))


@gpu
@pytest.mark.parametrize("theta", [0.0, 1.0])
def test_tracers_change_neither_energy_nor_bounds(nb, theta):
    n = 2000
    posm, vel = R.scene(n, n + 19)
    rng = np.random.default_rng(5)
    tr_pos = rng.uniform(-450, 450, (300, 3)).astype(np.float32)
    tr_vel = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    seen = []
    for tracers in (False, True):
        with nb.NBodyEngine(n, theta=theta) as e:
            e.set_state(posm, vel)
            if tracers:
                e.set_tracers(tr_pos, tr_vel)
                assert e.tracer_count == 300
            before = (e.energy(), e.bounds())
            e.step(0.01, 2)
            seen.append((before, e.energy(), e.bounds()))
    assert seen[0] == seen[1]
    assert seen[0][0][0] != seen[0][1]                                 # the steps did move the bodies


# ---- 5. live buffers after odd step counts -------------------------------------------------------------------------------------------

def _diagnostics_follow_the_steps(nb, oracle, e, prec, posm, vel, kernel, label, held=False):
    dt = np_dtype(prec)
    assert e.launch_config()["kernel"] == kernel
    e.set_state(posm, vel)
    if held:
        e.device_ptr(nb.BUF_POSM)                                      # the caller holds the buffer: two launches per step from here on
    last = posm
    for done, more in ((1, 1), (3, 2)):
        e.step(0.01, more)
        assert e.launch_config()["kernel"] == kernel
        ke_pe, size = e.energy(), e.bounds()
        p, v, _ = e.state(dt)
        assert e.steps_done() == done and not np.array_equal(p, last)
        last = p
        check_energy(f"{label} after {done} steps", prec, ke_pe, oracle_energy(oracle, p, v, 0.0))
        assert size == expected_bounds(oracle, p, prec), (label, done)
        assert (e.energy(), e.bounds()) == (ke_pe, size)


@gpu
@pytest.mark.parametrize("held", [False, True])
def test_diagnostics_after_odd_step_counts_one_launch_step(nb, oracle, held):
    n = 2560
    posm, vel = R.scene(n, n + 31)
    with nb.NBodyEngine(n) as e:
        _diagnostics_follow_the_steps(nb, oracle, e, "f32", posm, vel, BLOCK_PK, f"N={n} one-launch step held={held}", held)


@gpu
@pytest.mark.parametrize("prec", ["f32_kahan", "f64"])
def test_diagnostics_after_odd_step_counts_block_kernel(nb, oracle, prec):
    n = 2001
    posm, vel = R.scene(n, n + 37, np_dtype(prec))
    with nb.NBodyEngine(n, precision=prec) as e:
        _diagnostics_follow_the_steps(nb, oracle, e, prec, posm, vel, BLOCK, f"N={n} block kernel")


@gpu
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("equal", [True, False])
def test_diagnostics_after_odd_step_counts_fused_symmetric_step(nb, oracle, equal, held):
    n = 24576
    posm, vel = R.scene(n, n + 41, equal=equal)
    with nb.NBodyEngine(n) as e:
        assert e.launch_config()["algorithm"] == "symmetric"
        _diagnostics_follow_the_steps(nb, oracle, e, "f32", posm, vel, SYM_PK, f"N={n} symmetric step equal={equal} held={held}", held)


@gpu
def test_diagnostics_after_odd_step_counts_barnes_hut(nb, oracle):
    n = 5000
    posm, vel = R.scene(n, n + 43)
    with nb.NBodyEngine(n, theta=1.0) as e:
        _diagnostics_follow_the_steps(nb, oracle, e, "f32", posm, vel, BH_LANE, f"N={n} theta=1")


# ---- 6. bounds -----------------------------------------------------------------------------------------------------------------------

PLANT = 777.25


def placements(n):
    """(body, axis, negative) for the planted extreme: index 0, n - 1, n // 2 and the last index of the first full workgroup; on
    every axis with either sign in the small systems, cycled through in the large ones."""
    where = sorted({0, n - 1, n // 2, min(n - 1, R.K_BLOCK - 1)})
    if n <= 2000:
        return [(i, axis, neg) for i in where for axis in range(3) for neg in (False, True)]
    return [(i, (k + n) % 3, k % 2 == 1) for k, i in enumerate(where)]


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 2000, 100003, 1048576])
def test_bounds_finds_a_planted_extreme(nb, oracle, n, prec):
    dt = np_dtype(prec)
    base, vel = R.scene(n, n + 53, dt)
    assert np.abs(base[:, :3]).max() <= 500.0
    with nb.NBodyEngine(n, precision=prec) as e:
        e.set_state(base, vel)
        assert e.bounds() == expected_bounds(oracle, base, prec)
        for i, axis, neg in placements(n):
            posm = base.copy()
            posm[i, axis] = -PLANT if neg else PLANT
            e.set_state(posm, vel)
            got = e.bounds()
            assert got == PLANT == expected_bounds(oracle, posm, prec), (n, prec, i, axis, neg, got)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bounds_of_bodies_all_at_the_origin_is_zero(nb, prec):
    n, dt = 300, np_dtype(prec)
    posm = np.zeros((n, 4), dt)
    posm[:, 3] = 1.0
    posm[137, 1] = -0.0
    with nb.NBodyEngine(n, precision=prec) as e:
        e.set_state(posm, np.zeros((n, 4), dt))
        got = e.bounds()
    assert got == 0.0 and math.copysign(1.0, got) == 1.0


@gpu
@pytest.mark.parametrize("planted,want", [(777.2500000001, 777.25), (-777.2500000001, 777.25), (16777217.0, 16777216.0)])
def test_bounds_of_an_fp64_context_is_the_float_of_the_largest_coordinate(nb, planted, want):
    n = 1000
    posm, vel = R.scene(n, n + 59, np.float64)
    posm[n - 3, 2] = planted
    assert float(np.float32(abs(planted))) == want
    with nb.NBodyEngine(n, precision="f64") as e:
        e.set_state(posm, vel)
        assert e.bounds() == want


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bounds_of_a_slice_is_its_own_bodies(nb, oracle, prec):
    n, cuts, dt = 5000, (0, 1999, 4001, 5000), np_dtype(prec)
    base, vel = R.scene(n, n + 61, dt)
    for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        posm = base.copy()
        outside = [i for i in (lo - 1, hi) if 0 <= i < n]              # the neighbours of the slice's two ends
        for i in outside:
            posm[i, k % 3] = -900.5
        with nb.NBodyEngine(n, precision=prec, i_begin=lo, i_count=hi - lo) as e:
            e.set_state(posm, vel)
            assert e.bounds() == expected_bounds(oracle, posm[lo:hi], prec) < 500.0
            for i in (lo, hi - 1):                                      # and its own extreme on its first and on its last body
                q = posm.copy()
                q[i, (k + 1) % 3] = -PLANT
                e.set_state(q, vel)
                assert e.bounds() == PLANT, (prec, lo, hi, i)
