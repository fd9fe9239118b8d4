"""nbody_get_moments / nbody_mass_within without a device: the exported symbols, the struct against the header, the refusals that need no
context, the references of tests/moments_ref.py against exact rational sums, the geometry rule the GPU tests' sizes are chosen by, and
ShardedSimulation's all-reduce of the ranks' shares over gloo with a numpy stand-in for the engine."""
import ctypes
import os
import socket
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import diagnostics_ref as R
import moments_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = {"struct_size": 0, "reserved": 4, "count": 8, "mass": 16, "mx": 24, "p": 48, "l": 72, "second": 96, "kinetic": 144,
           "virial": 152, "force": 160, "torque": 184}


def test_both_symbols_are_exported_and_bound(nb):
    L = nb.lib()
    for name in ("nbody_get_moments", "nbody_mass_within"):
        assert getattr(L, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()
    assert "NBODY_AMD_API int nbody_get_moments(" in header and "NBODY_AMD_API int nbody_mass_within(" in header


def test_moments_struct_matches_the_header(nb, tmp_path):
    S = nb._lib.Moments
    assert ctypes.sizeof(S) == 208
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == OFFSETS
    # ... and the header itself, through a C compiler
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody.h"\nint main(void) {\n  printf("%zu", sizeof(nbody_moments));\n'
                   + "".join(f'  printf(" %zu", offsetof(nbody_moments, {k}));\n' for k in OFFSETS) + '  return 0;\n}\n')
    exe = str(tmp_path / "offsets")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(w) for w in subprocess.check_output([exe]).split()]
    assert out == [208] + list(OFFSETS.values())


def test_refusals_that_need_no_context(nb):
    L = nb.lib()
    m = nb._lib.Moments()
    m.struct_size = ctypes.sizeof(m)
    assert L.nbody_get_moments(None, ctypes.byref(m)) == nb._lib.ERR_INVALID
    m.struct_size = 200
    assert L.nbody_get_moments(None, ctypes.byref(m)) == nb._lib.ERR_INVALID
    assert L.nbody_get_moments(None, None) == nb._lib.ERR_INVALID
    c = (ctypes.c_double * 3)(0, 0, 0)
    r = (ctypes.c_double * 1)(1.0)
    out = (ctypes.c_double * 1)()
    assert L.nbody_mass_within(None, c, r, 1, out, None) == nb._lib.ERR_INVALID


def test_geometry_rule_and_the_sizes_the_gpu_tests_use():
    assert M.geometry(1) == (1, 1) and M.geometry(256) == (1, 256) and M.geometry(257) == (2, 129)
    assert M.geometry(2000) == (8, 250) and M.geometry(100003) == (391, 256)
    assert M.geometry(262144) == (1024, 256)                             # the cap is reached with one trip each ...
    assert M.geometry(262145) == (1021, 257)                             # ... one body more: two trips, the second with one lane
    assert M.geometry(1 << 20) == (1024, 1024) and M.geometry(1 << 23) == (1024, 8192)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1999, 2000, 2049, 4096, 100003, 262144, 262145, (1 << 20) + 1):
        slots, per = M.geometry(n)
        assert 1 <= slots <= M.SLOT_CAP and (slots - 1) * per < n <= slots * per


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_references_agree_with_exact_rational_sums(dtype):
    n = 50
    posm, vel = R.scene(n, 4242, dtype)
    acc = np.random.default_rng(7).uniform(-300, 300, (n, 4)).astype(dtype)
    s0, big = M.reference(posm, vel, acc)
    exact = M.exact_sums(posm, vel, acc)
    # fsum adds the ROUNDED terms exactly and rounds once; a term is formed with at most 4 roundings (l, torque: two products, their
    # difference, the mass factor), each 2^-53 of a product that enters A: |S0 - exact| <= 8 * 2^-53 * A with room to spare
    for k in range(24):
        assert abs(Fraction(float(s0[k])) - exact[k]) <= Fraction(8, 2 ** 53) * Fraction(float(big[k])), M.NAMES[k]
        assert big[k] > 0 and abs(exact[k]) <= Fraction(float(big[k])) * (1 + Fraction(8, 2 ** 53))
    # the mass profile: numpy's membership against a plain Python loop over the same expression, masses against exact sums
    centre = np.array([12.345678901234567, -7.1122334455667788, 3.3000000000000003])
    d2 = M.distances2(posm, centre)
    radii = np.concatenate([[0.0], np.sqrt(np.sort(d2))[::7], [1e4]])
    mass, count, big = M.mass_within(posm, centre, radii)
    for q, r in enumerate(radii):
        inside = []
        for i in range(n):
            dx, dy, dz = float(posm[i, 0]) - centre[0], float(posm[i, 1]) - centre[1], float(posm[i, 2]) - centre[2]
            if (dx * dx + dy * dy) + dz * dz <= float(r) * float(r):
                inside.append(i)
        assert count[q] == len(inside)
        want = sum((Fraction(float(posm[i, 3])) for i in inside), Fraction(0))
        assert abs(Fraction(float(mass[q])) - want) <= Fraction(1, 2 ** 53) * Fraction(float(big[q]))
    assert count[0] == 0 and count[-1] == n and (np.diff(count) >= 0).all()


def test_derived_fields_of_a_moments_result(nb):
    from parallelnbody_amd.engine import MOMENT_FIELDS, moments_result
    n = 50
    posm, vel = R.scene(n, 99, np.float64)
    acc = np.zeros_like(vel)
    s0, _ = M.reference(posm, vel, acc)
    sums, at = {}, 0
    for k, w in zip(MOMENT_FIELDS, (1, 3, 3, 3, 6, 1, 1, 3, 3)):
        sums[k] = s0[at] if w == 1 else s0[at:at + w]
        at += w
    m = moments_result(n, sums)
    assert m.count == n and isinstance(m.mass, float) and m.second.shape == (6,)
    np.testing.assert_array_equal(M.flat(m), s0)
    mass = posm[:, 3]
    com = (mass[:, None] * posm[:, :3]).sum(0) / mass.sum()
    vcom = (mass[:, None] * vel[:, :3]).sum(0) / mass.sum()
    l_com = (mass[:, None] * np.cross(posm[:, :3] - com, vel[:, :3] - vcom)).sum(0)
    np.testing.assert_allclose(m.com, com, rtol=1e-13)
    np.testing.assert_allclose(m.com_velocity, vcom, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(m.l_about_com, l_com, rtol=1e-9)


# ---- ShardedSimulation.moments() / .mass_within(): the ranks' shares through one all-reduce ----------------------------------------------

class MomentsEngine:
    """Stand-in with NBodyEngine's interface for the two calls: this rank's shares from the numpy references."""

    def __init__(self, n_total, i_begin, i_count, posm_tensor, device_index, **kw):
        self.lo, self.cnt = i_begin, i_count
        self.posm = posm_tensor.numpy()
        self.vel = np.zeros((i_count, 4), np.float32)
        self.acc = np.zeros((i_count, 4), np.float32)

    def set_state(self, posm, vel):
        self.posm[:] = posm
        self.vel[:] = vel[self.lo:self.lo + self.cnt]
        self.acc[:, :3] = 0.25 * self.vel[:, :3] - 0.5            # anything that differs from body to body

    def exchange_ranks(self):
        return 0

    def moments(self):
        from parallelnbody_amd.engine import MOMENT_FIELDS, moments_result
        s0, _ = M.reference(self.posm[self.lo:self.lo + self.cnt], self.vel, self.acc)
        sums, at = {}, 0
        for k, w in zip(MOMENT_FIELDS, (1, 3, 3, 3, 6, 1, 1, 3, 3)):
            sums[k] = s0[at] if w == 1 else s0[at:at + w]
            at += w
        return moments_result(self.cnt, sums)

    def mass_within(self, centre, radii):
        mass, count, _ = M.mass_within(self.posm[self.lo:self.lo + self.cnt], centre, radii)
        return mass.reshape(np.shape(radii)), count.reshape(np.shape(radii))

    def close(self):
        pass


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import parallelnbody_amd as nb
    posm, vel = R.scene(n, 31)
    sim = nb.ShardedSimulation(posm, vel, rank=rank, world_size=world, device="cpu", engine_factory=MomentsEngine)
    m = sim.moments()
    mass, count = sim.mass_within((1.5, -2.5, 0.125), np.array([[0.0, 100.0], [250.0, 1e4]]))
    np.savez(os.path.join(out_dir, f"m{rank}.npz"), flat=M.flat(m), count=m.count, com=m.com, mass=mass, counts=count,
             acc=sim.engine.acc)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_add_their_shares(nb, tmp_path):
    import torch.multiprocessing as mp
    n = 256
    mp.spawn(_worker, args=(2, _free_port(), n, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "m0.npz"), np.load(tmp_path / "m1.npz")
    for k in ("flat", "count", "com", "mass", "counts"):
        np.testing.assert_array_equal(r0[k], r1[k])                 # every rank holds the system's totals
    posm, vel = R.scene(n, 31)
    acc = np.concatenate([r0["acc"], r1["acc"]])
    halves = [M.reference(posm[lo:lo + n // 2], vel[lo:lo + n // 2], acc[lo:lo + n // 2])[0] for lo in (0, n // 2)]
    np.testing.assert_array_equal(r0["flat"], halves[0] + halves[1])      # one fp64 addition per field
    assert int(r0["count"]) == n
    _, big = M.reference(posm, vel, acc)
    assert (np.abs(r0["flat"] - M.reference(posm, vel, acc)[0]) <= M.gamma(n) * big).all()
    mass, count, _ = M.mass_within(posm, (1.5, -2.5, 0.125), [0.0, 100.0, 250.0, 1e4])
    assert r0["counts"].shape == (2, 2) and r0["counts"].dtype == np.int64
    np.testing.assert_array_equal(r0["counts"].reshape(-1), count)
    np.testing.assert_allclose(r0["mass"].reshape(-1), mass, rtol=1e-14)
    assert count[-1] == n
