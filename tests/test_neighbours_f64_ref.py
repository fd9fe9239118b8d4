"""The fp64 neighbour census without a device: the four symbols are declared and bound, the yardstick of tests/neighbours_f64_ref.py
agrees with a brute-force sort on small scenes, with closed forms and with itself across float64 and long double, and every scene the GPU
tests use meets the GAP CONDITION on all of its rows — no entry of a list (the runner-up behind it included) is within 1e-9 of the next,
so an index can be held to the reference."""
import os
import re

import numpy as np
import pytest

import census_f64_ref as C
import hermite_ref as H
import neighbours_f64_ref as N
from jerk_ref import probe_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SYMBOLS = ("nbody_get_neighbours_f64", "nbody_neighbours_at_f64", "nbody_get_density_f64", "nbody_density_centre_f64")
METHODS = ("neighbours_f64", "neighbours_at_f64", "density_f64", "core_f64")


def test_the_four_symbols_are_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = nb.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert getattr(L, s).argtypes is not None, f"{s} has no prototype in parallelnbody_amd/_lib.py"
    assert [len(getattr(L, s).argtypes) for s in SYMBOLS] == [4, 7, 4, 3]
    for name in METHODS:
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__
    assert int(re.search(r"#define NBODY_NEIGHBOURS_MAX (\d+)", text).group(1)) == nb._lib.NEIGHBOURS_MAX == N.K_MAX
    # struct nbody_core as the header lays it out: four 32-bit words, then seven doubles
    import ctypes
    assert ctypes.sizeof(nb._lib.Core) == 16 + 7 * 8 and nb._lib.Core.rho_max.offset == 16 and nb._lib.Core.rho2_sum.offset == 64


def test_the_command_line_refuses_core_lines_without_fp64(capsys):
    from parallelnbody_amd.__main__ import main
    for argv in (["--core-every", "2"], ["--core-every", "2", "--precision", "f32_kahan"],
                 ["--core-every", "2", "--precision", "f64", "--core-k", "1"], ["--core-every", "2", "--precision", "f64", "--core-k", "9"]):
        with pytest.raises(SystemExit) as er:
            main(argv)
        assert er.value.code == 2
        err = capsys.readouterr().err
        assert "--core-every needs --precision f64" in err or "--core-k must be 2 .. 8" in err


def brute(pos, x, own, k):
    """the definition, one row at a time: sorted by (d2, index)"""
    cand = []
    for j in range(pos.shape[0]):
        d = pos[j] - x
        d2 = float((d * d).sum())
        if j != own and np.isfinite(d2):
            cand.append((d2, j))
    cand.sort()
    cand = cand[:k] + [(np.inf, -1)] * (k - len(cand[:k]))
    return [c[1] for c in cand], [c[0] for c in cand]


@pytest.mark.parametrize("n", [1, 2, 5, 9, 40])
def test_brute_force_agrees_on_small_scenes(n):
    rng = np.random.default_rng(n)
    pos = rng.integers(-3, 4, (n, 3)).astype(np.float64)           # a small lattice: exact arithmetic and many ties
    pts = rng.integers(-3, 4, (7, 3)).astype(np.float64) + 0.5
    for k in (1, 3, 8):
        bi, bd, _ = N.neighbours(pos, k=k)
        pi, pd, _ = N.neighbours(pos, pts, k=k)
        for i in range(n):
            wi, wd = brute(pos, pos[i], i, k)
            assert bi[i].tolist() == wi and bd[i].tolist() == wd
        for i in range(7):
            wi, wd = brute(pos, pts[i], -1, k)
            assert pi[i].tolist() == wi and pd[i].tolist() == wd
    full = N.neighbours(pos, k=8)
    for k in range(1, 8):                                          # the answer for k is the prefix of the answer for 8
        part = N.neighbours(pos, k=k)
        assert (part[0] == full[0][:, :k]).all() and (part[1] == full[1][:, :k]).all()
    near = C.census(pos, np.ones(n), np.zeros((n, 3)))[0]          # and k = 1 is the census's nearest
    one = N.neighbours(pos, k=1)
    assert (one[0][:, 0] == near["near"]).all() and (one[1][:, 0] == near["near_d2"]).all()


def test_ties_go_to_the_lowest_index_and_what_is_not_finite_is_never_listed():
    pos = np.array([[0.0, 0, 0], [2.0, 0, 0], [-2.0, 0, 0], [0.0, 2, 0], [np.nan, 0, 0], [0.0, 0, 0], [np.inf, 0, 0]])
    idx, d2, gap = N.neighbours(pos, k=4)
    assert idx[0].tolist() == [5, 1, 2, 3] and d2[0].tolist() == [0.0, 4.0, 4.0, 4.0]      # the coincident body first, then ties by index
    assert idx[1].tolist() == [0, 5, 3, 2] and d2[1].tolist() == [4.0, 4.0, 8.0, 16.0]
    assert idx[4].tolist() == [-1] * 4 and idx[6].tolist() == [-1] * 4 and (d2[4] == np.inf).all() and (d2[6] == np.inf).all()
    assert not np.isin(idx, [4, 6]).any()                          # nobody lists the bodies at NaN and +inf
    assert gap[0] == 0.0 and gap[4] == 1.0
    idx8, d28, _ = N.neighbours(pos, k=8)
    assert idx8[0].tolist() == [5, 1, 2, 3, -1, -1, -1, -1] and (d28[0][4:] == np.inf).all()
    pidx, pd2, _ = N.neighbours(pos, np.array([[0.0, 0, 0]]), k=3)
    assert pidx[0].tolist() == [0, 5, 1] and pd2[0].tolist() == [0.0, 0.0, 4.0]            # a point drops nobody by index


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_a_kepler_binary_each_is_the_others_first_neighbour(dtype):
    posm, _, _ = H.kepler(0.5, m1=1000.0, m2=3000.0, a=100.0)
    idx, d2, gap = N.neighbours(posm, k=2, dtype=dtype)
    assert idx.tolist() == [[1, -1], [0, -1]] and d2[0, 0] == d2[1, 0] and (d2[:, 1] == np.inf).all() and (gap == 1).all()
    assert abs(float(d2[0, 0]) - 50.0 ** 2) < 1e-12 * 2500
    rho, rk2 = N.density(idx, d2, posm[:, 3], 2, dtype)
    assert (rho == 0).all() and (rk2 == np.inf).all()              # N <= k: the k-th neighbour is missing


def test_the_density_and_the_core_in_closed_form():
    # a body at the origin, neighbours at distances 1, 2, 3 with masses 5, 7, 11: k = 3 -> (5 + 7) / (4 pi / 3 * 27)
    pos = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]]); mass = np.array([2.0, 5.0, 7.0, 11.0])
    idx, d2, _ = N.neighbours(pos, k=3)
    rho, rk2 = N.density(idx, d2, mass, 3)
    assert idx[0].tolist() == [1, 2, 3] and rk2[0] == 9.0 and rho[0] == 12.0 / ((4.0 * np.pi / 3.0) * 27.0)
    rho2, _ = N.density(idx, d2, mass, 2)
    assert rho2[0] == 5.0 / ((4.0 * np.pi / 3.0) * 8.0)
    # r2 == 0: +inf with mass, 0 (a NaN quotient) without
    twin = np.array([[0.0, 0, 0], [0.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]])
    ti, td, _ = N.neighbours(twin, k=2)
    assert N.density(ti, td, np.ones(4), 2)[0][0] == np.inf and N.density(ti, td, np.zeros(4), 2)[0][0] == 0.0
    # the reductions: weights 1, 3 at x = 0, 4 -> centre 3; core radius sqrt((1 * 9 + 9 * 1) / 10); +inf and 0 weigh nothing
    c = N.core(np.array([1.0, 3.0, np.inf, 0.0, np.nan]), np.array([[0.0, 0, 0], [4.0, 0, 0], [9.0, 9, 9], [7.0, 7, 7], [1.0, 1, 1]]))
    assert c["used"] == 2 and c["densest"] == 1 and c["rho_max"] == 3.0 and c["centre"].tolist() == [3.0, 0.0, 0.0]
    assert abs(float(c["core_radius"]) - np.sqrt(1.8)) < 1e-15 and c["rho_sum"] == 4 and c["rho2_sum"] == 10
    none = N.core(np.zeros(3), np.zeros((3, 3)))
    assert none["used"] == 0 and none["densest"] == -1 and np.isnan(none["centre"]).all() and np.isnan(none["core_radius"])


def test_the_geometry_the_gpu_tests_count_on():
    assert probe_geometry(N.N_CHUNKS) == (65, 512) and len(N.ROWS_CHUNKS) == 134
    assert probe_geometry(N.N_SLAB) == (65, 512) and C.probe_slab_points(N.N_SLAB, N.K_MAX) == 31744
    assert probe_geometry(300) == (2, 256) and probe_geometry(257) == (2, 256)


@pytest.mark.parametrize("n,m", N.CASES)
def test_the_scenes_meet_the_gap_condition_and_the_yardstick_agrees_with_itself(nb, n, m):
    """The nine nearest (k = 8 and the runner-up) in long double, all rows, none left out."""
    for kind in ("bodies", "points"):
        ld = N.reference(nb, kind, n, m)
        print(f"N = {n}, M = {m}, {kind}: smallest gap {N.gaps_hold(ld):.2e}")
        if n <= 1000:
            f = N.reference(nb, kind, n, m, np.float64)
            assert (f[0] == ld[0]).all() and np.abs((f[1] - ld[1]) / ld[1]).max() < 1e-14


def test_the_sampled_rows_at_512_body_chunks_and_beyond_a_slab_meet_the_gap_condition(nb):
    for kind in ("chunks", "slab"):
        ld = N.reference(nb, kind)
        print(f"{kind}: smallest gap {N.gaps_hold(ld):.2e}")
        f = N.reference(nb, kind, dtype=np.float64)
        assert (f[0] == ld[0]).all() and np.abs((f[1] - ld[1]) / ld[1]).max() < 1e-14


def test_the_padding_points_and_the_clump_scene_meet_the_gap_condition(nb):
    posm = C.scene(nb, 257)[0]
    pts = np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [0.0, -1e-3, 0.0], [1e-3, 1e-3, 1e-3], [0.0, 0.0, 1e-6]])
    print(f"points round the origin at N = 257: smallest gap {N.gaps_hold(N.neighbours(posm, pts, dtype=LD)):.2e}")
    posm, _, members, scale = N.clump_scene(nb)
    ref = N.neighbours(posm, dtype=LD)
    print(f"the clump scene: smallest gap {N.gaps_hold(ref):.2e}")
    rho, _ = N.density(ref[0], ref[1], posm[:, 3], 6, LD)
    c = N.core(rho, posm)
    centre = np.asarray(c["centre"], np.float64)
    spot = posm[members, :3].mean(0)
    com = (posm[:, 3:4] * posm[:, :3]).sum(0) / posm[:, 3].sum()
    print(f"the density centre is {np.linalg.norm(centre - spot) / (N.CLUMP_SIGMA * scale):.3f} sigma from the clump's mean, the centre of "
          f"mass {np.linalg.norm(com - spot) / scale:.2f} scale lengths")
    assert np.linalg.norm(centre - spot) < 3 * N.CLUMP_SIGMA * scale and c["densest"] in members and np.linalg.norm(com - spot) > scale


def test_the_lattice_scene_sorts_in_full_with_exact_ties():
    posm, _ = C.lattice_scene()
    f = N.neighbours(posm)
    ld = N.neighbours(posm, dtype=LD)
    assert (f[0] == ld[0]).all() and (f[1] == ld[1]).all()         # exact in both
    assert (f[2] == 0).sum() > 100 and (f[1][:, 0] == 0).sum() == 12
    # ties whose candidates lie in both chunks of 256
    d = posm[None, :, :3] - posm[:, None, :3]
    d2 = (d * d).sum(-1)
    tied = (d2 == f[1][:, 7][:, None]) & ~np.eye(300, dtype=bool)
    assert (tied[:, :256].any(1) & tied[:, 256:].any(1)).sum() > 10
