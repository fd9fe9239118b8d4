"""The fp64 pair census without a device: the seven symbols are declared and bound, the yardstick of tests/census_f64_ref.py meets
the closed forms of one and two bodies, agrees with itself across float64 and long double on every scene the GPU tests use, and
every such scene meets the GAP CONDITION — no row's answer is within 1e-9 of its runner-up, so an index can be held to the reference."""
import os
import re

import numpy as np
import pytest

import census_f64_ref as C
import hermite_ref as H
from jerk_ref import G, probe_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SYMBOLS = ("nbody_get_nearest_f64", "nbody_nearest_at_f64", "nbody_closest_pair_f64", "nbody_get_partners_f64", "nbody_partner_at_f64",
           "nbody_hardest_pair_f64", "nbody_pair_time_f64")
METHODS = ("nearest_f64", "nearest_at_f64", "closest_pair_f64", "partners_f64", "partner_at_f64", "hardest_pair_f64", "pair_time_f64",
           "binaries_f64")


def test_the_seven_symbols_are_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = nb.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert getattr(L, s).argtypes is not None, f"{s} has no prototype in parallelnbody_amd/_lib.py"
    assert [len(getattr(L, s).argtypes) for s in SYMBOLS] == [3, 6, 4, 4, 9, 5, 4]
    for name in METHODS:
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_one_body_has_nobody(dtype):
    o = C.census(np.array([[1.5, -2.25, 3.0]]), [7.0], np.zeros((1, 3)), eps=(0.0, 0.5), dtype=dtype)
    for r in o:
        assert r["near"].tolist() == [-1] and r["part"].tolist() == [-1]
        assert r["near_d2"][0] == np.inf and r["part_e"][0] == np.inf and r["part_d2"][0] == np.inf
    assert C.pair_of(o[0]["near"], o[0]["near_d2"]) == (-1, -1, np.inf)
    # a point, though, has that body — at d2 = 0 when it sits on it, with e = 0.5 v^2 there at eps == 0 and 0.5 v^2 - G m / eps else
    p = C.census(np.array([[1.5, -2.25, 3.0]]), [7.0], np.zeros((1, 3)), pts=np.array([[1.5, -2.25, 3.0]]), pvel=np.array([[3.0, 0.0, 4.0]]),
                 eps=(0.0, 0.5), dtype=dtype)
    assert p[0]["near"].tolist() == [0] and p[0]["near_d2"][0] == 0 and p[0]["part"].tolist() == [0]
    assert p[0]["part_e"][0] == 12.5 and p[1]["part_e"][0] == dtype(12.5) - dtype(G) * 7 / dtype(0.5)


@pytest.mark.parametrize("e", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_a_binary_in_closed_form(e, dtype):
    """Two bodies on a Kepler orbit of semi-major axis a (e = 0: circular): each is the other's nearest and partner, and the pair's
    specific orbital energy is -G (m1 + m2) / (2 a) — at every point of the orbit, so at the pericentre kepler() starts from."""
    m1, m2, a = 1000.0, 3000.0, 100.0
    posm, vel, _ = H.kepler(e, m1=m1, m2=m2, a=a)
    r = C.census(posm[:, :3], posm[:, 3], vel, dtype=dtype)[0]
    assert r["near"].tolist() == [1, 0] and r["part"].tolist() == [1, 0]
    want = -G * (m1 + m2) / (2 * a)
    rp = a * (1 - e)
    assert np.abs(r["part_e"].astype(np.float64) - want).max() < 1e-14 * (G * (m1 + m2) / rp)      # (e cancels from terms of that size)
    assert np.abs(r["near_d2"].astype(np.float64) - rp * rp).max() < 1e-14 * rp * rp
    assert r["part_e"][0] == r["part_e"][1] and r["near_d2"][0] == r["near_d2"][1] and (r["part_d2"] == r["near_d2"]).all()
    assert (r["near_gap"] == 1).all() and (r["part_gap"] == 1).all()                              # no runner-up at all
    assert C.pair_of(r["near"], r["near_d2"]) == (0, 1, float(r["near_d2"][0]))
    t = C.pair_time_of(rp * rp, m1, m2)
    assert abs(t - (rp ** 3 / (G * (m1 + m2))) ** 0.5) < 1e-15 * t and C.pair_time_of(4.0, 0.0, 0.0) == np.inf


def test_ties_go_to_the_lowest_index_and_what_is_not_finite_is_never_chosen():
    pos = np.array([[0.0, 0, 0], [2.0, 0, 0], [-2.0, 0, 0], [0.0, 2, 0], [np.nan, 0, 0], [0.0, 0, 0]])
    mass = np.full(6, 5.0); vel = np.zeros((6, 3))
    r = C.census(pos, mass, vel)[0]
    assert r["near"].tolist() == [5, 0, 0, 0, -1, 0]               # the coincident body; then 0 before 5; the NaN body has nobody
    assert r["near_d2"].tolist()[:4] == [0.0, 4.0, 4.0, 4.0] and r["near_d2"][4] == np.inf
    assert r["part"].tolist() == [1, 0, 0, 0, -1, 1]               # at eps == 0 the coincident body gives e = 0: the first at distance 2 wins
    assert (r["near"] != 4).all() and (r["part"] != 4).all()
    assert r["near_gap"][0] == 1.0 and r["near_gap"][1] == 0.0     # (4 - 0) / 4; an exact tie
    t = C.census(pos, mass, vel, beyond_exact_ties=True)[0]
    assert t["near"].tolist() == r["near"].tolist() and t["near_gap"][1] == 0.5    # body 1: 4 (twice), then 8


def test_the_geometry_the_gpu_tests_count_on():
    assert probe_geometry(C.N_CHUNKS) == (65, 512) and C.N_CHUNKS - 64 * 512 == 1 and len(C.ROWS_CHUNKS) == 134
    assert probe_geometry(C.N_SLAB) == (65, 512) and C.probe_slab_points(C.N_SLAB, 2) == 129024
    assert probe_geometry(300) == (2, 256) and probe_geometry(257) == (2, 256)


def agree(a, b):
    """two census dicts of one scene, float64 and long double: the same indices, values within a few fp64 roundings"""
    assert (a["near"] == b["near"]).all() and (a["part"] == b["part"]).all()
    assert np.abs((a["near_d2"] - b["near_d2"]) / b["near_d2"]).max() < 1e-14
    assert np.abs((a["part_d2"] - b["part_d2"]) / b["part_d2"]).max() < 1e-14
    assert np.abs((a["part_e"] - b["part_e"]) / b["part_scale"]).max() < 1e-14


@pytest.mark.parametrize("n,m", C.CASES)
def test_the_scenes_meet_the_gap_condition_and_the_yardstick_agrees_with_itself(nb, n, m):
    """Measured: the smallest gaps over these scenes are 2.1e-4 (nearest, N = 4097) and 2.9e-5 (partner, N = 1000), bodies and
    points, the same at both eps to two digits — four orders above GAP_MIN."""
    for kind in ("bodies", "points"):
        for eps in C.EPS:
            ld = C.reference(nb, kind, n, m)[eps]
            near, part = C.gaps_hold(ld)
            print(f"N = {n}, M = {m}, {kind}, eps = {eps}: smallest gaps {near:.2e} (nearest), {part:.2e} (partner)")
            if n <= 1000:                                          # (the float64 twin of the largest scene adds nothing but time)
                agree(C.reference(nb, kind, n, m, np.float64)[eps], ld)


def test_the_sampled_rows_at_512_body_chunks_and_beyond_a_slab_meet_the_gap_condition(nb):
    for kind in ("chunks", "slab"):
        for eps in C.EPS:
            ld = C.reference(nb, kind, 0)[eps]
            near, part = C.gaps_hold(ld)
            print(f"{kind}, eps = {eps}: smallest gaps {near:.2e} (nearest), {part:.2e} (partner)")
            agree(C.reference(nb, kind, 0, 0, np.float64)[eps], ld)


def test_the_lattice_scene_has_exact_ties_and_nothing_else_close():
    posm, vel = C.lattice_scene()
    n = posm.shape[0]
    assert n == 300 and (posm[:, :3] == np.round(posm[:, :3])).all() and (vel == np.round(vel)).all() and (posm[:, 3] == posm[0, 3]).all()
    plain = C.census(posm[:, :3], posm[:, 3], vel, dtype=LD)[0]
    beyond = C.census(posm[:, :3], posm[:, 3], vel, dtype=LD, beyond_exact_ties=True)[0]
    f64 = C.census(posm[:, :3], posm[:, 3], vel)[0]
    assert (plain["near_gap"] == 0).sum() > 100 and (plain["part_gap"] == 0).sum() > 10      # exact ties, many of them
    assert (plain["near_d2"] == 0).sum() == 12                     # six coincident pairs
    chunk = probe_geometry(n)[1]
    d = posm[None, :, :3] - posm[:, None, :3]
    tied = ((d * d).sum(-1) == f64["near_d2"][:, None].astype(np.float64)) & ~np.eye(n, dtype=bool)
    assert (tied[:, :chunk].any(1) & tied[:, chunk:].any(1)).sum() > 10          # ... whose candidates lie in both chunks
    near, part = float(beyond["near_gap"].min()), float(beyond["part_gap"].min())
    print(f"lattice, seed {C.LATTICE_SEED}: beyond the exact ties the smallest gaps are {near:.2e} (nearest), {part:.2e} (partner)")
    assert near > C.GAP_MIN and part > C.GAP_MIN
    assert (f64["near"] == plain["near"]).all() and (f64["part"] == plain["part"]).all()
    assert (f64["near_d2"] == plain["near_d2"]).all() and (f64["part_d2"] == plain["part_d2"]).all()   # exact in both


def test_the_planted_binary_is_the_hardest_pair_of_its_scene(nb):
    posm, vel, a, ecc = C.binary_scene(nb)
    r = C.census(posm[:, :3], posm[:, 3], vel, dtype=LD)[0]
    assert r["part"][0] == 1 and r["part"][1] == 0
    i, j, e = C.pair_of(r["part"], r["part_e"])
    assert (i, j) == (0, 1)
    mu = G * (posm[0, 3] + posm[1, 3])
    assert abs(-mu / (2 * e) - a) < 1e-12 * a
    C.gaps_hold(r)
