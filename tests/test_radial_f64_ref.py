"""The fp64 radial census without a device: the two symbols are declared and bound, struct nbody_lagrange is laid out as the header
says, the command line refuses what it must, the blocked scan of tests/radial_f64_ref.py stays within the bound of ANY summation order of
the long-double sum and never decreases, the closed forms hold, radial_profile()'s formulas give a hand-made system's numbers, and every
(scene, fraction) pair the GPU tests compare a body index for meets the GAP CONDITION — gap >= 4 n 2^-53, no pair left out."""
import ctypes
import os
import re

import numpy as np
import pytest

import radial_f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SYMBOLS = ("nbody_radial_order_f64", "nbody_lagrange_radii_f64")
METHODS = ("radial_order_f64", "lagrange_f64", "radial_profile_f64")


def test_the_two_symbols_are_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = nb.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert getattr(L, s).argtypes is not None, f"{s} has no prototype in parallelnbody_amd/_lib.py"
    assert [len(getattr(L, s).argtypes) for s in SYMBOLS] == [6, 6]
    for name in METHODS:
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__
    assert int(re.search(r"#define NBODY_LAGRANGE_MAX (\d+)", text).group(1)) == nb._lib.LAGRANGE_MAX == 64
    assert "stay with the caller" not in text                      # nbody_mass_within points at the new call


def test_struct_nbody_lagrange_is_forty_bytes(nb):
    S = nb._lib.Lagrange
    assert ctypes.sizeof(S) == 40 == R.ROW.itemsize
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == \
        [("fraction", 0), ("r2", 8), ("radius", 16), ("mass", 24), ("body", 32), ("count", 36)]
    assert [(f, R.ROW.fields[f][1]) for f in R.ROW.names] == [(f, getattr(S, f).offset) for f, _ in S._fields_]
    from parallelnbody_amd.engine import LAGRANGE_FRACTIONS
    assert tuple(LAGRANGE_FRACTIONS) == R.FRACTIONS


def test_the_command_line_refuses_lagrange_lines_it_cannot_print(capsys):
    from parallelnbody_amd.__main__ import main
    f64 = ["--lagrange-every", "2", "--precision", "f64"]
    for argv, why in ((["--lagrange-every", "2"], "--lagrange-every needs --precision f64"),
                      (["--lagrange-every", "2", "--precision", "f32_kahan"], "--lagrange-every needs --precision f64"),
                      (["--lagrange-every", "-1", "--precision", "f64"], "--lagrange-every must be >= 0"),
                      (f64 + ["--core-k", "1"], "--core-k must be 2 .. 8"), (f64 + ["--core-k", "9"], "--core-k must be 2 .. 8"),
                      (f64 + ["--lagrange-fractions", "0.5,0"], "--lagrange-fractions must be"),
                      (f64 + ["--lagrange-fractions", "0.5,1.5"], "--lagrange-fractions must be"),
                      (f64 + ["--lagrange-fractions", "0.5,nan"], "--lagrange-fractions must be"),
                      (f64 + ["--lagrange-fractions", "half"], "--lagrange-fractions must be"),
                      (f64 + ["--lagrange-fractions", ",".join(["0.5"] * 65)], "--lagrange-fractions must be"),
                      (["--precision", "f64", "--lagrange-fractions", "0.5"], "--lagrange-fractions belongs to --lagrange-every")):
        with pytest.raises(SystemExit) as er:
            main(argv)
        assert er.value.code == 2
        assert why in capsys.readouterr().err, argv


# ---- the scan ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SIZES)
def test_the_scan_mirror_stays_within_the_bound_of_any_summation_order(n):
    c = R.gauss_case(n)
    exact = np.cumsum(c["w"].astype(LD))
    err = float(np.abs(c["cum"].astype(LD) - exact).max())
    bound = n * 2.0 ** -53 * float(np.abs(c["w"]).sum())
    print(f"N = {n}: the blocked scan is within {err:.3e} of the long-double sum; the bound of any order is {bound:.3e}")
    assert err <= bound
    assert (np.diff(c["cum"]) >= 0.0).all()                        # non-decreasing for non-negative masses
    assert c["total"] == c["cum"][-1]


def test_the_scan_mirror_is_the_definition_addition_by_addition():
    w = np.random.default_rng(4).uniform(0.0, 1.0, 700)
    want, off = np.zeros(700), 0.0
    for b in range(0, 700, 256):
        acc = None
        for p in range(b, min(b + 256, 700)):
            acc = w[p] if acc is None else acc + w[p]
            want[p] = off + acc
        for _ in range(min(b + 256, 700), b + 256):                # the padding of the last block
            acc = acc + 0.0
        off = off + acc
    assert R.scan(w).tobytes() == want.tobytes()
    assert R.scan(np.array([0.25])).tolist() == [0.25]


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------

def test_bodies_at_equal_distance_come_out_in_index_order():
    posm = np.zeros((13, 4)); posm[:, 3] = 1.0
    axes = np.array([[2, 0, 0], [0, 2, 0], [0, 0, 2], [-2, 0, 0], [0, -2, 0], [0, 0, -2]], np.float64)
    posm[1:7, :3] = axes[::-1]                                     # six bodies at d2 = 4 ...
    posm[7:13, :3] = 0.5 * axes                                    # ... six at d2 = 1, behind them in index order; body 0 on the centre
    order, d2s, cum, n_finite, _ = R.radial(posm, np.zeros(3))
    assert order.tolist() == [0] + list(range(7, 13)) + list(range(1, 7))
    assert d2s.tolist() == [0.0] + [1.0] * 6 + [4.0] * 6 and n_finite == 13 and cum.tolist() == list(np.arange(1.0, 14.0))
    posm[3, 0] = np.nan; posm[9, 1] = np.inf                        # a NaN comes last, +inf before it, and neither adds mass
    order, d2s, cum, n_finite, _ = R.radial(posm, np.zeros(3))
    assert order.tolist()[-2:] == [9, 3] and n_finite == 11 and np.isinf(d2s[-2]) and np.isnan(d2s[-1])
    assert cum[-1] == cum[-2] == cum[-3] == 11.0


def test_dyadic_masses_select_position_511_by_the_comparison_alone():
    posm = R.dyadic_scene()
    order, d2s, cum, n_finite, w = R.radial(posm, np.zeros(3))
    assert (cum == np.arange(1, 1025) * 2.0 ** -10).all() and cum[-1] == 1.0   # every partial sum is exact
    rows, total = R.select(order, d2s, cum, (0.5, 1.0, 2.0 ** -10))
    assert rows["count"].tolist() == [512, 1024, 1] and rows["mass"].tolist() == [0.5, 1.0, 2.0 ** -10] and total == 1.0
    assert rows["body"].tolist() == [order[511], order[1023], order[0]]
    p, gap, _ = R.select_ld(w, (0.5,))
    assert p[0] == 511 and gap[0] == 0.0                           # a tie: no gap — decided by >=, not by the arithmetic


def test_equal_masses_and_round_fractions_do_not_meet_the_gap_condition():
    w = np.full(1000, 1.0 / 1000)
    assert R.scan(w)[499] == 0.5 * R.scan(w)[-1]                    # to the last bit: such scenes are no index yardstick
    assert R.select_ld(w, (0.5,))[1][0] < R.gap_bound(1000)


def test_a_plummer_spheres_half_mass_radius():
    posm, a = R.plummer_half_mass()
    order, d2s, cum, _, _ = R.radial(posm, np.zeros(3))
    rows, _ = R.select(order, d2s, cum, (0.5,))
    want = a / np.sqrt(2.0 ** (2.0 / 3.0) - 1.0)
    assert abs(want - 1.3048 * a) < 1e-4 and abs(rows["radius"][0] / want - 1.0) < 0.03   # 20000 bodies: ~1 % sampling noise
    assert rows["radius"][0] == np.sqrt(rows["r2"][0]) and rows["r2"][0] == d2s[rows["count"][0] - 1]


def test_nothing_qualifies_without_a_positive_total():
    order, d2s = np.arange(3, dtype=np.int32), np.array([1.0, 2.0, 3.0])
    for cum in (np.zeros(3), np.array([1.0, 0.0, -1.0]), np.array([1.0, 2.0, np.nan])):
        rows, _ = R.select(order, d2s, cum, (0.5, 1.0))
        assert rows["body"].tolist() == [-1, -1] and rows["count"].tolist() == [0, 0] and np.isnan(rows["r2"]).all()
    rows, _ = R.select(order, d2s, np.array([2.0, -1.0, 1.0]), (0.5, 1.0))       # negative masses: the FIRST position, linearly
    assert rows["count"].tolist() == [1, 1]


# ---- radial_profile ---------------------------------------------------------------------------------------------------------------------

def test_radial_profile_on_a_hand_made_three_shell_system():
    from parallelnbody_amd.engine import radial_profile
    # shell 0: two bodies at r = 1 moving radially outwards at 1 and 3 (masses 1 and 1); shell 1: two bodies at r = 2 on circular
    # motion, speed 2, masses 1 and 3; shell 2: one body at r = 4 at rest
    posm = np.array([[1, 0, 0, 1], [0, -1, 0, 1], [0, 2, 0, 1], [0, 0, -2, 3], [4, 0, 0, 2]], np.float64)
    vel = np.array([[1, 0, 0], [0, -3, 0], [2, 0, 0], [0, 2, 0], [0, 0, 0]], np.float64)
    order = np.array([0, 1, 2, 3, 4])
    count, p = radial_profile(order, posm, vel, np.zeros(3), counts=[2, 4, 5], radii=[1.0, 2.0, 4.0], vcentre=np.zeros(3))
    assert count.tolist() == [2, 2, 1] and p["mass"].tolist() == [2.0, 4.0, 2.0]
    assert p["r_in"].tolist() == [0.0, 1.0, 2.0] and p["r_out"].tolist() == [1.0, 2.0, 4.0]
    vol = 4.0 * np.pi / 3.0
    assert np.allclose(p["density"], [2.0 / vol, 4.0 / (vol * 7.0), 2.0 / (vol * 56.0)], rtol=1e-15)
    assert p["v_r"].tolist() == [2.0, 0.0, 0.0] and p["sigma_r2"].tolist() == [1.0, 0.0, 0.0]
    assert p["sigma_t2"].tolist() == [0.0, 4.0, 0.0]
    assert p["beta"][0] == 1.0 and p["beta"][1] == -np.inf and np.isnan(p["beta"][2])
    # vcentre = None: each shell's own mass-weighted mean velocity is taken out first
    count, q = radial_profile(order, posm, vel, np.zeros(3), counts=[2, 4, 5], radii=[1.0, 2.0, 4.0])
    vc = np.array([0.5, -1.5, 0.0])                                # shell 0's mean velocity
    u = vel[:2] - vc
    ur = np.array([u[0, 0], -u[1, 1]])
    assert q["v_r"][0] == ur.mean() and q["sigma_r2"][0] == ((ur - ur.mean()) ** 2).mean()
    assert q["sigma_t2"][0] == ((u * u).sum(1) - ur * ur).mean()
    # an empty shell (a repeated count) has no mass and NaN means
    count, z = radial_profile(order, posm, vel, np.zeros(3), counts=[2, 2, 5], radii=[1.0, 1.0, 4.0], vcentre=np.zeros(3))
    assert count.tolist() == [2, 0, 3] and z["mass"][1] == 0.0 and np.isnan(z["v_r"][1])


# ---- the gap condition on everything the GPU tests compare an index for -------------------------------------------------------------

@pytest.mark.parametrize("n", R.SIZES)
def test_the_gap_condition_on_every_scene_and_fraction_the_gpu_tests_use(n):
    c = R.gauss_case(n)
    print(f"N = {n}: smallest gap {c['gap'].min():.3e} over {len(R.FRACTIONS)} fractions; the bound is {R.gap_bound(n):.3e}")
    assert (c["gap"] >= R.gap_bound(n)).all()                       # no pair left out
    assert (c["p_ld"] + 1 == c["rows"]["count"]).all()             # ... and there the fp64 mirror selects the long-double body
