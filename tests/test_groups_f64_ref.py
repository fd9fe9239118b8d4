"""The fp64 group census without a device: the three symbols are declared and bound, struct nbody_groups is laid out as the header says,
the command line refuses what it must, the two mirrors of tests/groups_f64_ref.py — the definitions through a union-find, and the
device's rounds — agree on the labels of every scene the GPU tests use, d2 is symmetric in every bit, the hand-made edge cases come out
as the header says, group_table()'s formulas give a hand-made system's numbers, and the CHAIN CONDITION holds: the rounds scheme needs
at most 16 rounds on a 4096-body chain in permuted and in bit-reversed order, where plain label propagation needs thousands."""
import ctypes
import os
import re

import numpy as np
import pytest

import groups_f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbody_get_radius_counts_f64", "nbody_radius_counts_at_f64", "nbody_get_groups_f64")
METHODS = ("radius_counts_f64", "radius_counts_at_f64", "groups_f64", "group_table_f64")


def test_the_three_symbols_are_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = nb.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert getattr(L, s).argtypes is not None, f"{s} has no prototype in parallelnbody_amd/_lib.py"
    assert [len(getattr(L, s).argtypes) for s in SYMBOLS] == [3, 6, 6]
    for name in METHODS:
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__
    assert int(re.search(r"NBODY_ERR_INTERNAL = (-\d+)", text).group(1)) == nb._lib.ERR_INTERNAL == -7


def test_struct_nbody_groups_is_thirty_two_bytes(nb):
    S = nb._lib.Groups
    assert ctypes.sizeof(S) == 32
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == \
        [("groups", 0), ("multiples", 4), ("largest", 8), ("largest_members", 12), ("rounds", 16), ("reserved", 20), ("links", 24)]
    from parallelnbody_amd.engine import GroupsSummary
    assert GroupsSummary._fields == ("groups", "multiples", "largest", "largest_members", "rounds", "links")
    assert tuple(f for f in GroupsSummary._fields if f != "rounds") == R.Summary._fields


def test_the_command_line_refuses_group_lines_it_cannot_print(capsys):
    from parallelnbody_amd.__main__ import main
    f64 = ["--groups-every", "2", "--precision", "f64"]
    for argv, why in ((["--groups-every", "2", "--linking-length", "0.1"], "--groups-every needs --precision f64"),
                      (["--groups-every", "2", "--linking-length", "0.1", "--precision", "f32_kahan"], "--groups-every needs --precision f64"),
                      (["--groups-every", "-1", "--precision", "f64", "--linking-length", "0.1"], "--groups-every must be >= 0"),
                      (f64, "--groups-every needs --linking-length"),
                      (["--precision", "f64", "--linking-length", "0.1"], "--linking-length belongs to --groups-every"),
                      (f64 + ["--linking-length", "-0.5"], "--linking-length must be finite and >= 0"),
                      (f64 + ["--linking-length", "nan"], "--linking-length must be finite and >= 0"),
                      (f64 + ["--linking-length", "inf"], "--linking-length must be finite and >= 0")):
        with pytest.raises(SystemExit) as er:
            main(argv)
        assert er.value.code == 2
        assert why in capsys.readouterr().err, argv


# ---- the two mirrors ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,radius", R.cases())
def test_the_two_mirrors_agree_on_every_scene_the_gpu_tests_use(name, radius):
    g = R.case(name, radius)
    n = len(R.scene(name))
    label, rounds = R.rounds_scheme(n, g["i"], g["j"])
    print(f"{name} at b = {radius}: {g['summary']}, {rounds} rounds")
    assert label.tobytes() == g["label"].tobytes()
    assert rounds <= n and (rounds == 1) == (g["summary"].links == 0)
    assert (g["label"] <= np.arange(n)).all() and (g["label"][g["label"]] == g["label"]).all()   # the lowest index names a group
    assert (g["label"][g["i"]] == g["label"][g["j"]]).all()                                     # a link never crosses groups
    assert g["members"].sum() == (g["members"].astype(np.int64) ** 2)[g["label"] == np.arange(n)].sum()


@pytest.mark.parametrize("n", (1000, 4097))
def test_the_window_in_x_leaves_no_linked_pair_out(n):
    posm = R.scene(f"gauss{n}")
    for radius in R.gauss_radii(n) + (0.0, 3.0):
        a, b = R.pairs_full(posm, radius), R.pairs(posm, radius)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), radius


def test_d2_is_symmetric_in_every_bit():
    for scale in (1.0, 1e-150, 1e150, 1e-3):
        x = R.gauss_scene(700)[:, :3] * scale
        d2 = R.d2_block(x, x)
        assert d2.tobytes() == np.ascontiguousarray(d2.T).tobytes()
    i, j = R.pairs_full(R.scene("gauss1000"), 0.4)
    assert (i < j).all() and len(set(zip(i.tolist(), j.tolist()))) == len(i)


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------------------

def test_two_coincident_bodies_at_radius_zero():
    posm = np.array([[1.5, -2.0, 0.25, 1.0], [1.5, -2.0, 0.25, 1.0], [1.5, -2.0, 0.25000000000000006, 1.0]])
    g = R.groups(posm, 0.0)
    assert g["label"].tolist() == [0, 0, 2] and g["degree"].tolist() == [1, 1, 0] and g["members"].tolist() == [2, 2, 1]
    assert g["summary"] == R.Summary(groups=2, multiples=1, largest=0, largest_members=2, links=1)


def test_a_pair_exactly_at_the_radius_is_linked_and_one_ulp_outside_is_not():
    posm = np.array([[0.0, 0.0, 0.0, 1.0], [3.0, 4.0, 12.0, 1.0]])        # d2 = 169 = 13 * 13 exactly
    assert R.groups(posm, 13.0)["label"].tolist() == [0, 0]
    assert R.groups(posm, np.nextafter(13.0, 0.0))["label"].tolist() == [0, 1]
    out = posm.copy(); out[1, 2] = np.nextafter(12.0, 13.0)               # one ulp further: d2 rounds above 169
    assert R.d2_block(out[:1, :3], out[1:, :3])[0, 0] > 169.0
    assert R.groups(out, 13.0)["label"].tolist() == [0, 1]
    assert R.counts_at(posm[:, :3], posm, 13.0).tolist() == [2, 2] and R.counts_at(out[:, :3], out, 13.0).tolist() == [1, 1]


def test_a_nan_body_is_a_group_of_one():
    posm = np.zeros((5, 4)); posm[:, 0] = np.arange(5); posm[:, 3] = 1.0
    posm[2, 1] = np.nan                                             # the chain 0 - 1 - [2] - 3 - 4 is cut there
    g = R.groups(posm, 1.0)
    assert g["label"].tolist() == [0, 0, 2, 3, 3] and g["degree"].tolist() == [1, 1, 0, 1, 1]
    posm[2, 1] = np.inf
    assert R.groups(posm, 1.0)["label"].tolist() == [0, 0, 2, 3, 3]
    assert R.groups(posm, 2.0)["label"].tolist() == [0, 0, 2, 0, 0]   # 1 and 3 are 2 apart


def test_a_zero_mass_body_links_like_any_other():
    posm = np.zeros((3, 4)); posm[:, 0] = (0.0, 1.0, 2.0); posm[:, 3] = (1.0, 0.0, 1.0)
    g = R.groups(posm, 1.0)
    assert g["label"].tolist() == [0, 0, 0] and g["degree"].tolist() == [1, 2, 1]      # the massless one is the bridge


def test_group_table_on_a_hand_made_two_group_system():
    from parallelnbody_amd.engine import GROUP_TABLE_DTYPE, group_table
    # group 0: bodies 0 and 2, masses 1 and 3, on the x axis at 0 and 4, moving along y at 2 and -2; body 1 is alone; group 3: bodies 3, 4
    # and 5, equal masses, at (10, 0, 0), (10, 3, 0), (10, 0, 3), at rest
    posm = np.array([[0, 0, 0, 1], [50, 0, 0, 9], [4, 0, 0, 3], [10, 0, 0, 2], [10, 3, 0, 2], [10, 0, 3, 2]], np.float64)
    vel = np.array([[0, 2, 0], [7, 7, 7], [0, -2, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float64)
    label = np.array([0, 1, 0, 3, 3, 3], np.int32)
    t = group_table(label, posm, vel)
    assert t.dtype == GROUP_TABLE_DTYPE and t["label"].tolist() == [0, 3] and t["count"].tolist() == [2, 3]
    assert t["mass"].tolist() == [4.0, 6.0]
    assert t["com"].tolist() == [[3.0, 0.0, 0.0], [10.0, 1.0, 1.0]] and t["velocity"].tolist() == [[0.0, -1.0, 0.0], [0.0, 0.0, 0.0]]
    assert t["r_rms"][0] == np.sqrt((1 * 9.0 + 3 * 1.0) / 4.0) and t["sigma"][0] == np.sqrt((1 * 9.0 + 3 * 1.0) / 4.0)
    assert t["r_rms"][1] == np.sqrt((2 * 2.0 + 2 * 5.0 + 2 * 5.0) / 6.0) and t["sigma"][1] == 0.0
    assert group_table(label, posm, vel, min_members=1)["label"].tolist() == [0, 1, 3]
    assert group_table(label, posm, vel, min_members=3)["label"].tolist() == [3] and len(group_table(label, posm, vel, min_members=4)) == 0
    posm[[0, 2], 3] = 0.0                                           # a group of no mass: NaN, not an error
    z = group_table(label, posm, vel)
    assert z["mass"][0] == 0.0 and np.isnan(z["com"][0]).all() and np.isnan(z["sigma"][0]) and z["mass"][1] == 6.0


# ---- the chain condition ------------------------------------------------------------------------------------------------------------------

def propagation_rounds(n, i, j, cap):
    """plain min-label propagation, no hook at the root: the rounds it needs, or cap + 1"""
    label = np.arange(n)
    a, b = np.concatenate([i, j]), np.concatenate([j, i])
    for rounds in range(1, cap + 1):
        new = label.copy()
        np.minimum.at(new, a, label[b])
        if (new == label).all():
            return rounds
        label = new
    return cap + 1


@pytest.mark.parametrize("kind", ("permuted", "bitrev"))
def test_the_chain_condition(kind):
    g = R.case(f"chain_{kind}", 1.5)
    n = 4096
    assert g["summary"] == R.Summary(groups=1, multiples=1, largest=0, largest_members=n, links=n - 1)
    assert sorted(R.scene(f"chain_{kind}")[:, 0].tolist()) == list(range(n)) and g["degree"].max() == 2
    label, rounds = R.rounds_scheme(n, g["i"], g["j"])
    print(f"the {kind} chain of {n}: {rounds} rounds")
    assert (label == 0).all() and rounds <= 16
    assert propagation_rounds(n, g["i"], g["j"], 64) > 64           # what the condition keeps out
