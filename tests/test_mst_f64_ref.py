"""The fp64 minimum spanning tree without a device: the symbol is declared and bound, struct nbody_mst is laid out as the header says,
the command line refuses what it must, and the two mirrors of tests/mst_f64_ref.py — Prim under the key (d2, i, j), and the device's
Boruvka rounds — give the same edges on every scene the GPU tests use; cutting the tree at a scene's linking lengths gives the labels
of tests/groups_f64_ref.py's groups; the rounds stay within ceil(log2 n) + 1; the length is numpy's cumulative sum."""
import ctypes
import os
import re

import numpy as np
import pytest

import groups_f64_ref as R
import mst_f64_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    assert "nbody_get_mst_f64" in declared
    assert len(nb.lib().nbody_get_mst_f64.argtypes) == 6
    for name in ("mst_f64", "mst_groups_f64"):
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__


def test_struct_nbody_mst_is_thirty_two_bytes(nb):
    S = nb._lib.Mst
    assert ctypes.sizeof(S) == 32
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == \
        [("edges", 0), ("components", 4), ("rounds", 8), ("reserved", 12), ("length", 16), ("longest_d2", 24)]
    from parallelnbody_amd.engine import MstResult, MstSummary
    assert MstSummary._fields == ("edges", "components", "rounds", "length", "longest_d2")
    assert tuple(f for f in MstSummary._fields if f != "rounds") == M.Summary._fields
    assert MstResult._fields == ("i", "j", "d2", "component", "summary")


def test_the_command_line_refuses_tree_lines_it_cannot_print(capsys):
    from parallelnbody_amd.__main__ import main
    for argv, why in ((["--mst-every", "2"], "--mst-every needs --precision f64"),
                      (["--mst-every", "2", "--precision", "f32_kahan"], "--mst-every needs --precision f64"),
                      (["--mst-every", "-1", "--precision", "f64"], "--mst-every must be >= 0")):
        with pytest.raises(SystemExit) as er:
            main(argv)
        assert er.value.code == 2
        assert why in capsys.readouterr().err, argv


# ---- the two mirrors ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.names())
def test_prim_and_the_rounds_agree_and_the_cut_is_the_groups(name):
    posm = R.scene(name)
    n = len(posm)
    want, got = M.case(name), M.rounds_scheme(posm)
    s = want["summary"]
    tied = int((want["d2"][1:] == want["d2"][:-1]).sum())
    print(f"{name}: {s}, {got['passes']} passes, {tied} edges tied in d2")
    for f in ("i", "j", "d2", "component"):
        assert want[f].dtype == got[f].dtype and want[f].tobytes() == got[f].tobytes(), f
    assert got["summary"] == s
    assert (s.edges, s.components, got["passes"], tied) == M.EXPECTED[name]
    assert got["passes"] <= M.round_bound(n)
    # the output's own rules
    assert s.edges + s.components == n and len(want["i"]) == s.edges
    assert (want["i"] < want["j"]).all() and (want["i"] >= 0).all() and (want["j"] < n).all()
    key = list(zip(want["d2"].tolist(), want["i"].tolist(), want["j"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)
    assert want["d2"].tobytes() == M.d2_of(posm, want["i"], want["j"]).tobytes()
    assert s.length == (float(np.cumsum(np.sqrt(want["d2"]))[-1]) if s.edges else 0.0)
    assert s.longest_d2 == (float(want["d2"][-1]) if s.edges else 0.0)
    assert (want["component"] <= np.arange(n)).all() and len(np.unique(want["component"])) == s.components
    # cut at the scene's linking lengths: the groups' labels, exactly
    for radius in M.radii(name):
        groups = R.case(name, radius)
        assert M.cut(want, n, radius).tobytes() == groups["label"].tobytes(), radius


def test_the_round_bound():
    assert [M.round_bound(n) for n in (1, 2, 3, 4, 5, 256, 257, 4096, 4097, 32769)] == [1, 2, 3, 3, 4, 9, 10, 13, 14, 17]


def test_the_six_bodies_that_are_not_finite_are_components_of_their_own():
    t = M.case("nonfinite")
    for b in R.NONFINITE_BODIES:
        assert t["component"][b] == b and b not in t["i"] and b not in t["j"]
    assert t["summary"].components == 7 and t["summary"].edges == 293


def test_an_overflowing_distance_is_no_edge():
    posm = np.zeros((4, 4)); posm[:, 0] = (-1e160, -1e160 + 1e150, 1e160, 1e160 - 1e150)   # the two pairs are 2e160 apart: d2 = +inf
    t, r = M.prim(posm), M.rounds_scheme(posm)
    assert t["i"].tolist() == [0, 2] and t["j"].tolist() == [1, 3] and t["component"].tolist() == [0, 0, 2, 2]
    assert r["i"].tobytes() == t["i"].tobytes() and r["j"].tobytes() == t["j"].tobytes() and r["passes"] == 2


def test_mst_groups_is_the_cut(nb):
    from parallelnbody_amd.engine import MstResult, MstSummary
    for name in ("gauss1000", "lattice", "coincident", "nonfinite"):
        t, n = M.case(name), len(R.scene(name))
        s = t["summary"]
        mst = MstResult(t["i"], t["j"], t["d2"], t["component"], MstSummary(s.edges, s.components, 0, s.length, s.longest_d2))
        for radius in M.radii(name):
            groups = R.case(name, radius)
            label, members = nb.NBodyEngine.mst_groups_f64(mst, radius)
            assert label.dtype == np.int32 and label.tobytes() == groups["label"].tobytes()
            assert members.dtype == np.int32 and members.tobytes() == groups["members"].tobytes()


def test_the_analytic_chain_is_what_prim_finds_at_a_size_prim_can_do():
    posm, want = M.chain_tree(1025)
    t = M.prim(posm)
    for f in ("i", "j", "d2", "component"):
        assert want[f].dtype == t[f].dtype and want[f].tobytes() == t[f].tobytes(), f
    assert t["summary"] == want["summary"]
