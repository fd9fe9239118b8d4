"""The fp64 separation census without a device: the two symbols are declared and bound and the header states the radii of a pass, the
command line refuses what it must, the mirror of tests/pairs_f64_ref.py agrees with a plain Python double loop and with the group
census's links at every scene the group tests use, unsorted and repeated radii are each answered on their own, and the histogram helper
and the Landy-Szalay formula of parallelnbody_amd/engine.py give a hand-computed system's numbers."""
import os
import re

import numpy as np
import pytest

import groups_f64_ref as R
import pairs_f64_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbody_get_pair_counts_f64", "nbody_pair_counts_at_f64")
METHODS = ("pair_counts_f64", "pair_counts_at_f64", "pair_histogram_f64", "correlation_f64")


def test_the_two_symbols_are_declared_and_bound(nb):
    text = open(os.path.join(ROOT, "include", "nbody.h")).read()
    declared = set(re.findall(r"NBODY_AMD_API[^;]*?\b(nbody_[a-z0-9_]+)\s*\(", text, flags=re.S))
    L = nb.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/nbody.h"
        assert getattr(L, s).argtypes is not None, f"{s} has no prototype in parallelnbody_amd/_lib.py"
    assert [len(getattr(L, s).argtypes) for s in SYMBOLS] == [4, 7]
    for name in METHODS:
        assert callable(getattr(nb.NBodyEngine, name)) and getattr(nb.NBodyEngine, name).__doc__
    assert int(re.search(r"#define NBODY_PAIR_RADII_MAX (\d+)", text).group(1)) == nb._lib.PAIR_RADII_MAX == P.K_MAX == 64
    assert int(re.search(r"#define NBODY_PAIR_RADII_PER_PASS (\d+)", text).group(1)) == nb._lib.PAIR_RADII_PER_PASS == P.G
    kernels = open(os.path.join(ROOT, "parallelnbody_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"#define NBODY_PAIRS64_GROUP (\d+)", kernels).group(1)) == P.G      # the kernel's group is the header's


def test_the_command_line_refuses_pair_lines_it_cannot_print(capsys):
    from parallelnbody_amd.__main__ import main
    f64 = ["--pairs-every", "2", "--precision", "f64"]
    for argv, why in ((["--pairs-every", "2", "--pair-radii", "0.1"], "--pairs-every needs --precision f64"),
                      (["--pairs-every", "-1", "--precision", "f64", "--pair-radii", "0.1"], "--pairs-every must be >= 0"),
                      (f64, "--pairs-every needs --pair-radii"),
                      (["--precision", "f64", "--pair-radii", "0.1"], "--pair-radii belongs to --pairs-every"),
                      (f64 + ["--pair-radii", "0.1,-0.5"], "--pair-radii must be"),
                      (f64 + ["--pair-radii", "nan"], "--pair-radii must be"),
                      (f64 + ["--pair-radii", "0.1,x"], "--pair-radii must be"),
                      (f64 + ["--pair-radii", ",".join(["0.1"] * 65)], "--pair-radii must be")):
        with pytest.raises(SystemExit) as er:
            main(argv)
        assert er.value.code == 2
        assert why in capsys.readouterr().err, argv


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 2, 7, 64))
def test_the_mirror_against_a_plain_double_loop(n):
    posm = R.gauss_scene(n)
    radii = np.array([0.7, 0.0, 3.0, 0.2, 0.7, 100.0, 1.3])         # unsorted, a repeat, 0 and one beyond the system
    want = P.pairs_plain(posm, radii)
    got = P.pair_counts(posm, radii)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    assert got[-2] == n * (n - 1) // 2 and got[1] == 0 and got[0] == got[4]
    points = np.random.default_rng(5).normal(0.0, 1.0, (9, 3))
    points[3] = posm[n - 1, :3]                                     # on a body: that body counts, at radius 0 too
    at = P.pair_counts_at(points, posm, radii)
    assert at.tolist() == P.at_plain(points, posm, radii).tolist()
    assert at[1] == 1 and at[-2] == 9 * n
    assert P.pair_counts_at(np.zeros((0, 3)), posm, radii).tolist() == [0] * len(radii)
    # the points at the bodies' own positions: every ordered pair and every body on itself
    assert P.pair_counts_at(posm[:, :3], posm, radii).tolist() == (2 * got + n).tolist()


def test_the_mirror_with_bodies_that_are_not_finite_and_coincident():
    posm = np.array(R.gauss_scene(40))
    posm[3, 0] = np.nan; posm[9, 1] = np.inf; posm[11, 2] = -np.inf; posm[20, :3] = posm[21, :3]
    radii = np.array([0.0, 0.5, 1e3])
    got = P.pair_counts(posm, radii)
    assert got.tolist() == P.pairs_plain(posm, radii).tolist()
    assert got[0] == 1 and got[2] == 37 * 36 // 2                   # the coincident pair; the three bodies that are not finite count nowhere
    at = P.pair_counts_at(posm[:, :3], posm, radii)
    assert at.tolist() == P.at_plain(posm[:, :3], posm, radii).tolist() == (2 * got + 37).tolist()


@pytest.mark.parametrize("name,radius", R.cases())
def test_the_mirror_counts_the_group_census_links(name, radius):
    assert int(P.pair_counts(R.scene(name), [radius])[0]) == R.case(name, radius)["summary"].links


def test_unsorted_and_repeated_radii_are_each_answered_on_their_own():
    posm = R.scene("gauss1000")
    radii = np.array([0.4, 0.05, 0.4, 0.0, 50.0, 0.2, 0.05, 0.2000000000000001])
    got = P.pair_counts(posm, radii)
    assert got.tolist() == [int(P.pair_counts(posm, [r])[0]) for r in radii]
    assert got[0] == got[2] and got[1] == got[6] and got[3] == 0 and got[4] == 1000 * 999 // 2
    assert (got[np.argsort(radii, kind="stable")][1:] >= got[np.argsort(radii, kind="stable")][:-1]).all()      # C(r) never falls
    for k in (1, P.G - 1, P.G, P.G + 1, P.K_MAX):
        r = P.radii_set(k, 0.02, 3.0)
        assert len(set(r.tolist())) == k and P.pair_counts(posm, r).tolist() == P.pair_counts(posm, np.sort(r))[np.argsort(np.argsort(r))].tolist()


# ---- the helpers of engine.py --------------------------------------------------------------------------------------------------------------

def test_the_histogram_of_four_bodies_on_a_line():
    from parallelnbody_amd.engine import pair_histogram
    posm = np.zeros((4, 4)); posm[:, 0] = (0.0, 1.0, 3.0, 6.0)      # separations 1, 3, 6, 2, 5, 3
    edges = np.array([0.0, 1.0, 2.0, 3.0, 6.0])
    cumulative = P.pair_counts(posm, edges)
    assert cumulative.tolist() == [0, 1, 2, 4, 6]
    hist = pair_histogram(edges, cumulative)
    assert hist.dtype == np.int64 and hist.tolist() == [1, 1, 2, 2]   # (0, 1], (1, 2], (2, 3], (3, 6]: the upper edge closed
    assert pair_histogram([1.0, 3.0], P.pair_counts(posm, [1.0, 3.0])).tolist() == [3]   # the lower edge OPEN: the pair at 1 is in no bin
    assert pair_histogram([2.0, 2.0, 5.0], [2, 2, 5]).tolist() == [0, 3]
    for bad in (([1.0], [0]), ([2.0, 1.0], [0, 0]), ([0.0, np.nan], [0, 0]), ([0.0, 1.0], [0, 1, 2])):
        with pytest.raises(ValueError):
            pair_histogram(*bad)


def test_the_landy_szalay_formula_by_hand():
    from parallelnbody_amd.engine import CorrelationResult, landy_szalay
    # 4 bodies (6 pairs), 5 randoms (10 pairs, 20 cross pairs):  DD = (1/3, 1/6), DR = (1/5, 3/10), RR = (3/10, 0)
    xi = landy_szalay([2, 1], [4, 6], [3, 0], 4, 5)
    assert xi.dtype == np.float64 and np.isnan(xi[1])               # no random pair in the bin: NaN
    assert abs(xi[0] - 7.0 / 9.0) < 4 * np.finfo(np.float64).eps    # (1/3 - 2/5 + 3/10) / (3/10) = 7/9, a few roundings
    same = landy_szalay([2, 4], [5, 10], [2, 4], 5, 5)              # DD = DR = RR = (1/5, 2/5): xi = 0
    assert np.abs(same).max() < 4 * np.finfo(np.float64).eps
    assert CorrelationResult._fields == ("xi", "dd", "dr", "rr")
