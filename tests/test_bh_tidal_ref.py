"""The yardsticks of the tidal tensor (tests/bh_tidal_ref.py: tests/cpp/bh_tidal_ref.c at theta > 0, direct_tidal at theta == 0) pinned
against each other and against what the project already trusts.  No GPU.

The walk's term takes the fp32 differences and the fp32 root the walk itself decides on (include/nbody.h), so on an arbitrary scene a
walk that opens every cell differs from the fp64 direct sum by fp32 roundings, a few 1e-7.  The 1e-12 comparisons therefore run on
LATTICE scenes on which every fp32 operation of the term is exact: bodies on integer points at an integer distance from the probe
(differences, squares, their sums and the root are then exact), so that what is left between the walk and direct_tidal is the order and
the rounding of fp64 operations — and any mistake in the formula.  The golden scene is compared as well, at the bound its fp32
roundings give."""
import numpy as np
import pytest

from bh_pot_ref import PotRef
from bh_tidal_ref import G, TidalRef, direct_tidal, frob
from probe_scenes import N_PROBES, bodies, probes_for

TOL_EXACT = 1e-12

# An arbitrary scene: the differences carry 2^-24 each, d2 five of them (tests/test_bh_pot_ref.py), ds half of that plus its own; a
# term 3 G m e_a e_b / ds^5 - G m / ds^3 then carries at most (2 + 5 * 3.5) * 2^-24 relative to 3 G m / ds^3, and ||T||_F is not smaller
# than a term's scale only where terms do not cancel — on these scenes (a heavy body at the origin) they do not; 32 * 2^-24 = 1.9e-6.
# Measured: 3.8e-7.
TOL_F32 = 32 * 2.0 ** -24


@pytest.fixture(scope="module")
def tidal(tmp_path_factory):
    return TidalRef(tmp_path_factory.mktemp("bh_tidal_ref"))


@pytest.fixture(scope="module")
def pot(tmp_path_factory):
    return PotRef(tmp_path_factory.mktemp("bh_pot_ref"))


def lattice_scene(seed, count=300, reach=40, radius=None):
    """`count` distinct integer points within +-reach whose distance from the origin is an integer (`radius`: that integer), masses
    1 .. 64 in whole numbers."""
    r = np.arange(-reach, reach + 1)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    d2 = (x * x + y * y + z * z).ravel()
    root = np.rint(np.sqrt(d2)).astype(np.int64)
    ok = (root * root == d2) & (d2 > 0)
    if radius is not None:
        ok &= root == radius
    cand = np.stack([x.ravel()[ok], y.ravel()[ok], z.ravel()[ok]], 1)
    rng = np.random.default_rng(seed)
    pick = rng.choice(cand.shape[0], min(count, cand.shape[0]), replace=False)
    return cand[pick].astype(np.float32), rng.integers(1, 65, pick.size).astype(np.float32)


def err(got, ref):
    return frob(np.asarray(got, np.float64) - ref) / frob(ref)


@pytest.mark.parametrize("shift", [(0, 0, 0), (7, -3, 11), (-64, 128, 5)])
@pytest.mark.parametrize("seed", [1, 2])
def test_a_walk_that_opens_every_cell_is_the_direct_sum(tidal, seed, shift):
    pos, mass = lattice_scene(seed)
    shift = np.array(shift, np.float32)
    pos, pt = pos + shift, shift[None, :].copy()
    got = tidal.walk(pos, mass, pt, 1e-30)
    ref = direct_tidal(pos, mass, pt)
    assert got["nodes"] > pos.shape[0] and frob(ref)[0] > 0.0
    e = err(got["t64"], ref)[0]
    tr = abs(got["t64"][0, :3].sum()) / frob(got["t64"])[0]
    print(f"bh_tidal_ref theta=1e-30 lattice seed={seed} shift={shift}: rel err {e:.3e}, |trace| / ||T|| {tr:.3e}")
    assert e < TOL_EXACT
    assert tr < TOL_EXACT                                          # eps == 0: the tensor is trace-free
    assert got["t"].tobytes() == got["t64"].astype(np.float32).tobytes()


def test_a_softened_walk_that_opens_every_cell_is_the_direct_sum(tidal):
    # every body 5 away, eps = 12: s = 13 exactly.  The trace is -3 sum G m eps^2 / s^5.
    pos, mass = lattice_scene(3, count=24, reach=5, radius=5)
    assert pos.shape[0] >= 20
    pt = np.zeros((1, 3), np.float32)
    got = tidal.walk(pos, mass, pt, 1e-30, eps=12.0)
    ref = direct_tidal(pos, mass, pt, eps=12.0)
    assert err(got["t64"], ref)[0] < TOL_EXACT
    want = -3.0 * G * float(mass.astype(np.float64).sum()) * 144.0 / 13.0 ** 5
    assert got["t64"][0, :3].sum() == pytest.approx(want, rel=TOL_EXACT) and ref[0, :3].sum() == pytest.approx(want, rel=TOL_EXACT)


@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_the_golden_scene_within_its_fp32_roundings(nb, tidal, eps):
    posm, _ = bodies(nb, 2000)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    pts = probes_for(pos, N_PROBES)[50:]                          # (probes 0-49 sit ON bodies: below)
    got = tidal.walk(pos, mass, pts, 1e-30, eps=eps)
    ref = direct_tidal(pos, mass, pts, eps=eps)
    e = err(got["t64"], ref)
    print(f"bh_tidal_ref theta=1e-30 N=2000 eps={eps}: max rel err {e.max():.3e}")
    assert e.max() < TOL_F32
    if eps == 0.0:
        tr = np.abs(ref[:, :3].sum(1)) / frob(ref)                # the direct sum's own trace: fp64 roundings only
        assert tr.max() < TOL_EXACT


def test_a_single_body_on_the_x_axis(tidal):
    for m, r, eps in [(3.0, 4.0, 0.0), (5000.0, 0.125, 0.0), (7.0, 3.0, 4.0)]:
        pos, mass = np.array([[r, 0.0, 0.0]], np.float32), np.array([m], np.float32)
        pt = np.zeros((1, 3), np.float32)
        s = float(np.sqrt(r * r + eps * eps))
        want = np.array([3.0 * G * m * r * r / s ** 5 - G * m / s ** 3, -G * m / s ** 3, -G * m / s ** 3, 0.0, 0.0, 0.0])
        if eps == 0.0:
            assert np.allclose(want, G * m / r ** 3 * np.array([2.0, -1.0, -1.0, 0.0, 0.0, 0.0]), rtol=1e-15, atol=0.0)
        for theta in (1e-30, 1.0):
            got = tidal.walk(pos, mass, pt, theta, eps=eps, root_size=r)["t64"][0]
            assert np.abs(got - want).max() <= TOL_EXACT * np.abs(want).max(), (m, r, eps, theta, got, want)
            assert (got[3:] == 0.0).all()
        assert np.abs(direct_tidal(pos, mass, pt, eps=eps)[0] - want).max() <= TOL_EXACT * np.abs(want).max()


@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_from_a_bodys_own_position_its_own_leaf_adds_nothing(nb, tidal, eps):
    # d == 0 ends the walk at the body's own leaf before the term (OctreeSearch.h:102), softened or not: the walk from body i's
    # position is the walk of the scene without body i (every cell open: the same leaves, in the order of another tree)
    posm, _ = bodies(nb, 2000)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    size = float(np.max(np.abs(pos)))
    for i in (0, 17, 1671, 1999):
        keep = np.arange(2000) != i
        own = tidal.walk(pos, mass, pos[i:i + 1], 1e-30, eps=eps, root_size=size)["t64"]
        without = tidal.walk(pos[keep], mass[keep], pos[i:i + 1], 1e-30, eps=eps, root_size=size)["t64"]
        assert err(own, without)[0] < TOL_EXACT, (i, eps)
        if eps > 0.0:                                             # ... where the theta == 0 definition has the body's -G m / eps^3
            at = direct_tidal(pos, mass, pos[i:i + 1], eps=eps)[0]
            skip = direct_tidal(pos, mass, pos, eps=eps, skip_self=True)[i]
            d = at - skip
            assert np.abs(d[:3] + G * float(mass[i]) / eps ** 3).max() <= 1e-9 * G * float(mass[i]) / eps ** 3 and np.abs(d[3:]).max() == 0.0


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("n", [2000, 5000])
def test_same_tree_same_walk_as_the_potential_yardstick(nb, tidal, pot, n, eps, div_mode):
    posm, _ = bodies(nb, n)
    pos, mass = np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])
    first = pot.walk(pos, mass, pos[:1], 1.0, eps=eps, div_mode=div_mode)
    extra = np.array([first["root_com"], (1e6, 0.0, 0.0), pos[123], pos[321] + np.float32(1e-3)], np.float32)
    pts = np.concatenate([probes_for(pos, N_PROBES), extra, pos])
    ref = pot.walk(pos, mass, pts, 1.0, eps=eps, div_mode=div_mode)
    got = tidal.walk(pos, mass, pts, 1.0, eps=eps, div_mode=div_mode)
    assert got["acc"].tobytes() == ref["acc"].tobytes()
    assert got["root_com"].tobytes() == ref["root_com"].tobytes() and got["nodes"] == ref["nodes"]
    assert np.isfinite(got["t64"]).all()
    assert not got["t64"][N_PROBES].any()                         # d == 0 at the root ends the walk there
    one = tidal.walk(pos, mass, pts[17:18], 1.0, eps=eps, div_mode=div_mode)    # a point does not see the other points
    assert one["t64"].tobytes() == got["t64"][17:18].tobytes()
