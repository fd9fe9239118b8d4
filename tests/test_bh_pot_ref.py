"""The yardstick of the potential at theta > 0 (tests/cpp/bh_pot_ref.c) against what the project already trusts.  Its tree and its
walk are those of tests/cpp/bh_probe_ref.c — accelerations, root CoM and node count equal in every byte —, and the potential it sums
in that walk is pinned from three sides: a walk that opens every cell is the direct sum, a probe on the root's CoM gets exactly 0, a
probe far outside exactly the root's single term.  No GPU."""
import numpy as np
import pytest

from bh_pot_ref import PotRef, direct_potential
from bh_probe_ref import G, ProbeRef, eps2f
from probe_scenes import N_PROBES, bodies, probes_for

# A walk that opens every cell adds one term G m_j / ds_j per body, all of one sign, so the sum's relative error is at most a term's:
# the fp32 differences (1 rounding each, doubled by the square), the squares (1), the two adds (2) put at most 5 * 2^-24 on d2, half of
# that on d; the root adds 1, the softening's add at most 1, the final rounding to fp32 1; the double operations 2^-53 each.  Below
# 5 * 2^-24 = 2.98e-7 in all; measured on these scenes: 4.8e-8 (the fp64 sum) and 7.4e-8 (rounded).
TOL_POT = 5 * 2.0 ** -24


@pytest.fixture(scope="module")
def pot(tmp_path_factory):
    return PotRef(tmp_path_factory.mktemp("bh_pot_ref"))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return ProbeRef(tmp_path_factory.mktemp("bh_probe_ref"))


def scene(nb, n):
    posm, _ = bodies(nb, n)
    return np.ascontiguousarray(posm[:, :3]), np.ascontiguousarray(posm[:, 3])


def points(pos, root_com):
    """tests/test_field_gpu.py's tree_probes: the 777 probes, the root's CoM, a far point, a point on a body, one 1e-3 beside a body."""
    extra = np.array([root_com, (1e6, 1e6, 1e6), pos[123], pos[321] + np.float32(1e-3)], np.float32)
    return np.concatenate([probes_for(pos, N_PROBES), extra])


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("n", [2000, 5000])
def test_same_tree_same_walk_as_the_field_yardstick(nb, pot, probe, n, eps, div_mode):
    pos, mass = scene(nb, n)
    _, com, _ = probe.field(pos, mass, pos[:1], 1.0, eps=eps, div_mode=div_mode)
    pts = np.concatenate([points(pos, com), pos])                 # ... and from every body's own position
    ref, rcom, rnodes = probe.field(pos, mass, pts, 1.0, eps=eps, div_mode=div_mode)
    got = pot.walk(pos, mass, pts, 1.0, eps=eps, div_mode=div_mode)
    assert got["acc"].tobytes() == ref.tobytes()
    assert got["root_com"].tobytes() == rcom.tobytes() and got["nodes"] == rnodes
    assert got["phi"].tobytes() == (got["phi64"]).astype(np.float32).tobytes()
    assert np.isfinite(got["phi64"]).all() and (got["phi64"] <= 0.0).all()
    one = pot.walk(pos, mass, pts[17:18], 1.0, eps=eps, div_mode=div_mode)      # a point does not see the other points
    assert one["phi64"].tobytes() == got["phi64"][17:18].tobytes()


@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("n", [2000, 5000])
def test_a_walk_that_opens_every_cell_is_the_direct_sum(nb, pot, n, eps):
    pos, mass = scene(nb, n)
    pts = np.concatenate([probes_for(pos, N_PROBES), pos[::7]])
    got = pot.walk(pos, mass, pts, 1e-30, eps=eps)
    ref = direct_potential(pos, mass, pts, eps=eps)
    if eps > 0.0:
        # at d == 0 the walk ends before the term (OctreeSearch.h:102), softened or not: a point ON a body does not feel that body's
        # G m / eps in a walk.  The direct sum of the theta == 0 definition does; take it out where the point is a body's position.
        on = np.concatenate([np.arange(50), np.arange(N_PROBES, pts.shape[0])])
        body = np.concatenate([np.arange(50), np.arange(0, n, 7)])
        ref[on] += G * mass[body].astype(np.float64) / eps
    e64 = np.abs(got["phi64"] - ref) / np.abs(ref)
    e32 = np.abs(got["phi"].astype(np.float64) - ref) / np.abs(ref)
    print(f"bh_pot_ref theta=1e-30 N={n} eps={eps}: max rel err fp64 sum {e64.max():.3e}, rounded {e32.max():.3e}")
    assert e64.max() < TOL_POT and e32.max() < TOL_POT


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("n", [2000, 5000])
def test_the_root_com_probe_and_the_far_probe(nb, pot, n, eps, div_mode):
    pos, mass = scene(nb, n)
    first = pot.walk(pos, mass, pos[:1], 1.0, eps=eps, div_mode=div_mode)
    com, M = first["root_com"], np.float32(first["root_mass"])
    far = np.array([1e6, 1e6, 1e6], np.float32)
    got = pot.walk(pos, mass, np.stack([com, far]), 1.0, eps=eps, div_mode=div_mode)
    assert got["phi64"][0] == 0.0 and got["phi"][0] == 0.0 and not got["acc"][0].any()   # d == 0 at the root ends the walk there
    e = far - com                                                 # fp32, the walk's own order
    d2 = np.float32(np.float32(e[0] * e[0]) + np.float32(e[1] * e[1]))
    d2 = np.float32(d2 + np.float32(e[2] * e[2]))
    ds = np.sqrt(np.float32(d2 + eps2f(eps)))
    assert ds.dtype == np.float32
    term = -(G * float(M) / float(ds))
    assert got["phi64"][1] == term and got["phi"][1] == np.float32(term)
