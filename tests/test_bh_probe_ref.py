"""The yardstick of the field queries at theta > 0 (tests/cpp/bh_probe_ref.c: the reference's octree walked from arbitrary points)
against the checkers the project already trusts: with the points set to the bodies' own positions it IS the oracle's octree path —
every bit of the accelerations, the root CoM, the node count — and, with softening, the softened restatement's.  Any other point goes
through the same walk function.  No GPU."""
import os

import numpy as np
import pytest

from bh_probe_ref import ProbeRef
from bh_softened_ref import SoftenedRef

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["refbox_n2000_seed1", "plummer_n1024_seed1"]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return ProbeRef(tmp_path_factory.mktemp("bh_probe_ref"))


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return SoftenedRef(tmp_path_factory.mktemp("bh_softened_ref"))


def _bodies(fixture):
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    return np.ascontiguousarray(g["posm"][:, :3]), np.ascontiguousarray(g["posm"][:, 3])


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("fixture", FIXTURES)
def test_at_the_bodies_own_positions_it_is_the_oracle(oracle, probe, fixture, theta, div_mode):
    pos, m = _bodies(fixture)
    ref, com, nodes = oracle.octree_forces_f32(pos, m, theta, pow_mode=3, div_mode=div_mode)
    got, gcom, gnodes = probe.field(pos, m, pos, theta, div_mode=div_mode)
    assert got.tobytes() == ref.tobytes()
    assert gcom.tobytes() == com.tobytes() and gnodes == nodes


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("fixture", FIXTURES)
def test_softened_at_the_bodies_own_positions_it_is_the_softened_restatement(probe, soft, fixture, theta, div_mode):
    pos, m = _bodies(fixture)
    ref, com, nodes = soft.forces(pos, m, theta, eps=0.05, div_mode=div_mode)
    got, gcom, gnodes = probe.field(pos, m, pos, theta, eps=0.05, div_mode=div_mode)
    assert got.tobytes() == ref.tobytes()
    assert gcom.tobytes() == com.tobytes() and gnodes == nodes
    plain, _, _ = probe.field(pos, m, pos, theta, div_mode=div_mode)
    assert plain.tobytes() != got.tobytes()                        # (the softening is in the term)


def test_a_point_does_not_see_the_other_points(probe):
    pos, m = _bodies(FIXTURES[0])
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1500, 1500, (100, 3)).astype(np.float32)
    pts[0] = pos[5]                                                # on a body: its own leaf is d == 0
    all_, com, _ = probe.field(pos, m, pts, 1.0)
    one, _, _ = probe.field(pos, m, pts[17:18], 1.0)
    assert one.tobytes() == all_[17:18].tobytes()
    own, _, _ = probe.field(pos, m, pos, 1.0)
    assert all_[0].tobytes() == own[5].tobytes()
    at_com, _, _ = probe.field(pos, m, com[None, :], 1.0)          # d == 0 at the root ends the walk (OctreeSearch.h:102)
    assert not at_com.any()
    assert np.isfinite(all_).all()
