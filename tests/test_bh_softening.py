"""The CPU restatement of the softened Barnes-Hut walk (tests/cpp/bh_softened_ref.c) against the oracle: at eps = 0 it IS the oracle's
octree path (every bit of the forces, the root CoM, the node count and the Ticks), and at an opening angle that opens every internal node
its softened term is the Plummer law of the fp64 direct sum.  No GPU."""
import os

import numpy as np
import pytest

from bh_softened_ref import SoftenedRef
from conftest import particles_from, rel_err

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return SoftenedRef(tmp_path_factory.mktemp("bh_softened_ref"))


def _scene(nb, n, kind, seed=1):
    if kind == "box":
        posm, vel = nb.ic_reference_box(n, 1000.0, seed=seed)
    else:
        posm, vel = nb.ic_plummer(n, seed=seed)
    return posm, vel


def _deep_pair(nb, n):
    """tests/test_bh_deep_gpu.py's "far" scene: a runaway body holds Size at 1e9, a pair 1e-4 apart at |x| ~ 500 goes below level 42."""
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=1)
    posm[0, :3] = (1.0e9, -2.0e8, 3.0e8)
    posm[0, 3] = np.float32(1e-6)
    posm[1, :3] = (500.25, 300.5, -200.75)
    posm[2, :3] = posm[1, :3] + np.float32(1e-4)
    vel[:3, :3] = 0.0
    return posm, vel


def _same_as_oracle(soft, oracle, posm, theta, div_mode, root=(0.0, 0.0, 0.0)):
    pos = np.ascontiguousarray(posm[:, :3]); m = np.ascontiguousarray(posm[:, 3])
    ref, com, nodes = oracle.octree_forces_f32(pos, m, theta, root_origin=root, pow_mode=3, div_mode=div_mode)
    got, gcom, gnodes = soft.forces(pos, m, theta, eps=0.0, root_origin=root, div_mode=div_mode)
    assert got.tobytes() == ref.tobytes(), (posm.shape[0], theta, div_mode)
    assert gcom.tobytes() == com.tobytes() and gnodes == nodes


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("theta", [0.5, 1.0])
@pytest.mark.parametrize("n,kind", [(2, "box"), (100, "box"), (2000, "box"), (2000, "plummer"), (65536, "box")])
def test_at_eps_zero_the_restatement_is_the_oracle(nb, oracle, soft, n, kind, theta, div_mode):
    posm, _ = _scene(nb, n, kind)
    _same_as_oracle(soft, oracle, posm, theta, div_mode, root=(0.0, 0.0, 0.0) if n != 100 else tuple(posm[3, :3]))


@pytest.mark.parametrize("fixture", ["refbox_n2000_seed1", "plummer_n1024_seed1"])
@pytest.mark.parametrize("div_mode", [0, 1])
def test_at_eps_zero_on_the_golden_fixtures(oracle, soft, fixture, div_mode):
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    _same_as_oracle(soft, oracle, g["posm"], 1.0, div_mode)


@pytest.mark.parametrize("div_mode", [0, 1])
def test_at_eps_zero_on_a_tree_deeper_than_42_levels(nb, oracle, soft, div_mode):
    posm, _ = _deep_pair(nb, 2000)
    assert oracle.octree_depth_f32(posm[:, :3]) > 42
    _same_as_oracle(soft, oracle, posm, 1.0, div_mode)


@pytest.mark.parametrize("div_mode", [0, 1])
@pytest.mark.parametrize("kind", ["box", "plummer"])
def test_at_eps_zero_five_ticks_are_the_oracle_ticks(nb, oracle, soft, kind, div_mode):
    posm, vel = _scene(nb, 2000, kind, seed=2)
    p = particles_from(nb, posm, vel)
    q = p.copy()
    com_p = com_q = None
    for frame in range(5):
        com_p, size_p = soft.tick(p, 0.01, 1.0, eps=0.0, root_com=com_p, div_mode=div_mode)
        com_q, size_q = oracle.tick_aos_f32(q, 0.01, theta=1.0, root_com=com_q, pow_mode=3, div_mode=div_mode)
        assert p.tobytes() == q.tobytes(), frame
        assert size_p == size_q and com_p.tobytes() == com_q.tobytes(), frame


def test_an_eps_whose_square_rounds_to_zero_is_eps_zero(nb, soft):
    posm, _ = _scene(nb, 2000, "box")
    pos = posm[:, :3]; m = posm[:, 3]
    a0, _, _ = soft.forces(pos, m, 1.0, eps=0.0)
    a1, _, _ = soft.forces(pos, m, 1.0, eps=1e-30)
    assert a0.tobytes() == a1.tobytes()


@pytest.mark.parametrize("eps", [1.0, 15.0, 500.0])       # below, about, far above the scenes' nearest-neighbour distances
@pytest.mark.parametrize("kind", ["box", "plummer"])
def test_every_node_opened_gives_the_plummer_law(nb, oracle, soft, kind, eps):
    # theta = 1e-30: no internal node passes Size / d < Theta, so every body's sum runs over the other bodies' leaves — the
    # softened direct sum, in the tree's order
    posm, _ = _scene(nb, 2000, kind)
    pos = posm[:, :3]; m = posm[:, 3]
    got, _, _ = soft.forces(pos, m, 1e-30, eps=eps)
    ref = oracle.forces_direct_f64(pos, m, eps=eps)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 2e-5
    # (body by body: ~2e-6 at the 99th percentile; a body whose terms nearly cancel loses a few more fp32 digits in the sum)
    assert rel_err(got, ref).max() < 1e-4
    unsoftened = oracle.forces_direct_f64(pos, m, eps=0.0)
    assert np.median(rel_err(unsoftened, ref)) > 1e-4          # (five times the tolerance: the law is not the unsoftened one)
