"""The continuation of Octree::Add below the path keys' 42 levels (csrc/bh_deep_path.h), compiled for the host: the level at which it
splits two bodies apart is the oracle's, on random pairs near the origin, far from it and under large roots; and the deep-tree
setting is declared in the header and bound in the Python layer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallelnbody_amd", "csrc")


def _pairs(rng, count):
    recs = []
    for k in range(count):
        kind = k % 3
        size = np.float32(10.0 ** rng.uniform(0, 9)) if kind != 2 else np.float32(1e9)
        centre = np.float32(rng.uniform(-0.5, 0.5) * size) * np.ones(3, np.float32) if kind == 1 else np.zeros(3, np.float32)
        if kind == 0:        # near the origin: tiny coordinates, tiny separations
            a = (rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-30, 0)).astype(np.float32)
        else:                # far from it
            a = (rng.uniform(-1, 1, 3) * size * 0.9).astype(np.float32)
        sep = (rng.uniform(-1, 1, 3) * np.abs(a).max() * 10.0 ** rng.uniform(-7, -1)).astype(np.float32)
        b = (a + sep).astype(np.float32)
        if np.array_equal(a, b):
            b = np.nextafter(a, np.float32(np.inf)).astype(np.float32)
        recs.append(np.concatenate([centre, [size], a, b]).astype(np.float32))
    return np.array(recs, np.float32)


def test_split_level_equals_the_oracle_depth(oracle, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "deep_split_level")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "deep_split_level.cpp"), "-o", exe])
    recs = _pairs(np.random.default_rng(7), 3000)
    path = tmp_path / "pairs.bin"
    recs.tofile(path)
    got = np.array(subprocess.check_output([exe, str(path)]).split(), int).reshape(-1, 2)
    assert got.shape[0] == recs.shape[0]
    deep = 0
    for r, (lev, before) in zip(recs, got):
        pos = np.stack([r[4:7], r[7:10]])
        depth = oracle.octree_depth_f32(pos, root_origin=r[0:3], root_size=r[3])
        assert lev + 1 == depth, (r.tolist(), lev, depth)
        deep += depth > 43
        if depth <= 200:                                             # the order of the two leaves: the oracle's depth-first walk
            _, order = oracle.octree_leaves_f32(pos, np.ones(2, np.float32), root_origin=r[0:3], root_size=r[3])
            assert before == (order[0] == 0), (r.tolist(), before, order)
    assert deep > 300, deep                                          # most of the pairs go below the keys' 42 levels


def test_the_setting_is_declared_and_bound():
    h = open(os.path.join(ROOT, "include", "nbody.h")).read()
    assert re.search(r"int nbody_set_bh_max_depth\(nbody_ctx \*ctx, int32_t levels\)", h)
    assert re.search(r"int nbody_get_bh_max_depth\(nbody_ctx \*ctx, int32_t \*levels\)", h)
    assert "nbody_actor_set_bh_max_depth" in open(os.path.join(ROOT, "include", "nbody_actor.h")).read()
    lib = open(os.path.join(ROOT, "parallelnbody_amd", "_lib.py")).read()
    for name in ("nbody_set_bh_max_depth", "nbody_get_bh_max_depth", "nbody_actor_set_bh_max_depth"):
        assert f'sig("{name}"' in lib
    from parallelnbody_amd.engine import NBodyEngine
    from parallelnbody_amd.actor import OctreeSearch
    assert callable(NBodyEngine.set_bh_max_depth) and callable(NBodyEngine.bh_max_depth)
    assert callable(OctreeSearch.set_bh_max_depth)
