"""numpy mirrors of the fp64 minimum spanning tree (include/nbody.h: nbody_get_mst_f64), bit for bit: every float64 operation below is
the one the header names, in its order, and numpy never contracts.

    d2 = (dx*dx + dy*dy) + dz*dz  with dx = x_j - x_i;   an edge iff d2 is finite;   edges compare by the key (d2, i, j), i < j

Two independent routes to the forest:
  prim()          the definition: Prim's algorithm under the key, restarted at the lowest body left for every component — nothing of the
                  device's rounds in it
  rounds_scheme() the device's Boruvka rounds themselves — every body's nearest body under another label (the first minimum in ascending
                  j), per label the smallest d2 by its bit pattern and then the smallest packed pair, the hook with its rule for two
                  labels that chose the same edge, the chase to the roots — which also returns the passes it takes

The scenes are those of tests/groups_f64_ref.py, so that cutting a tree can be held to that file's groups."""
import collections
import functools

import numpy as np

import groups_f64_ref as R

Summary = collections.namedtuple("Summary", ("edges", "components", "length", "longest_d2"))

GAUSS_SIZES = (1, 2, 3, 255, 256, 257, 513, 1000, 4097)
STRUCTURAL = ("lattice", "coincident", "chain_permuted", "chain_bitrev", "nonfinite", "interleaved")
NONE = np.uint64(0xffffffffffffffff)

# name: (edges, components, passes, edges that share their d2 with the edge before them) — include/nbody.h's early stop included
EXPECTED = {"gauss1": (0, 1, 0, 0), "gauss2": (1, 1, 1, 0), "gauss3": (2, 1, 1, 0), "gauss255": (254, 1, 4, 0), "gauss256": (255, 1, 4, 0),
            "gauss257": (256, 1, 4, 0), "gauss513": (512, 1, 5, 0), "gauss1000": (999, 1, 4, 0), "gauss4097": (4096, 1, 5, 0),
            "chain_permuted": (4095, 1, 7, 4094), "chain_bitrev": (4095, 1, 11, 4094), "lattice": (728, 1, 1, 727),
            "coincident": (299, 1, 1, 298), "nonfinite": (293, 7, 5, 0), "interleaved": (599, 1, 5, 0)}


def names():
    return tuple(f"gauss{n}" for n in GAUSS_SIZES) + STRUCTURAL


def radii(name):
    """the linking lengths tests/groups_f64_ref.py holds the scene's groups at"""
    return R.gauss_radii(int(name[5:])) if name.startswith("gauss") else R.STRUCTURAL[name][1]


def round_bound(n):
    """ceil(log2 n) + 1"""
    return (n - 1).bit_length() + 1


def positions(posm):
    return np.ascontiguousarray(np.asarray(posm)[:, :3], np.float64)


def finish(n, d2, lo, hi):
    """the edges in key order and what follows from them"""
    d2, lo, hi = np.asarray(d2, np.float64), np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    assert (lo < hi).all() and np.isfinite(d2).all()
    order = np.lexsort((hi, lo, d2))
    d2, lo, hi = d2[order], lo[order], hi[order]
    component = R.union_find(n, lo, hi)
    length = float(np.cumsum(np.sqrt(d2))[-1]) if len(d2) else 0.0
    s = Summary(edges=len(d2), components=n - len(d2), length=length, longest_d2=float(d2[-1]) if len(d2) else 0.0)
    return dict(i=lo.astype(np.int32), j=hi.astype(np.int32), d2=d2, component=component, summary=s)


def prim(posm):
    """dict(i, j: int32, d2: float64 — the edges in key order; component: int32[n]; summary) by the definition"""
    pos = positions(posm)
    n = len(pos)
    idx = np.arange(n)
    dist = np.full(n, np.inf)                                       # per body outside the tree: the smallest key of an edge into it
    frm = np.full(n, -1, np.int64)
    outside = np.ones(n, bool)
    d2s, los, his = [], [], []

    def add(v):
        outside[v] = False
        d = R.d2_block(pos[v:v + 1], pos)[0]
        d = np.where(np.isfinite(d), d, np.inf)
        lo_new, hi_new = np.minimum(idx, v), np.maximum(idx, v)
        lo_old, hi_old = np.minimum(idx, frm), np.maximum(idx, frm)
        tie = (d == dist) & (d < np.inf) & ((lo_new < lo_old) | ((lo_new == lo_old) & (hi_new < hi_old)))
        better = outside & ((d < dist) | tie)
        dist[better] = d[better]
        frm[better] = v

    while outside.any():
        m = np.where(outside, dist, np.inf).min()
        if not m < np.inf:                                          # no edge leaves the tree: the next component starts
            add(int(np.flatnonzero(outside)[0]))
            continue
        tie = np.flatnonzero(outside & (dist == m))
        lo, hi = np.minimum(tie, frm[tie]), np.maximum(tie, frm[tie])
        k = np.lexsort((hi, lo))[0]
        d2s.append(m); los.append(int(lo[k])); his.append(int(hi[k]))
        add(int(tie[k]))
    return finish(n, d2s, los, his)


def nearest_foreign(pos, label, block=512):
    """(index, d2) per body: the body under another label with the smallest finite d2, the lowest index among ties; none: (-1, +inf)"""
    n = len(pos)
    near_j, near_d2 = np.full(n, -1, np.int64), np.full(n, np.inf)
    for a in range(0, n, block):
        d = R.d2_block(pos[a:a + block], pos)
        d[~np.isfinite(d)] = np.inf
        d[label[a:a + block, None] == label[None, :]] = np.inf
        j = d.argmin(1)                                             # the first minimum: ascending j under strict <
        v = d[np.arange(len(j)), j]
        near_j[a:a + block] = np.where(v < np.inf, j, -1)
        near_d2[a:a + block] = v
    return near_j, near_d2


def rounds_scheme(posm):
    """prim()'s dict by the device's rounds, and `passes`: the all-pairs passes taken"""
    pos = positions(posm)
    n = len(pos)
    idx = np.arange(n)
    label = idx.copy()
    d2s, los, his = [], [], []
    passes, edges = 0, 0
    while edges + 1 < n:
        assert passes < round_bound(n)
        near_j, near_d2 = nearest_foreign(pos, label)
        passes += 1
        has = near_j >= 0
        bits = near_d2.view(np.uint64)
        best = np.full(n, NONE)
        np.minimum.at(best, label[has], bits[has])
        attains = has & (bits == best[label])
        lo, hi = np.minimum(idx, near_j), np.maximum(idx, near_j)
        pair = np.full(n, NONE)
        np.minimum.at(pair, label[attains], (lo[attains].astype(np.uint64) << np.uint64(32)) | hi[attains].astype(np.uint64))
        roots = np.flatnonzero((label == idx) & (pair != NONE))
        if len(roots) == 0:
            break
        p = pair[roots]
        plo, phi = (p >> np.uint64(32)).astype(np.int64), (p & np.uint64(0xffffffff)).astype(np.int64)
        other = np.where(label[plo] == roots, label[phi], label[plo])
        both = pair[other] == p                                     # two labels chose the same edge
        succ = idx.copy()
        succ[roots] = np.where(both & (roots < other), roots, other)
        appended = ~(both & (roots > other))
        d2s += best[roots[appended]].view(np.float64).tolist(); los += plo[appended].tolist(); his += phi[appended].tolist()
        edges = len(d2s)
        r = label
        for _ in range(n):                                          # the chase of every body at once
            up = succ[r]
            if (up == r).all():
                break
            r = up
        label = r
    out = finish(n, d2s, los, his)
    lowest = idx.copy()
    np.minimum.at(lowest, label, idx)
    assert out["component"].tobytes() == lowest[label].astype(np.int32).tobytes()
    out["passes"] = passes
    return out


def cut(tree, n, radius):
    """label[n] of the groups at linking length `radius` from a tree's edges: a union-find over those with d2 <= radius * radius"""
    keep = tree["d2"] <= R.r2_of(radius)
    return R.union_find(n, tree["i"][keep].astype(np.int64), tree["j"][keep].astype(np.int64))


def d2_of(posm, i, j):
    """the d2 of the pairs (i, j), the header's expression"""
    pos = positions(posm)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (pos[j, k] - pos[i, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def chain_tree(n):
    """(posm, tree) of R.chain_scene("permuted", n): the tree is the n - 1 edges between consecutive integers, d2 = 1.0 each, known
    without a search — built from the inverse permutation"""
    posm = R.chain_scene("permuted", n)
    inverse = np.empty(n, np.int64)
    inverse[posm[:, 0].astype(np.int64)] = np.arange(n)
    a, b = inverse[:-1], inverse[1:]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo))
    s = Summary(edges=n - 1, components=1, length=float(n - 1), longest_d2=1.0)
    return posm, dict(i=lo[order].astype(np.int32), j=hi[order].astype(np.int32), d2=np.ones(n - 1), component=np.zeros(n, np.int32), summary=s)


@functools.lru_cache(maxsize=None)
def case(name):
    """prim() of a scene, computed once and shared"""
    t = prim(R.scene(name))
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t
