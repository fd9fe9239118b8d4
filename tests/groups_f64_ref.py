"""numpy mirrors of the fp64 group census (include/nbody.h: nbody_get_radius_counts_f64, nbody_radius_counts_at_f64,
nbody_get_groups_f64), bit for bit: every float64 operation below is the one the header names, in its order, and numpy never contracts.

    d2 = (dx*dx + dy*dy) + dz*dz  with dx = x_j - x_i;   linked iff d2 <= radius * radius

Two independent routes to the labels:
  groups()        the definitions: the linked pairs, blockwise, then a union-find — nothing of the device's rounds in it
  rounds_scheme() the device's scheme itself on the same pairs — every body learns the smallest parent among its linked bodies, the ROOT
                  of its tree is hooked to it by min, every tree is flattened — which also returns its round count

The pairs come from blocks of rows against a WINDOW of columns in x order: a linked pair has dx*dx <= d2 <= r2 (adding non-negative terms
and rounding are monotone), so |dx| <= radius (1 + 2^-50) and a window that wide leaves no linked pair out; bodies whose x is not finite
link nothing and stay out of it.  pairs_full() is the same without the window, for the tests that hold the window to it.

The scenes of tests/test_groups_f64_gpu.py live here too, so that the device-free tests check the very same ones."""
import collections
import functools

import numpy as np

Summary = collections.namedtuple("Summary", ("groups", "multiples", "largest", "largest_members", "links"))

GAUSS_SIZES = (1, 2, 255, 256, 257, 1000, 4097, 32769)
POINT_COUNTS = (1, 300, 513)


def gauss_radii(n):
    """the linking lengths a Gaussian scene of n bodies is tested at"""
    if n in (1000, 4097):
        return (0.05, 0.2, 0.4)
    if n == 32769:
        return (0.1,)
    return (0.4, 10.0) if n <= 2 else (0.4,)      # 10: the two bodies of N = 2 are linked


def d2_block(rows, cols):
    """d2[a, b] between rows[a] and cols[b] ([., 3] float64 each): dx = cols - rows, (dx*dx + dy*dy) + dz*dz"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = cols[None, :, 0] - rows[:, None, 0]
        dy = cols[None, :, 1] - rows[:, None, 1]
        dz = cols[None, :, 2] - rows[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def r2_of(radius):
    r2 = np.float64(radius) * np.float64(radius)
    assert np.isfinite(radius) and radius >= 0.0 and np.isfinite(r2)
    return r2


def pairs_full(pos, radius, block=512):
    """(i, j), i < j, of every linked pair, lexicographic: all rows against all columns"""
    pos = np.ascontiguousarray(pos[:, :3], np.float64)
    r2, out = r2_of(radius), []
    for a in range(0, len(pos), block):
        with np.errstate(invalid="ignore"):
            hit = d2_block(pos[a:a + block], pos) <= r2
        i, j = np.nonzero(hit)
        i += a
        out.append(np.stack([i[i < j], j[i < j]], 1))
    p = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)


def pairs(pos, radius, block=256):
    """pairs_full()'s answer from blocks of rows in x order against the window of columns within radius (1 + 2^-50) in x"""
    pos = np.ascontiguousarray(pos[:, :3], np.float64)
    r2 = r2_of(radius)
    finite = np.flatnonzero(np.isfinite(pos[:, 0]))
    order = finite[np.argsort(pos[finite, 0], kind="stable")]
    xs, ps = pos[order, 0], pos[order]
    reach = np.float64(radius) * (1.0 + 2.0 ** -50) + np.finfo(np.float64).tiny
    out = []
    for a in range(0, len(order), block):
        b = min(a + block, len(order))
        lo = np.searchsorted(xs, xs[a] - reach, "left")
        hi = np.searchsorted(xs, xs[b - 1] + reach, "right")
        with np.errstate(invalid="ignore"):
            hit = d2_block(ps[a:b], ps[lo:hi]) <= r2
        i, j = np.nonzero(hit)
        i, j = order[i + a], order[j + lo]
        out.append(np.stack([i[i < j], j[i < j]], 1))
    p = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    p = p[np.lexsort((p[:, 1], p[:, 0]))]
    return p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)


def counts_at(points, pos, radius, block=512):
    """the bodies within radius of every point: NO body is dropped by index"""
    points = np.ascontiguousarray(np.asarray(points, np.float64)[:, :3])
    pos = np.ascontiguousarray(pos[:, :3], np.float64)
    r2, out = r2_of(radius), np.zeros(len(points), np.int32)
    for a in range(0, len(points), block):
        with np.errstate(invalid="ignore"):
            out[a:a + block] = (d2_block(points[a:a + block], pos) <= r2).sum(1)
    return out


def union_find(n, i, j):
    """label[n]: the lowest index of every body's component under the links (i, j) — a union-find, the lower root wins"""
    parent = list(range(n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r
    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    return np.array([find(a) for a in range(n)], np.int32)


def rounds_scheme(n, i, j):
    """(label, rounds): the device's rounds on the links (i, j).  Per round: mn[a] = min(parent[a], parent[b] over a's linked b); a copy of
    parent is lowered at parent[a] to mn[a] where mn[a] < parent[a] (min: any order); every body's new parent is the fixed point of that
    copy.  The first round that changes nothing is the last, and is counted."""
    parent = np.arange(n, dtype=np.int64)
    both_a, both_b = np.concatenate([i, j]), np.concatenate([j, i])
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= n
        mn = parent.copy()
        np.minimum.at(mn, both_a, parent[both_b])
        hooked = parent.copy()
        low = mn < parent
        np.minimum.at(hooked, parent[low], mn[low])
        while True:                                                 # the chase of every body at once: hooked never ascends
            up = hooked[hooked]
            if (up == hooked).all():
                break
            hooked = up
        if (hooked == parent).all():
            return parent.astype(np.int32), rounds
        parent = hooked


def summarise(label, degree):
    n = len(label)
    members = np.bincount(label, minlength=n)[label].astype(np.int32)
    roots = np.flatnonzero(label == np.arange(n))
    size = members[roots]
    largest = int(roots[np.argmax(size)])                           # argmax: the first — the lowest label — among ties
    s = Summary(groups=len(roots), multiples=int((size >= 2).sum()), largest=largest, largest_members=int(size.max()),
                links=int(degree.astype(np.int64).sum()) // 2)
    return members, s


def groups(pos, radius):
    """dict(label, members, degree: int32[n]; summary; i, j: the links) by the definitions"""
    n = len(pos)
    i, j = pairs(pos, radius)
    degree = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n)).astype(np.int32)
    label = union_find(n, i, j)
    members, s = summarise(label, degree)
    return dict(label=label, members=members, degree=degree, summary=s, i=i, j=j)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------

def gauss_scene(n):
    rng = np.random.default_rng(n)
    posm = np.empty((n, 4))
    posm[:, :3] = rng.normal(0.0, 1.0, (n, 3))
    posm[:, 3] = rng.uniform(0.5, 1.5, n) / n
    return posm


def bit_reverse(bits):
    k = np.arange(1 << bits)
    out = np.zeros_like(k)
    for b in range(bits):
        out |= ((k >> b) & 1) << (bits - 1 - b)
    return out


def chain_scene(kind, n=4096):
    """n bodies at integer x = 0 .. n - 1, body k at x = order[k]: `permuted` (default_rng(1).permutation) or `bitrev`"""
    order = np.random.default_rng(1).permutation(n) if kind == "permuted" else bit_reverse(n.bit_length() - 1)
    posm = np.zeros((n, 4))
    posm[:, 0] = order
    posm[:, 3] = 1.0 / n
    return posm


def lattice_scene(side=9):
    g = np.arange(side, dtype=np.float64)
    posm = np.zeros((side ** 3, 4))
    posm[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    posm[:, 3] = 1.0
    return posm


def coincident_scene(n=300):
    posm = np.zeros((n, 4))
    posm[:, :3] = (0.25, -1.5, 3.0)
    posm[:, 3] = 1.0 / n
    return posm


def nonfinite_scene():
    """gauss_scene(300) with a NaN in x, y and z of three bodies and +inf / -inf in three more (the chunk's second tile among them)"""
    posm = gauss_scene(300)
    posm[5, 0] = np.nan; posm[17, 1] = np.nan; posm[280, 2] = np.nan
    posm[40, 0] = np.inf; posm[41, 1] = -np.inf; posm[299, 2] = np.inf
    return posm
NONFINITE_BODIES = (5, 17, 280, 40, 41, 299)


def interleaved_scene(n=600):
    """two Gaussian clusters of scale 0.05, 100 apart: the even bodies in one, the odd ones in the other"""
    rng = np.random.default_rng(7)
    posm = np.zeros((n, 4))
    posm[:, :3] = rng.normal(0.0, 0.05, (n, 3))
    posm[1::2, 0] += 100.0
    posm[:, 3] = 1.0 / n
    return posm


STRUCTURAL = {                                                      # name: (scene, radii)
    "chain_permuted": (lambda: chain_scene("permuted"), (1.5,)),
    "chain_bitrev": (lambda: chain_scene("bitrev"), (1.5,)),
    "lattice": (lattice_scene, (1.0, 0.99)),
    "coincident": (coincident_scene, (0.0,)),
    "nonfinite": (nonfinite_scene, (0.4,)),
    "interleaved": (interleaved_scene, (1.0,)),
}


def cases():
    """(name, radius) of every scene the GPU tests use"""
    out = [(f"gauss{n}", r) for n in GAUSS_SIZES for r in gauss_radii(n)]
    return out + [(name, r) for name, (_, radii) in STRUCTURAL.items() for r in radii]


@functools.lru_cache(maxsize=None)
def scene(name):
    posm = gauss_scene(int(name[5:])) if name.startswith("gauss") else STRUCTURAL[name][0]()
    posm.setflags(write=False)
    return posm


@functools.lru_cache(maxsize=None)
def case(name, radius):
    """groups() of a scene, computed once and shared"""
    g = groups(scene(name), radius)
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g
