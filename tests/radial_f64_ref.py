"""The yardsticks of the fp64 radial census — nbody_radial_order_f64, nbody_lagrange_radii_f64: the definitions of include/nbody.h in
plain numpy, in float64 (every line a bit-for-bit mirror of the device) and in np.longdouble, and the GAP of every selection.

    d2        dx = x - centre[0] (dy, dz alike); d2 = (dx*dx + dy*dy) + dz*dz — numpy never contracts
    order     np.argsort(key, kind="stable") of key = ~0 for a NaN, else the bit pattern of d2: ascending (d2, index), finite d2 first,
              then +inf, then NaN
    mass_cum  blocks of 256 positions, left to right inside a block (np.cumsum along the rows IS the sequential sum), then the blocks'
              offsets in order: off[0] = 0.0, off[b + 1] = off[b] + loc[b][255]
    select    target = f * total; the first position with mass_cum >= target; none unless total > 0
    gap       of a selection at p: min(|cum_ld[p] - target_ld|, |cum_ld[p - 1] - target_ld|) / total_ld (cum_ld[-1] = 0) — how far the
              target is from the nearest cumulative mass that could change the answer.  Any order of fp64 additions leaves mass_cum
              within n 2^-53 sum|m| of the exact sum, and the target within 2^-53 of its own, so where gap >= GAP_FACTOR n 2^-53 the
              fp64 selection IS the long-double one and a body index can be compared."""
import functools

import numpy as np

LD = np.longdouble
BLOCK = 256
FRACTIONS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9)       # NBodyEngine.lagrange_f64's default
SIZES = (1, 2, 255, 256, 257, 4095, 4096, 4097, 32769, 300001)     # the scan block's and the radix tile's boundaries, 9 and 74 tiles
GAP_FACTOR = 4.0
ROW = np.dtype([("fraction", "<f8"), ("r2", "<f8"), ("radius", "<f8"), ("mass", "<f8"), ("body", "<i4"), ("count", "<i4")])
assert ROW.itemsize == 40


def gauss_scene(n, seed=None):
    """(posm, vel) [n, 4] float64: a Gaussian ball, masses that all differ — uniform(0.5, 1.5) / n —, so that no cumulative mass is a
    round fraction of the total"""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    posm, vel = np.zeros((n, 4)), np.zeros((n, 4))
    posm[:, :3] = rng.normal(0.0, 1.0, (n, 3)); posm[:, 3] = rng.uniform(0.5, 1.5, n) / n
    vel[:, :3] = rng.normal(0.0, 0.3, (n, 3))
    return posm, vel


CENTRE = np.array([0.03125, -0.0625, 0.015625])                    # where the Gaussian scenes are looked at from


def d2_of(pos, centre, dtype=np.float64):
    pos, c = np.asarray(pos, dtype), np.asarray(centre, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = pos[:, 0] - c[0], pos[:, 1] - c[1], pos[:, 2] - c[2]
        return (dx * dx + dy * dy) + dz * dz


def order_of(d2):
    """(order int32, n_finite): the device's keys, sorted stably"""
    d2 = np.ascontiguousarray(d2, np.float64)
    key = np.where(np.isnan(d2), np.uint64(0xFFFFFFFFFFFFFFFF), d2.view(np.uint64))
    return np.argsort(key, kind="stable").astype(np.int32), int(np.isfinite(d2).sum())


def scan(w):
    """mass_cum of the weights w in sorted order: the blocked sum of include/nbody.h"""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    pad = np.zeros(-(-n // BLOCK) * BLOCK)
    pad[:n] = w
    loc = np.cumsum(pad.reshape(-1, BLOCK), axis=1)
    off = np.cumsum(np.concatenate(([0.0], loc[:-1, -1])))         # 0.0, 0.0 + loc[0][255], ...
    return (off[:, None] + loc).reshape(-1)[:n]


def radial(posm, centre):
    """(order, d2 sorted, mass_cum, n_finite, w): nbody_radial_order_f64 in numpy; w = the weights in sorted order"""
    d2 = d2_of(posm[:, :3], centre)
    order, n_finite = order_of(d2)
    d2s = d2[order]
    w = np.where(np.isfinite(d2s), posm[order, 3], 0.0)
    return order, d2s, scan(w), n_finite, w


def select(order, d2s, cum, fractions):
    """(rows [k] of ROW, total): nbody_lagrange_radii_f64's selection on a given mass_cum"""
    total = cum[-1]
    rows = np.zeros(len(fractions), ROW)
    for q, f in enumerate(fractions):
        hits = np.flatnonzero(cum >= np.float64(f) * total) if total > 0.0 else np.zeros(0, np.int64)
        if hits.size:
            p = int(hits[0])
            rows[q] = (f, d2s[p], np.sqrt(d2s[p]), cum[p], order[p], p + 1)
        else:
            rows[q] = (f, np.nan, np.nan, np.nan, -1, 0)
    return rows, total


def select_ld(w, fractions):
    """(p [k], gap [k], cum_ld): the selection on the long-double running sum of the weights (no blocks: the exact sum has none),
    p = -1 where nothing qualifies, and its gap"""
    cum = np.cumsum(np.asarray(w, LD))
    total = cum[-1]
    ps, gaps = [], []
    for f in fractions:
        target = LD(np.float64(f)) * total
        hits = np.flatnonzero(cum >= target) if total > 0 else np.zeros(0, np.int64)
        if not hits.size:
            ps.append(-1); gaps.append(np.inf)
            continue
        p = int(hits[0])
        below = cum[p - 1] if p > 0 else LD(0)
        ps.append(p); gaps.append(float(min(abs(cum[p] - target), abs(below - target)) / total))
    return np.array(ps), np.array(gaps), cum


def gap_bound(n):
    return GAP_FACTOR * n * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def gauss_case(n):
    """The Gaussian scene of n bodies and its answers, computed once: a dict of posm, vel, order, d2, cum, n_finite, w, rows, total,
    p_ld, gap (read-only arrays)"""
    posm, vel = gauss_scene(n)
    order, d2s, cum, n_finite, w = radial(posm, CENTRE)
    rows, total = select(order, d2s, cum, FRACTIONS)
    p_ld, gap, _ = select_ld(w, FRACTIONS)
    out = dict(posm=posm, vel=vel, order=order, d2=d2s, cum=cum, n_finite=n_finite, w=w, rows=rows, total=total, p_ld=p_ld, gap=gap)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def wide_scene(n=6000):
    """Distances from 0 through subnormal d2 to 1e300: every one of the key's eight digits takes many values.  Body 0 sits on the
    centre (the origin), the rest on random directions at radii 10^u, u uniform in -170 .. 150 (d2 from subnormal to 1e300)."""
    rng = np.random.default_rng(77)
    posm = np.zeros((n, 4))
    u = rng.normal(0.0, 1.0, (n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = 10.0 ** rng.uniform(-170.0, 150.0, n)
    r[1:40] = 10.0 ** rng.uniform(-161.5, -154.0, 39)              # d2 among the subnormals
    posm[:, :3] = u * r[:, None]
    posm[0, :3] = 0.0
    posm[:, 3] = rng.uniform(0.5, 1.5, n) / n
    return posm


def lattice_scene(side=21):
    """A cubic lattice of side^3 points with integer coordinates, centred on a lattice point: thousands of exactly equal d2, across
    the radix tiles (21^3 = 9261 bodies: three tiles).  Masses all differ."""
    g = np.arange(side, dtype=np.float64) - side // 2
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    n = side ** 3
    posm = np.zeros((n, 4))
    posm[:, 0], posm[:, 1], posm[:, 2] = x.ravel(), y.ravel(), z.ravel()
    posm[:, 3] = np.random.default_rng(5).uniform(0.5, 1.5, n) / n
    return posm


def dyadic_scene(n=1024):
    """n = 1024 bodies of mass 2^-10 on distinct radii: every partial sum is exact, so f = 0.5 must select position 511 by >= alone"""
    rng = np.random.default_rng(9)
    posm = np.zeros((n, 4))
    u = rng.normal(0.0, 1.0, (n, 3))
    posm[:, :3] = u / np.linalg.norm(u, axis=1)[:, None] * rng.permutation(np.arange(1, n + 1) / n)[:, None]
    posm[:, 3] = 2.0 ** -10
    return posm


def plummer_half_mass(n=20000, a=1.0, seed=3):
    """(posm, a): a Plummer sphere of scale a by inversion of M(<r) = r^3 / (r^2 + a^2)^(3/2); its half-mass radius is
    a / sqrt(2^(2/3) - 1) = 1.3048 a"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, n)
    r = a / np.sqrt(x ** (-2.0 / 3.0) - 1.0)
    u = rng.normal(0.0, 1.0, (n, 3))
    posm = np.zeros((n, 4))
    posm[:, :3] = u / np.linalg.norm(u, axis=1)[:, None] * r[:, None]
    posm[:, 3] = rng.uniform(0.5, 1.5, n) / n
    return posm, a
