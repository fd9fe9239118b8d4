"""numpy mirror of the fp64 separation census (include/nbody.h: nbody_get_pair_counts_f64, nbody_pair_counts_at_f64), written from the
header's text: every float64 operation below is the one the header names, in its order, and numpy never contracts.

    d2 = (dx*dx + dy*dy) + dz*dz  with dx = x_j - x_i;   r2 = radius * radius;   a pair counts iff d2 <= r2

    pair_counts(posm, radii)           the UNORDERED pairs {i, j}, i != j by index, per radius
    pair_counts_at(points, posm, radii)   the (point, body) pairs per radius: NO body is dropped by index

The radii come in any order and with repeats and each is answered on its own.  d2 is formed blockwise (groups_f64_ref.d2_block) ONCE
per block and compared with every threshold; the answers are exact integers, so the tests hold the device to equality."""
import numpy as np

import groups_f64_ref as R

G = 16          # NBODY_PAIR_RADII_PER_PASS: the distinct radii one N^2 pass answers
K_MAX = 64      # NBODY_PAIR_RADII_MAX


def r2_of(radii):
    r = np.asarray(radii, np.float64).reshape(-1)
    r2 = r * r
    assert np.isfinite(r).all() and (r >= 0.0).all() and np.isfinite(r2).all()
    return r2


def _count(rows, cols, radii, skip_diagonal, block=256):
    """per radius the (row, col) pairs with d2 <= r2; skip_diagonal: rows is cols, the pairs (i, i) are left out BY INDEX.  Blocks of
    rows in x order against the window of columns within the largest radius in x, as groups_f64_ref.pairs: a counted pair has
    dx*dx <= d2 <= r2, and a row or column whose x is not finite has no finite d2."""
    r2 = r2_of(radii)
    out = np.zeros(len(r2), np.int64)
    by_r2 = np.argsort(r2, kind="stable")
    reach = np.float64(np.max(radii)) * (1.0 + 2.0 ** -50) + np.finfo(np.float64).tiny
    ri = np.flatnonzero(np.isfinite(rows[:, 0])); ri = ri[np.argsort(rows[ri, 0], kind="stable")]
    ci = np.flatnonzero(np.isfinite(cols[:, 0])); ci = ci[np.argsort(cols[ci, 0], kind="stable")]
    rs, cs, xs = rows[ri], cols[ci], cols[ci, 0]
    for a in range(0, len(ri), block):
        b = min(a + block, len(ri))
        lo, hi = np.searchsorted(xs, rs[a, 0] - reach, "left"), np.searchsorted(xs, rs[b - 1, 0] + reach, "right")
        d2 = R.d2_block(rs[a:b], cs[lo:hi])
        if skip_diagonal:
            d2[ri[a:b, None] == ci[None, lo:hi]] = np.nan          # (a NaN never counts)
        d2 = d2.reshape(-1)
        with np.errstate(invalid="ignore"):
            d2 = np.sort(d2[d2 <= r2[by_r2[-1]]])                   # NaN fails <=; what passes no threshold is dropped here
        out[by_r2] += np.searchsorted(d2, r2[by_r2], "right")       # the entries <= r2, each threshold on its own
    return out


def pairs_plain(posm, radii):
    """pair_counts() by a plain Python double loop over i < j (small N): float64 scalars, the header's expression"""
    pos = np.asarray(posm, np.float64)[:, :3]
    r2 = r2_of(radii)
    out = [0] * len(r2)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(pos)):
            for j in range(i + 1, len(pos)):
                dx, dy, dz = pos[j, 0] - pos[i, 0], pos[j, 1] - pos[i, 1], pos[j, 2] - pos[i, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                for q in range(len(r2)):
                    out[q] += bool(d2 <= r2[q])
    return np.array(out, np.int64)


def at_plain(points, posm, radii):
    """pair_counts_at() by a plain Python double loop (small sizes)"""
    pts, pos = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(posm, np.float64)[:, :3]
    r2 = r2_of(radii)
    out = [0] * len(r2)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in pts:
            for x in pos:
                dx, dy, dz = x[0] - p[0], x[1] - p[1], x[2] - p[2]
                d2 = (dx * dx + dy * dy) + dz * dz
                for q in range(len(r2)):
                    out[q] += bool(d2 <= r2[q])
    return np.array(out, np.int64)


def pair_counts(posm, radii):
    """int64[k]: the unordered pairs {i, j}, i != j by index, with d2 <= radii[q]^2 — half the ordered count (d2 is symmetric)"""
    pos = np.ascontiguousarray(np.asarray(posm, np.float64)[:, :3])
    ordered = _count(pos, pos, np.asarray(radii, np.float64).reshape(-1), True)
    assert (ordered % 2 == 0).all()
    return ordered // 2


def pair_counts_at(points, posm, radii):
    """int64[k]: the (point, body) pairs with d2 <= radii[q]^2 — a point on a body counts that body; no points: zeros"""
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    pos = np.ascontiguousarray(np.asarray(posm, np.float64)[:, :3])
    return _count(pts, pos, np.asarray(radii, np.float64).reshape(-1), False)


def radii_set(k, lo, hi, seed=0):
    """k distinct radii between lo and hi, log-spaced, in a shuffled order"""
    r = np.geomspace(lo, hi, k) if k > 1 else np.array([hi], np.float64)
    return np.random.default_rng(seed + k).permutation(r)
