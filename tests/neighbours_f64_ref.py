"""The yardsticks of the fp64 neighbour census — nbody_get_neighbours_f64, nbody_neighbours_at_f64, nbody_get_density_f64,
nbody_density_centre_f64: the definitions of include/nbody.h in plain numpy, in float64 or np.longdouble, and the GAP of every row.
TEST INFRASTRUCTURE ONLY.

A row's list: the k bodies (not the row's own, when the row is a body) with the smallest d2 = |x_j - x|^2, never softened, in STABLE
lexicographic (d2, index) order — the lowest index among equals; a d2 that is NaN or +inf is never listed; empty slots read -1, +inf.
Density (2 <= k): rho = msum / ((4 pi / 3) (r2 sqrt(r2))), msum the masses of the k - 1 nearest added in neighbour order, r2 = d2_k;
0 where the k-th is missing or the quotient is NaN.  Density centre: with w = rho where 0 < rho < +inf, else 0:
    centre = sum w x / sum w;   core_radius = sqrt(sum w^2 |x - centre|^2 / sum w^2)

A sorted list is only as sure as the distances between its entries, so every row carries its gap:
    min over q = 1 .. k of (d2_(q+1) - d2_q) / d2_(q+1)
— the runner-up behind the list included (q = k); a missing d2_(q+1) counts 1, an exact tie 0.  The device tests hold indices to this
reference only where the gap is far above the arithmetic's error (1e-9 against 1e-12) and fail on a scene that has a row below it."""
import numpy as np

import census_f64_ref as C

GAP_MIN = C.GAP_MIN                                                # 1e-9: 1000 x the project's fp64 parity bound
CASES = C.CASES                                                    # (N, M) of pot_tidal_f64_ref.plummer_scene
N_CHUNKS, ROWS_CHUNKS, N_SLAB = C.N_CHUNKS, C.ROWS_CHUNKS, C.N_SLAB
K_MAX = 8
LD = np.longdouble


def neighbours(pos, pts=None, rows=None, k=K_MAX, dtype=np.float64):
    """(index [m, k] int32, d2 [m, k] dtype, gap [m] dtype).  pts None: the rows are the bodies `rows` (None: all), each leaves itself
    out by index; else the rows are the points `pts` and nothing is dropped by index."""
    pos = np.asarray(pos, dtype)[:, :3]
    n = pos.shape[0]
    if pts is None:
        own = np.arange(n) if rows is None else np.asarray(rows)
        x = pos[own]
    else:
        own = None
        x = np.asarray(pts, dtype)[:, :3]
    m = x.shape[0]
    inf, one, zero = dtype(np.inf), dtype(1), dtype(0)
    index = np.full((m, k), -1, np.int32); d2o = np.full((m, k), inf, dtype); gap = np.empty(m, dtype)
    blk = max(1, min(1024, 1_000_000 // max(1, n)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(0, m, blk):
            b = min(a + blk, m)
            r = np.arange(b - a)
            d = pos[None, :, :] - x[a:b, None, :]
            d2 = (d * d).sum(-1)
            val = np.where(np.isfinite(d2), d2, inf)
            if own is not None:
                val[r, own[a:b]] = inf
            if n > 2048:                                           # the large scenes, for speed: the k + 1 smallest first.  A tie ACROSS that
                                                                   # cut shows as a gap of 0; scenes with exact ties are small and sort in full
                few = np.sort(np.argpartition(val, k, axis=1)[:, :k + 1], axis=1)
            else:
                few = np.broadcast_to(np.arange(n), (b - a, n))
            fv = np.take_along_axis(val, few, 1)
            order = np.argsort(fv, axis=1, kind="stable")          # columns ascend in index: stable = the lowest index among equals
            si, sv = np.take_along_axis(few, order, 1), np.take_along_axis(fv, order, 1)
            pad = k + 1 - sv.shape[1]
            if pad > 0:
                si = np.concatenate([si, np.full((b - a, pad), -1)], 1); sv = np.concatenate([sv, np.full((b - a, pad), inf, dtype)], 1)
            si = np.where(sv < inf, si, -1)
            index[a:b], d2o[a:b] = si[:, :k], sv[:, :k]
            lo, hi = sv[:, :k], sv[:, 1:k + 1]
            g = np.where(hi < inf, np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, one), zero), one)
            gap[a:b] = g.min(1)
    return index, d2o, gap


def density(index, d2, mass, k, dtype=np.float64):
    """(rho, rk2) from lists of at least k columns and the raw masses: the formula of include/nbody.h, operation by operation in `dtype`
    — in float64 every operation is the device's."""
    index = np.asarray(index); d2 = np.asarray(d2, dtype); mass = np.asarray(mass, dtype)
    have = index[:, k - 1] >= 0
    safe = np.where(index[:, :k - 1] >= 0, index[:, :k - 1], 0)
    msum = mass[safe[:, 0]].copy()
    for q in range(1, k - 1):
        msum = msum + mass[safe[:, q]]
    r2 = d2[:, k - 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        vol = (dtype(4.0) * dtype(np.pi) / dtype(3.0)) * (r2 * np.sqrt(r2))
        rho = msum / vol
    rho = np.where(have & ~np.isnan(rho), rho, dtype(0))
    return rho, r2


def core(rho, pos):
    """The two reduction passes in long double from the given densities: a dict of centre [3], core_radius, rho_sum, rho2_sum, used,
    rho_max, densest, and the sums of |terms| the device's fixed-order fp64 sums are held against: abs_s [3] (sum w |x|), abs_q (sum
    w^2 |x - centre|^2, itself: a sum of non-negative terms)."""
    rho = np.asarray(rho, LD); x = np.asarray(pos, LD)[:, :3]
    w = np.where((rho > 0) & (rho < np.inf), rho, LD(0))
    used = int((w > 0).sum())
    if used == 0:
        return {"used": 0, "centre": np.full(3, np.nan), "core_radius": np.nan, "rho_sum": LD(0), "rho2_sum": LD(0), "rho_max": 0.0,
                "densest": -1}
    s0 = w.sum()
    s = (w[:, None] * x).sum(0)
    centre = s / s0
    d = x - centre
    q0 = (w * w).sum()
    q2 = (w * w * (d * d).sum(1)).sum()
    return {"used": used, "centre": centre, "core_radius": np.sqrt(q2 / q0), "rho_sum": s0, "rho2_sum": q0, "rho_max": float(w.max()),
            "densest": int(np.argmax(w)), "abs_s": (w[:, None] * np.abs(x)).sum(0), "q2": q2}


# ---- the scenes of tests/test_neighbours_f64_gpu.py and their long-double answers, computed once and shared, read-only ----
_cache = {}


def slab_points(nb):
    """(pts, sampled): probe_slab_points(N_SLAB, 8) + 1000 points in the N_SLAB scene, and the 32 of them held to long double."""
    if "slab" not in _cache:
        posm, _, _, _ = C.scene(nb, N_SLAB)
        m = C.probe_slab_points(N_SLAB, K_MAX) + 1000
        rng = np.random.default_rng(34)
        pts = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
        sampled = np.sort(rng.permutation(m)[:32])
        pts.setflags(write=False); sampled.setflags(write=False)
        _cache["slab"] = (pts, sampled)
    return _cache["slab"]


def reference(nb, kind, n=0, m=0, dtype=LD):
    """(index, d2, gap) for k = 8 in `dtype`, computed once: kind "bodies" (every body of scene(n, m)), "points" (its points), "chunks"
    (the bodies ROWS_CHUNKS of scene(N_CHUNKS)), "slab" (the sampled points of slab_points)."""
    key = (kind, n, m, dtype)
    if key not in _cache:
        if kind == "slab":
            pts, sampled = slab_points(nb)
            got = neighbours(C.scene(nb, N_SLAB)[0], pts[sampled], dtype=dtype)
        elif kind == "chunks":
            got = neighbours(C.scene(nb, N_CHUNKS)[0], rows=ROWS_CHUNKS, dtype=dtype)
        else:
            posm, _, tpos, _ = C.scene(nb, n, m)
            got = neighbours(posm, dtype=dtype) if kind == "bodies" else neighbours(posm, tpos, dtype=dtype)
        for a in got:
            a.setflags(write=False)
        _cache[key] = got
    return _cache[key]


def gaps_hold(ref):
    """The gap condition on one (index, d2, gap): every row's every entry is more than GAP_MIN from the next.  Returns the smallest gap."""
    g = float(ref[2].min())
    assert g > GAP_MIN, f"a row of this scene is too close to a tie: smallest gap {g:.3e}"
    return g


CLUMP_SIGMA = 1e-2                                                 # of the scene's scale: 40 bodies there are ~1e4 times the mean density


def clump_scene(nb, n=1000):
    """(posm, vel, members, scale): the N = 1000 Plummer scene with its last 40 bodies gathered into a tight clump (a Gaussian of
    CLUMP_SIGMA x scale) well away from the centre of mass — the density centre belongs there, the centre of mass does not."""
    if "clump" not in _cache:
        posm, vel, _, _ = C.scene(nb, n, 25)
        posm, vel = posm.copy(), vel.copy()
        scale = float(np.abs(posm[:, :3]).std())
        members = np.arange(n - 40, n)
        rng = np.random.default_rng(40)
        posm[members, :3] = np.array([3.0, -2.0, 1.5]) * scale + rng.normal(0.0, CLUMP_SIGMA * scale, (40, 3))
        posm.setflags(write=False); vel.setflags(write=False)
        _cache["clump"] = (posm, vel, members, scale)
    return _cache["clump"]
