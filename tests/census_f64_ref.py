"""The yardsticks of the fp64 pair census — nbody_get_nearest_f64, nbody_nearest_at_f64, nbody_closest_pair_f64,
nbody_get_partners_f64, nbody_partner_at_f64, nbody_hardest_pair_f64, nbody_pair_time_f64: the definitions of include/nbody.h in plain
numpy, in float64 or np.longdouble, with the lowest-index tie rule, and the GAP of every answer to its runner-up.  TEST INFRASTRUCTURE
ONLY.

For a row at (x, v) with mass term g (a body: g = G m_i; a point: g = 0) and body j, d = x_j - x, w = v_j - v:
    d2 = |d|^2 (never softened);  s2 = d2 + eps^2;  t = (s2 > 0 and j is not the row's own body) ? 1 / sqrt(s2) : 0
    e  = 0.5 |w|^2 - (G m_j + g) t
Nearest: the other body with the smallest d2; partner: the other body with the smallest e; strict <, the lowest index among equals.  A
candidate whose value is NaN or whose d2 is not finite is never chosen; nobody chosen: index -1, d2 = e = +inf.

An argmin is only as sure as the distance to its runner-up, so every row carries its gap:
    nearest: (d2_2 - d2_1) / d2_2        partner: (e_2 - e_1) / max(|e_1|, |e_2|)
with the runner-up (., _2) the best of all OTHER candidates (an exact tie has gap 0; no runner-up: gap 1).  The device tests hold
indices to this reference only where the gap is far above the arithmetic's error (1e-9 against 1e-12) and fail on a scene that has a
row below it."""
import numpy as np

from jerk_ref import G

GAP_MIN = 1e-9                                                     # 1000 x the project's fp64 parity bound (test_jerk_gpu.py: TOL_F64)
CASES = [(1000, 25), (257, 300), (4097, 64)]                       # (N, M) of pot_tidal_f64_ref.plummer_scene
EPS = [0.0, 0.05]
N_CHUNKS = 32769                                                   # 65 chunks of 512 bodies, the last one body and 255 pads
ROWS_CHUNKS = list(range(64)) + [511, 512, 513, 16383, 16384, 32767] + list(range(N_CHUNKS - 64, N_CHUNKS))
N_SLAB = 33000
LATTICE_SEED = 1                                                   # chosen on the CPU: test_census_f64_ref.py holds its gaps


def _two_smallest(val, keys=None):
    """(index of the first smallest, smallest, second smallest over all other columns) per row of val (no NaN; +inf = no candidate).
    keys: arrays shaped like val; the columns that equal the chosen one in every key are its exact ties and are no runner-up."""
    rows = np.arange(val.shape[0])
    at = np.argmin(val, axis=1)                                    # the first of equals: the lowest index
    best = val[rows, at]
    rest = val.copy()
    rest[rows, at] = np.inf
    if keys is not None:
        tied = np.ones(val.shape, bool)
        for key in keys:
            tied &= key == key[rows, at][:, None]
        rest[tied] = np.inf
    return at, best, rest.min(axis=1)


def census(pos, mass, vel, pts=None, pvel=None, rows=None, eps=(0.0,), dtype=np.float64, g=G, beyond_exact_ties=False):
    """One dict per eps in `eps`, every array in `dtype` but the indices (int32):
        near, near_d2, near_gap                       (the same for every eps: d2 is never softened)
        part, part_e, part_d2, part_gap, part_scale   part_scale = 0.5 |w|^2 + (G m_j + g) t of the chosen pair: what e cancels from
    pts None: the rows are the bodies `rows` (None: all), each leaves itself out by index and has g = G m_i; else the rows are the
    points `pts` moving with `pvel` (None: at rest), g = 0, and nothing is dropped by index.  beyond_exact_ties (scenes whose d2 and
    |w|^2 are exact and whose masses are equal): the gaps are those to the best candidate that is NOT an exact tie of the chosen one —
    equal d2 (nearest), equal d2 and |w|^2 (partner) —, since exact ties are decided by the index, not by the arithmetic."""
    pos = np.asarray(pos, dtype)[:, :3]; vel = np.asarray(vel, dtype)[:, :3]
    gm = dtype(g) * np.asarray(mass, dtype)
    n = pos.shape[0]
    if pts is None:
        own = np.arange(n) if rows is None else np.asarray(rows)
        x, v, gi = pos[own], vel[own], gm[own]
    else:
        own = None
        x = np.asarray(pts, dtype)[:, :3]
        v = np.zeros_like(x) if pvel is None else np.asarray(pvel, dtype)[:, :3]
        gi = np.zeros(x.shape[0], dtype)
    m = x.shape[0]
    inf, zero, half, one = dtype(np.inf), dtype(0), dtype(0.5), dtype(1)
    out = [{"near": np.empty(m, np.int32), "near_d2": np.empty(m, dtype), "near_gap": np.empty(m, dtype),
            "part": np.empty(m, np.int32), "part_e": np.empty(m, dtype), "part_d2": np.empty(m, dtype), "part_gap": np.empty(m, dtype),
            "part_scale": np.empty(m, dtype)} for _ in eps]
    blk = max(1, min(1024, 1_000_000 // max(1, n)))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a in range(0, m, blk):
            b = min(a + blk, m)
            k = np.arange(b - a)
            d = pos[None, :, :] - x[a:b, None, :]
            d2 = (d * d).sum(-1)
            w = vel[None, :, :] - v[a:b, None, :]
            w2 = (w * w).sum(-1)
            other = np.ones(d2.shape, bool)
            if own is not None:
                other[k, own[a:b]] = False
            admit = other & np.isfinite(d2)
            at, best, second = _two_smallest(np.where(admit, d2, inf), (d2,) if beyond_exact_ties else None)
            none = ~(best < inf)
            ngap = np.where(second < inf, np.where(second > 0, (second - best) / np.where(second > 0, second, one), zero), one)
            mu = gm[None, :] + gi[a:b, None]
            for o, ep in zip(out, eps):
                o["near"][a:b] = np.where(none, -1, at); o["near_d2"][a:b] = best; o["near_gap"][a:b] = np.where(none, one, ngap)
                s2 = d2 + dtype(ep) * dtype(ep)
                ok = (s2 > 0) & other
                t = np.where(ok, one / np.sqrt(np.where(ok, s2, one)), zero)
                e = half * w2 - mu * t
                pa, pbest, psecond = _two_smallest(np.where(admit & ~np.isnan(e), e, inf), (d2, w2) if beyond_exact_ties else None)
                pnone = ~(pbest < inf)
                den = np.maximum(np.abs(pbest), np.abs(psecond))
                pgap = np.where(psecond < inf, np.where(den > 0, (psecond - pbest) / np.where(den > 0, den, one), zero), one)
                o["part"][a:b] = np.where(pnone, -1, pa); o["part_e"][a:b] = pbest
                o["part_d2"][a:b] = np.where(pnone, inf, d2[k, pa]); o["part_gap"][a:b] = np.where(pnone, one, pgap)
                o["part_scale"][a:b] = np.where(pnone, zero, half * w2[k, pa] + (mu * t)[k, pa])
    return out


def pair_of(index, value):
    """(i, j, value[i]) of nbody_closest_pair_f64 / nbody_hardest_pair_f64 from a per-body pass: the smallest value, the lowest row that
    attains it; (-1, -1, +inf) where no value is below +inf."""
    value = np.asarray(value, np.float64)
    i = int(np.argmin(value))                                      # (the first of equal minima; the passes hand out no NaN)
    if not value[i] < np.inf:
        return -1, -1, np.inf
    return i, int(index[i]), float(value[i])


def pair_time_of(d2, m_i, m_j, g=G):
    """nbody_pair_time_f64's t = sqrt(d2 sqrt(d2) / (G (m_i + m_j))), operation by operation in fp64; +inf for a massless pair."""
    gm = np.float64(g) * (np.float64(m_i) + np.float64(m_j))
    if not gm > 0:
        return np.inf
    d2 = np.float64(d2)
    return float(np.sqrt(d2 * np.sqrt(d2) / gm))


def lattice_scene(seed=LATTICE_SEED, n=300):
    """(posm, vel) in fp64: n bodies of equal mass on small-integer lattice coordinates with small-integer velocities, in shuffled
    order, the last few put exactly onto earlier ones (coincident bodies).  Every operation in d2 and w2 is exact in fp64, so the
    device's d2 equals numpy's in every byte and ties are exact ties."""
    rng = np.random.default_rng(seed)
    side = 7                                                       # 343 sites for ~294 distinct bodies: many equal distances
    sites = rng.permutation(side ** 3)[:n]
    posm = np.zeros((n, 4)); vel = np.zeros((n, 4))
    posm[:, 0], posm[:, 1], posm[:, 2] = sites % side, (sites // side) % side, sites // (side * side)
    posm[:, :3] -= side // 2
    posm[:, 3] = 64.0
    vel[:, :3] = rng.integers(-2, 3, (n, 3))
    twins = rng.permutation(n - 6)[:6]                             # six coincident pairs, the copies far from their originals in index
    posm[n - 6:, :3] = posm[twins, :3]
    return posm, vel


# ---- the scenes of tests/test_census_f64_gpu.py and their long-double answers, computed once and shared, read-only ----
_scenes, _refs = {}, {}
LD = np.longdouble


def scene(nb, n, m=0):
    """(posm, vel, tpos, tvel) in fp64, read-only: pot_tidal_f64_ref.plummer_scene."""
    import pot_tidal_f64_ref as R
    if (n, m) not in _scenes:
        _scenes[(n, m)] = R.plummer_scene(nb, n, m)
        for a in _scenes[(n, m)]:
            a.setflags(write=False)
    return _scenes[(n, m)]


def binary_scene(nb, n=257):
    """(posm, vel, a, ecc): the block sessions' scene — the Plummer sphere with bodies 0 and 1 a hard binary of a = 1, e = 0.5 at
    pericentre, 37 length units from the centre (hermite_block_ref.binary_in_cluster)."""
    import hermite_block_ref as B
    if ("binary", n) not in _scenes:
        posm, vel, _, _ = scene(nb, n)
        p, v, _ = B.binary_in_cluster(posm, vel)
        p.setflags(write=False); v.setflags(write=False)
        _scenes[("binary", n)] = (p, v, 1.0, 0.5)
    return _scenes[("binary", n)]


def probe_slab_points(n_total, width):
    """kernels_probe.hip's: the points whose partial rows (width float4 per point and chunk) fit 256 MiB, a multiple of 1024."""
    from jerk_ref import probe_geometry
    return max(1024, (256 << 20) // (probe_geometry(n_total)[0] * 16 * width) // 1024 * 1024)


def slab_points(nb):
    """(pts, pvel, sampled): probe_slab_points(N_SLAB, 2) + 1000 moving points in the N_SLAB scene, and the 32 of them held to long double."""
    if "slab" not in _scenes:
        posm, vel, _, _ = scene(nb, N_SLAB)
        m = probe_slab_points(N_SLAB, 2) + 1000
        rng = np.random.default_rng(33)
        pts = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
        pvel = rng.normal(0.0, float(np.abs(vel[:, :3]).std()) + 1e-3, (m, 3))
        sampled = np.sort(rng.permutation(m)[:32])
        for a in (pts, pvel, sampled):
            a.setflags(write=False)
        _scenes["slab"] = (pts, pvel, sampled)
    return _scenes["slab"]


def reference(nb, kind, n, m=0, dtype=LD):
    """{eps: census dict} over EPS in `dtype`, computed once: kind "bodies" (every body of scene(n)), "points" (scene(n, m)'s moving
    points), "chunks" (the bodies ROWS_CHUNKS of scene(N_CHUNKS)), "slab" (the sampled points of slab_points)."""
    key = (kind, n, m, dtype)
    if key not in _refs:
        if kind == "slab":
            posm, vel, _, _ = scene(nb, N_SLAB)
            pts, pvel, sampled = slab_points(nb)
            got = census(posm[:, :3], posm[:, 3], vel, pts[sampled], pvel[sampled], eps=EPS, dtype=dtype)
        elif kind == "chunks":
            posm, vel, _, _ = scene(nb, N_CHUNKS)
            got = census(posm[:, :3], posm[:, 3], vel, rows=ROWS_CHUNKS, eps=EPS, dtype=dtype)
        else:
            posm, vel, tpos, tvel = scene(nb, n, m)
            got = census(posm[:, :3], posm[:, 3], vel, eps=EPS, dtype=dtype) if kind == "bodies" else \
                census(posm[:, :3], posm[:, 3], vel, tpos, tvel, eps=EPS, dtype=dtype)
        for o in got:
            for a in o.values():
                a.setflags(write=False)
        _refs[key] = dict(zip(EPS, got))
    return _refs[key]


def gaps_hold(ref):
    """The gap condition on one census dict: every row's answer is more than GAP_MIN from its runner-up.  Returns the two smallest gaps."""
    near, part = float(ref["near_gap"].min()), float(ref["part_gap"].min())
    assert near > GAP_MIN and part > GAP_MIN, f"a row of this scene is too close to a tie: nearest gap {near:.3e}, partner gap {part:.3e}"
    return near, part
