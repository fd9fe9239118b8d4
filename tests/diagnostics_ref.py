"""Plain numpy references for tests/test_diagnostics_gpu.py: scenes, the energy shares of a slice of the bodies, and a
restatement of the geometry nbody_energy launches with (csrc/kernels.hip, energy_geometry).  Nothing here touches a GPU."""
from fractions import Fraction

import numpy as np

REF_G = 1.0e4          # OctreeSearch.h:104
K_BLOCK = 256          # kBlock, csrc/kernels.h


def scene(n, seed, dtype=np.float32, equal=False, box=500.0):
    """tests/test_block_gpu.py::scene in either width: positions uniform in +-box, masses 1..5000, velocities +-5, body 0 at
    the origin.  float64 scenes are drawn as doubles (all 53 bits in use), not widened floats."""
    rng = np.random.default_rng(seed)
    posm = np.concatenate([rng.uniform(-box, box, (n, 3)), rng.uniform(1, 5000, (n, 1))], 1).astype(dtype)
    if equal:
        posm[:, 3] = 37.5
    if n > 3:
        posm[0, :3] = 0.0
    vel = np.concatenate([rng.uniform(-5, 5, (n, 3)), np.zeros((n, 1))], 1).astype(dtype)
    return posm, vel


def energy_geometry(n_total, i_count=None):
    """(i-blocks, chunks launched, bodies per chunk) of nbody_energy: the j range is halved while that leaves fewer than 2048
    workgroups and chunks of at least four tiles; the chunk is then rounded up to whole tiles and the count recomputed."""
    i_count = n_total if i_count is None else i_count
    iblocks = (i_count + K_BLOCK - 1) // K_BLOCK
    js = 1
    while iblocks * js < 2048 and n_total // (js * 2) >= 4 * K_BLOCK:
        js *= 2
    chunk = (n_total + js - 1) // js
    chunk = (chunk + K_BLOCK - 1) // K_BLOCK * K_BLOCK
    return iblocks, (n_total + chunk - 1) // chunk, chunk


def potentials_f64(posm, g=REF_G, eps=0.0, rows=16):
    """phi_i = -G sum_j m_j / sqrt(d_ij^2 + eps^2) over all bodies j != i, pairs with d^2 + eps^2 == 0 skipped: [n] float64."""
    p = np.asarray(posm, np.float64)
    n = p.shape[0]
    x, y, z, m = (np.ascontiguousarray(p[:, k]) for k in range(4))
    eps2 = float(eps * eps)
    phi = np.empty(n, np.float64)
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        dx = x[None, :] - x[r0:r1, None]
        dy = y[None, :] - y[r0:r1, None]
        dz = z[None, :] - z[r0:r1, None]
        r2 = dx * dx + dy * dy + dz * dz + eps2
        r2[np.arange(r1 - r0), np.arange(r0, r1)] = 0.0          # no self term
        r2[r2 == 0.0] = np.inf                                    # ... and no pair at distance 0: 1 / sqrt(inf) = 0
        phi[r0:r1] = -g * ((1.0 / np.sqrt(r2)) * m[None, :]).sum(1)
    return phi


def kinetic_terms_f64(posm, vel):
    p = np.asarray(posm, np.float64)
    v = np.asarray(vel, np.float64)
    return 0.5 * p[:, 3] * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def energy_shares(posm, vel, cuts, g=REF_G, eps=0.0, phi=None):
    """[(ke, pe)] of the bodies [cuts[k], cuts[k+1]): ke = sum 1/2 m v^2 over the owned bodies, pe = sum 1/2 m_i phi_i over
    them, phi_i from ALL bodies.  posm and vel hold all n bodies."""
    p = np.asarray(posm, np.float64)
    if phi is None:
        phi = potentials_f64(p, g, eps)
    k = kinetic_terms_f64(p, vel)
    u = 0.5 * p[:, 3] * phi
    return [(float(k[lo:hi].sum()), float(u[lo:hi].sum())) for lo, hi in zip(cuts[:-1], cuts[1:])]


def one_body_kinetic(m, v):
    """Every value double arithmetic can give 0.5 * m * ((vx*vx + vy*vy) + vz*vz) for one body: each of the two additions either
    rounds its product first or is fused with it (one rounding of the exact a*b + c; which, is the compiler's choice).  No
    tolerance: a kernel must return one of these, to the bit.  For float velocities widened to double the products are exact and
    the set has one member."""
    m = float(m)
    vx, vy, vz = (float(c) for c in v[:3])
    fx, fy, fz = Fraction(vx), Fraction(vy), Fraction(vz)
    first = {vx * vx + vy * vy,                                   # both products rounded
             float(fx * fx + Fraction(vy * vy)),                  # fma(vx, vx, vy * vy)
             float(Fraction(vx * vx) + fy * fy)}                  # fma(vy, vy, vx * vx)
    out = set()
    for s in first:
        out.add(0.5 * m * (s + vz * vz))
        out.add(0.5 * m * float(Fraction(s) + fz * fz))           # fma(vz, vz, s)
    return out


def moved_partner_difference(posm, a, b, shift, g=REF_G, eps=0.0):
    """pe(scene) - pe(scene with body a moved by `shift`), for a body a that coincides with body b and eps > 0: the pair's own
    -G m_a m_b / eps, plus what the move changes in every other term of a — O(n) terms, no cancellation of whole energies."""
    p = np.asarray(posm, np.float64)
    assert eps > 0.0 and np.array_equal(p[a, :3], p[b, :3])
    eps2 = float(eps * eps)
    here = p[a, :3]
    there = here + np.asarray(shift, np.float64)
    others = np.ones(p.shape[0], bool)
    others[[a, b]] = False
    q = p[others]
    r_here = np.sqrt(((q[:, :3] - here) ** 2).sum(1) + eps2)
    r_there = np.sqrt(((q[:, :3] - there) ** 2).sum(1) + eps2)
    own = -g * p[a, 3] * p[b, 3] / eps
    rest = g * p[a, 3] * p[b, 3] / np.sqrt(((there - p[b, :3]) ** 2).sum() + eps2) \
        - g * p[a, 3] * float((q[:, 3] * (1.0 / r_here - 1.0 / r_there)).sum())
    return own + rest, own
