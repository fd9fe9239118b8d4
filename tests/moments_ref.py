"""Plain numpy / math.fsum references for tests/test_moments_gpu.py and tests/test_moments_abi.py: the 24 sums of nbody_get_moments, the
mass profile of nbody_mass_within, the tolerance both are held to, and a restatement of the launch geometry (csrc/kernels_moments.hip,
moments_geometry).  Nothing here touches a GPU.

Tolerance.  For a sum S = sum t_i over n bodies the reference S0 is math.fsum of the fp64 terms — the correctly rounded sum of the terms as
numpy forms them from exactly the values the context holds.  A is the sum over the bodies of the absolute values of the products that enter
t_i (for l[0]: sum |m| (|y vz| + |z vy|)).  Any order of fp64 summation of n terms, each formed with at most a few roundings (fused or
not), lies within GAMMA(n) * A of S0, GAMMA(n) = (n + 16) * 2^-53: n - 1 additions of relative error 2^-53 each against the partial sums'
bound A, and up to 16 roundings for forming a term on either side and for fsum's own."""
import math
from fractions import Fraction

import numpy as np

K_BLOCK = 256            # kBlock, csrc/pk_common.h
SLOT_CAP = 1024          # kMomentSlotCap, csrc/kernels.h
MASS_WITHIN_MAX = 64     # kMassWithinMax

# the 24 sums in the order of struct nbody_moments
NAMES = (["mass"] + [f"mx[{a}]" for a in range(3)] + [f"p[{a}]" for a in range(3)] + [f"l[{a}]" for a in range(3)]
         + [f"second[{a}]" for a in range(6)] + ["kinetic", "virial"] + [f"force[{a}]" for a in range(3)] + [f"torque[{a}]" for a in range(3)])
FIELDS = ("mass", "mx", "p", "l", "second", "kinetic", "virial", "force", "torque")


def gamma(n):
    return (n + 16) * 2.0 ** -53


def geometry(i_count):
    """(workgroups launched = slots, bodies per workgroup) of both calls: a function of the owned count alone."""
    n = max(int(i_count), 1)
    cap = min(SLOT_CAP, -(-n // K_BLOCK))
    per = -(-n // cap)
    return -(-n // per), per


def flat(m):
    """The 24 sums of a MomentsResult (or anything with the fields of FIELDS) as one float64 vector in NAMES' order."""
    return np.concatenate([np.atleast_1d(np.asarray(getattr(m, k), np.float64)) for k in FIELDS])


def _cross_terms(m, a, b):
    """terms and absolute terms of m (a x b), [n, 3] each"""
    t, s = [], []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        u, w = a[:, i] * b[:, j], a[:, j] * b[:, i]
        t.append(m * (u - w))
        s.append(np.abs(m) * (np.abs(u) + np.abs(w)))
    return np.stack(t, 1), np.stack(s, 1)


def terms(posm, vel, acc):
    """(terms [n, 24], absolute products [n, 24]) in fp64 from the values as they are held (float32 arrays are widened)."""
    p, v, a = (np.asarray(q, np.float64) for q in (posm, vel, acc))
    x, m = p[:, :3], p[:, 3]
    v, a = v[:, :3], a[:, :3]
    mm = m[:, None]
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    second = np.stack([m * (x[:, i] * x[:, j]) for i, j in pairs], 1)
    lt, la = _cross_terms(m, x, v)
    tt, ta = _cross_terms(m, x, a)
    kin = 0.5 * m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    xa = x * a
    vir = m * ((xa[:, 0] + xa[:, 1]) + xa[:, 2])
    t = np.concatenate([mm, mm * x, mm * v, lt, second, kin[:, None], vir[:, None], mm * a, tt], 1)
    s = np.concatenate([np.abs(mm), np.abs(mm * x), np.abs(mm * v), la, np.abs(second), np.abs(kin)[:, None],
                        (np.abs(m) * np.abs(xa).sum(1))[:, None], np.abs(mm * a), ta], 1)
    assert t.shape == s.shape == (p.shape[0], 24)
    return t, s


def reference(posm, vel, acc):
    """(S0 [24], A [24]): math.fsum of every column of terms()."""
    t, s = terms(posm, vel, acc)
    return (np.array([math.fsum(t[:, k].tolist()) for k in range(24)]), np.array([math.fsum(s[:, k].tolist()) for k in range(24)]))


def exact_sums(posm, vel, acc):
    """The 24 sums in exact rational arithmetic from the same values: [24] Fractions.  For small scenes (checks the checker)."""
    out = [Fraction(0)] * 24
    F = Fraction
    for pm, vv, aa in zip(np.asarray(posm, np.float64), np.asarray(vel, np.float64), np.asarray(acc, np.float64)):
        x, m = [F(float(c)) for c in pm[:3]], F(float(pm[3]))
        v, a = [F(float(c)) for c in vv[:3]], [F(float(c)) for c in aa[:3]]
        cross = lambda q, w: [q[1] * w[2] - q[2] * w[1], q[2] * w[0] - q[0] * w[2], q[0] * w[1] - q[1] * w[0]]
        row = ([m] + [m * c for c in x] + [m * c for c in v] + [m * c for c in cross(x, v)]
               + [m * x[i] * x[j] for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
               + [m * sum(c * c for c in v) / 2, m * sum(c * d for c, d in zip(x, a))] + [m * c for c in a] + [m * c for c in cross(x, a)])
        out = [o + r for o, r in zip(out, row)]
    return out


def distances2(posm, centre):
    """d2 of every body as nbody_mass_within forms it: dx = (double)x - centre[0], d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded
    on its own (numpy fuses nothing)."""
    p = np.asarray(posm, np.float64)
    c = np.asarray(centre, np.float64)
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def mass_within(posm, centre, radii):
    """(mass [k] by math.fsum, count [k] int64, A [k] = sum of |m| of the members) under the stated membership rule d2 <= r * r."""
    m = np.asarray(posm, np.float64)[:, 3]
    d2 = distances2(posm, centre)
    r = np.asarray(radii, np.float64).reshape(-1)
    mass, count, big = np.zeros(r.shape[0]), np.zeros(r.shape[0], np.int64), np.zeros(r.shape[0])
    for q in range(r.shape[0]):
        inside = d2 <= r[q] * r[q]
        count[q] = int(inside.sum())
        mass[q] = math.fsum(m[inside].tolist())
        big[q] = math.fsum(np.abs(m[inside]).tolist())
    return mass, count, big


def assert_moments(got24, posm, vel, acc, label=""):
    """|S - S0| <= GAMMA(n) A for each of the 24 sums; prints the worst ratio.  Returns (S0, A)."""
    s0, big = reference(posm, vel, acc)
    n = np.asarray(posm).shape[0]
    bound = gamma(n) * big
    err = np.abs(np.asarray(got24, np.float64) - s0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    print(f"moments {label}: n = {n}, worst |S - S0| / (gamma A) = {ratio[k]:.3e} in {NAMES[k]}")
    for j in range(24):
        assert np.isfinite(got24[j]) and err[j] <= bound[j], (label, NAMES[j], float(got24[j]), float(s0[j]), float(err[j]), float(bound[j]))
    return s0, big
