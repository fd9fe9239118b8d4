"""The yardsticks of nbody_potential_at_f64, nbody_get_potentials_f64, nbody_tidal_at_f64, nbody_get_tidal_f64 and nbody_tidal_time_f64:
the plain numpy sums of the definitions in float64 and np.longdouble, and the kernel's summation ORDER restated on the CPU.  TEST
INFRASTRUCTURE ONLY.

With d = x_j - x and s^2 = |d|^2 + eps^2:
    phi(x)  = -sum_j G m_j / s
    T_ab(x) =  sum_j G m_j [3 d_a d_b / s^5 - delta_ab / s^3]          six components: xx, yy, zz, xy, xz, yz
A pair with s^2 == 0 adds nothing to either sum; the per-body forms leave the body itself out by index."""
import numpy as np

from jerk_ref import G, probe_geometry

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))           # xx, yy, zz, xy, xz, yz


def direct(pos, mass, pts, eps=0.0, skip_self=False, dtype=np.float64, g=G):
    """(phi [m], T [m,6]) in `dtype` (np.float64 or np.longdouble): the sums of the definitions over all bodies at the points `pts`.
    skip_self: the points are the bodies themselves and row k leaves body k out by index."""
    pos = np.asarray(pos, dtype)[:, :3]; mass = np.asarray(mass, dtype); pts = np.asarray(pts, dtype)[:, :3]
    m, n = pts.shape[0], pos.shape[0]
    phi = np.empty(m, dtype); t6 = np.empty((m, 6), dtype)
    e2 = dtype(eps) * dtype(eps)
    one, three = dtype(1), dtype(3)
    blk = max(16, min(1024, 1_000_000 // max(1, n)))
    for a in range(0, m, blk):
        d = pos[None, :, :] - pts[a:a + blk, None, :]
        s2 = (d * d).sum(-1) + e2
        ok = s2 > 0
        inv = np.where(ok, one / np.sqrt(np.where(ok, s2, one)), dtype(0))
        if skip_self:
            k = np.arange(a, min(a + blk, m))
            inv[k - a, k] = 0
        gm = dtype(g) * mass[None, :]
        phi[a:a + blk] = -(gm * inv).sum(1)
        q = gm * inv * inv * inv                                   # g m / s^3
        h = three * q * inv * inv                                  # 3 g m / s^5
        for c, (x, y) in enumerate(PAIRS):
            term = h * d[..., x] * d[..., y]
            if x == y:
                term = term - q
            t6[a:a + blk, c] = term.sum(1)
    return phi, t6


def kernel_order(pos, mass, pts=None, eps=0.0, g=G):
    """(phi [m], T [m,6]) as kernels_pot64.hip sums them: fp64 per pair with the kernel's brackets, one chain per sum and chunk of
    probe_geometry in body order, the chunks added from 0.0 in chunk order, then phi = -P, T_aa = S_aa - Q.  pts None: the bodies
    themselves, each left out by index.  Multiplies and adds are numpy's own (no fused multiply-add, a correctly rounded root): the
    ORDER of the sums is the kernel's, not its last bit — this sizes the bound, it is not meant to match bits."""
    f64 = np.float64
    pos = np.asarray(pos, f64)[:, :3]
    gm = np.asarray(mass, f64) * f64(g)
    self_form = pts is None
    x = pos if self_form else np.asarray(pts, f64)[:, :3]
    m, n = x.shape[0], pos.shape[0]
    e2 = f64(eps) * f64(eps)
    chunk = probe_geometry(n)[1]
    P = np.zeros(m, f64); S = np.zeros((m, 7), f64)
    idx = np.arange(m)
    for c0 in range(0, n, chunk):
        j = np.arange(c0, min(c0 + chunk, n))
        d = pos[None, j, :] - x[:, None, :]
        s2 = d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + (d[..., 2] * d[..., 2] + e2))
        ok = s2 > 0
        if self_form:
            ok &= idx[:, None] != j[None, :]
        t = np.where(ok, 1.0 / np.sqrt(np.where(ok, s2, 1.0)), 0.0)
        t2 = t * t
        q = (gm[None, j] * t) * t2
        h = (3.0 * q) * t2
        hd = h[..., None] * d                                      # hx, hy, hz
        terms = np.stack([hd[..., 0] * d[..., 0], hd[..., 1] * d[..., 1], hd[..., 2] * d[..., 2],
                          hd[..., 0] * d[..., 1], hd[..., 0] * d[..., 2], hd[..., 1] * d[..., 2], q], axis=2)
        pc = np.zeros(m, f64); sc = np.zeros((m, 7), f64)
        for b in range(j.size):                                    # the chains, in body order
            pc = gm[j[b]] * t[:, b] + pc
            sc = terms[:, b, :] + sc
        P = P + pc; S = S + sc
    t6 = S[:, :6].copy()
    t6[:, :3] -= S[:, 6:7]
    return -P, t6


def n2_of(t6):
    """||T||_F^2 as nbody_tidal_time forms it, operation by operation in fp64: (Txx^2 + Tyy^2) + Tzz^2 + 2 ((Txy^2 + Txz^2) + Tyz^2);
    a value that is not finite counts as +inf."""
    t = np.asarray(t6, np.float64)
    sq = t * t
    n2 = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + 2.0 * ((sq[:, 3] + sq[:, 4]) + sq[:, 5])
    return np.where(np.isfinite(n2), n2, np.inf)


def tidal_time_of(t6):
    """(t_min, body) of nbody_tidal_time_f64 from the unrounded tensors: the largest n2, the lowest index that attains it."""
    n2 = n2_of(t6)
    body = int(np.argmax(n2))                                     # (the first of equal maxima)
    top = float(n2[body])
    t = np.inf if top == 0.0 else (float(np.float64(1.0) / np.sqrt(np.sqrt(np.float64(top)))) if np.isfinite(top) else 0.0)
    return t, body


def rel_phi(got, ref):
    """max |got - ref| / |ref| over the rows; a row whose reference is exactly zero must be exactly zero."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    zero = ref == 0.0
    assert not got[zero].any()
    return float(np.max(np.where(zero, 0.0, np.abs(got - ref) / np.where(zero, 1.0, np.abs(ref))), initial=0.0))


def plummer_scene(nb, n, m=0):
    """(posm, vel, tpos, tvel) in fp64 — tests/test_tracers_f64_gpu.py's scene(): a Plummer sphere whose masses all differ and whose
    coordinates are no fp32 numbers, and m random moving points inside it."""
    p32, v32 = nb.ic_plummer(n, seed=n)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    posm[:, :3] += 1e-7 * posm[:, :3] ** 2 + 1e-9
    vel[:, :3] += 1e-7 * vel[:, :3] ** 2 + 1e-9
    posm[:, 3] *= 1.0 + 0.5 * np.arange(n) / n + 1e-9 * np.arange(n)
    vel[:, 3] = 0.0
    rng = np.random.default_rng(7000 + n + m)
    tpos = rng.normal(0.0, float(np.abs(posm[:, :3]).std()), (m, 3))
    tvel = rng.normal(0.0, float(np.abs(vel[:, :3]).std()) + 1e-3, (m, 3))
    return posm, vel, tpos, tvel
