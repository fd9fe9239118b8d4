"""NBodyEngine — Python handle on one nbody_ctx (include/nbody.h).  All arithmetic happens in the HIP
kernels of libnbody_amd.so; this file only moves numpy buffers across the C-ABI."""
import collections
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import NBodyError, Params

# FParticle, /root/reference/Source/NBody/OctreeSearch.h:8-18 (40 bytes)
PARTICLE_DTYPE = np.dtype(
    [("Mass", "<f4"), ("Position", "<f4", (3,)), ("Velocity", "<f4", (3,)), ("Acceleration", "<f4", (3,))])

REF_G = 1.0e4       # OctreeSearch.h:104
REF_DT = 0.01       # OctreeSearch.cpp:8

_PREC = {"f32": _lib.PREC_F32, "f32_kahan": _lib.PREC_F32_KAHAN, "f64": _lib.PREC_F64}


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def ic_reference_box(n, size=200.0, center=(0.0, 0.0, 0.0), seed=1):
    """Seeded CreateSpacePoints distribution (OctreeSearch.cpp:58-72).  Returns (posm[n,4], vel[n,4]) fp32."""
    posm = np.empty((n, 4), np.float32)
    vel = np.empty((n, 4), np.float32)
    c = np.asarray(center, np.float32)
    rc = _lib.lib().nbody_ic_reference_box(n, size, _fp(c), seed, _fp(posm), _fp(vel))
    if rc:
        raise NBodyError(rc, "nbody_ic_reference_box: invalid argument")
    return posm, vel


def ic_plummer(n, total_mass=1000.0, scale_radius=100.0, G=REF_G, seed=1):
    """Seeded equal-mass Plummer sphere in virial equilibrium.  Returns (posm[n,4], vel[n,4]) fp32."""
    posm = np.empty((n, 4), np.float32)
    vel = np.empty((n, 4), np.float32)
    rc = _lib.lib().nbody_ic_plummer(n, total_mass, scale_radius, G, seed, _fp(posm), _fp(vel))
    if rc:
        raise NBodyError(rc, "nbody_ic_plummer: invalid argument")
    return posm, vel


def sym_plan(n_total, i_begin=0, i_count=0, bodies_per_iset=4096, slots=512, k_guided=3, min_sub=4, own_mode=1):
    """The work plan of the symmetric force pass (csrc/sym_plan.h), host only.  Returns (items[n,8] int32 —
    i0, j0, n_sub, flags (1 = own-block strip, 2 = no j-side sums), slot_i, slot_j, 0, 0 —, pool_elems).
    k_guided may be fractional in tenths (the library itself uses 1, 1.5, 3 and 6)."""
    L = _lib.lib()
    n, pe = ctypes.c_int32(), ctypes.c_uint64()
    k10 = int(round(float(k_guided) * 10))
    if abs(k10 - float(k_guided) * 10) > 1e-9:
        raise ValueError("k_guided must be a multiple of 0.1")
    rc = L.nbody_sym_plan_describe_tenths(n_total, i_begin, i_count, bodies_per_iset, slots, k10, min_sub, own_mode, ctypes.byref(n),
                                          ctypes.byref(pe), None, 0)
    if rc:
        raise NBodyError(rc, "nbody_sym_plan_describe: this range cannot be planned")
    items = np.zeros((n.value, 8), np.int32)
    rc = L.nbody_sym_plan_describe_tenths(n_total, i_begin, i_count, bodies_per_iset, slots, k10, min_sub, own_mode, ctypes.byref(n),
                                          ctypes.byref(pe), items.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.value)
    if rc:
        raise NBodyError(rc, "nbody_sym_plan_describe: this range cannot be planned")
    return items, pe.value


def sym_plan_phased(n_total, j_budget_elems, i_begin=0, i_count=0, bodies_per_iset=4096, slots=512, k_guided=3, min_sub=4):
    """A plan whose j-side segments share a pool area of at most j_budget_elems elements (csrc/sym_plan.h, pool phases).
    Returns (items[n,8], pool_elems, phase_item0[n_phases + 1])."""
    L = _lib.lib()
    n, pe, nph = ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int32()
    k10 = int(round(float(k_guided) * 10))
    args = (n_total, i_begin, i_count, bodies_per_iset, slots, k10, min_sub, int(j_budget_elems))
    rc = L.nbody_sym_plan_describe_phased(*args, ctypes.byref(n), ctypes.byref(pe), None, 0, ctypes.byref(nph), None, 0)
    if rc:
        raise NBodyError(rc, "nbody_sym_plan_describe_phased: this range cannot be planned")
    items = np.zeros((n.value, 8), np.int32)
    ph = np.zeros(nph.value + 1, np.int32)
    rc = L.nbody_sym_plan_describe_phased(*args, ctypes.byref(n), ctypes.byref(pe), items.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          n.value, ctypes.byref(nph), ph.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nph.value + 1)
    if rc:
        raise NBodyError(rc, "nbody_sym_plan_describe_phased: this range cannot be planned")
    return items, pe.value, ph


def sym_plan_even(n_total, bodies_per_iset=2048, n_items=768):
    """The even-share plan of the symmetric pass (csrc/sym_plan.h), host only.  Returns (items[n,8] int32 — i0, j0, n_sub,
    flags, slot_i, slot_j, k0, k_skip —, pool_elems)."""
    L = _lib.lib()
    n, pe = ctypes.c_int32(), ctypes.c_uint64()
    rc = L.nbody_sym_plan_describe_even(n_total, bodies_per_iset, n_items, ctypes.byref(n), ctypes.byref(pe), None, 0)
    if rc:
        raise NBodyError(rc, "nbody_sym_plan_describe_even: this system cannot be planned")
    items = np.zeros((n.value, 8), np.int32)
    rc = L.nbody_sym_plan_describe_even(n_total, bodies_per_iset, n_items, ctypes.byref(n), ctypes.byref(pe),
                                        items.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.value)
    if rc:
        raise NBodyError(rc, "nbody_sym_plan_describe_even: this system cannot be planned")
    return items, pe.value


MOMENT_FIELDS = ("mass", "mx", "p", "l", "second", "kinetic", "virial", "force", "torque")

# NBodyEngine.moments(): the raw sums of struct nbody_moments (floats / float64 arrays, about the origin; `second` = xx, yy, zz, xy, xz,
# yz), then what the parallel-axis identities give on the host: com = mx / mass, com_velocity = p / mass, l_about_com = l - com x p
MomentsResult = collections.namedtuple("MomentsResult", ("count",) + MOMENT_FIELDS + ("com", "com_velocity", "l_about_com"))


# NBodyEngine.core_f64(): the fields of struct nbody_core (centre a float64 array of 3), then — Python only — the mass and the number
# of bodies within core_radius of the centre, from mass_within()
CoreResult = collections.namedtuple("CoreResult", ("k", "used", "densest", "rho_max", "centre", "core_radius", "rho_sum", "rho2_sum",
                                                   "core_mass", "core_count"))


# NBodyEngine.lagrange_f64(): the centre used (float64[3]), the total mass, then one entry per fraction — the columns of struct
# nbody_lagrange: fraction, r2, radius, mass (float64), body, count (int32)
LagrangeResult = collections.namedtuple("LagrangeResult", ("centre", "total_mass", "fraction", "r2", "radius", "mass", "body", "count"))

# NBodyEngine.radial_profile_f64(): per shell between consecutive Lagrangian positions (radial_profile())
RadialProfileResult = collections.namedtuple("RadialProfileResult", ("centre", "total_mass", "fraction", "count", "mass", "r_in", "r_out",
                                                                     "density", "v_r", "sigma_r2", "sigma_t2", "beta"))

# NBodyEngine.groups_f64(): the fields of struct nbody_groups
GroupsSummary = collections.namedtuple("GroupsSummary", ("groups", "multiples", "largest", "largest_members", "rounds", "links"))

# NBodyEngine.groups_f64(): per body label, members, degree (int32[n_total]), then the summary
GroupsResult = collections.namedtuple("GroupsResult", ("label", "members", "degree", "summary"))

# NBodyEngine.mst_f64(): the fields of struct nbody_mst
MstSummary = collections.namedtuple("MstSummary", ("edges", "components", "rounds", "length", "longest_d2"))

# NBodyEngine.mst_f64(): the edges i < j with their d2 in ascending (d2, i, j) order (int32, int32, float64: [summary.edges] each), per
# body the lowest index of its component (int32[n_total]), then the summary
MstResult = collections.namedtuple("MstResult", ("i", "j", "d2", "component", "summary"))

# NBodyEngine.group_table_f64(): one row per group (group_table())
GROUP_TABLE_DTYPE = np.dtype([("label", np.int32), ("count", np.int32), ("mass", np.float64), ("com", np.float64, 3),
                              ("velocity", np.float64, 3), ("r_rms", np.float64), ("sigma", np.float64)])


def group_table(label, posm, vel, min_members=2):
    """The groups of at least `min_members` bodies in label order, a structured array (GROUP_TABLE_DTYPE), from the labels and the
    fp64 state, in numpy.  Over the bodies i of a group, in index order:
        count = their number;  mass = M = sum m_i;  com = sum m_i x_i / M;  velocity = sum m_i v_i / M
        r_rms = sqrt(sum m_i |x_i - com|^2 / M);  sigma = sqrt(sum m_i |v_i - velocity|^2 / M)      (the three-dimensional dispersion)
    A group whose mass is 0 has NaN com, velocity, r_rms and sigma."""
    label = np.asarray(label)
    labels, counts = np.unique(label, return_counts=True)
    keep = counts >= int(min_members)
    out = np.zeros(int(keep.sum()), GROUP_TABLE_DTYPE)
    for row, (l, k) in zip(out, zip(labels[keep], counts[keep])):
        at = np.flatnonzero(label == l)
        m, x, v = posm[at, 3], posm[at, :3], vel[at, :3]
        mass = m.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            com, vm = (m[:, None] * x).sum(0) / mass, (m[:, None] * v).sum(0) / mass
            r_rms = np.sqrt((m * ((x - com) ** 2).sum(1)).sum() / mass)
            sigma = np.sqrt((m * ((v - vm) ** 2).sum(1)).sum() / mass)
        row["label"], row["count"], row["mass"], row["com"], row["velocity"], row["r_rms"], row["sigma"] = l, k, mass, com, vm, r_rms, sigma
    return out


def mst_groups(i, j, d2, n, radius):
    """(label, members), int32[n] each: the connected components of n bodies under the edges (i, j) whose d2 <= radius * radius — a
    union-find, the lower root winning, so a label is the lowest index of its group.  The edges are ascending in d2 (a spanning
    forest's): those within the radius are a prefix."""
    r2 = np.float64(radius) * np.float64(radius)
    if not (np.isfinite(radius) and radius >= 0.0 and np.isfinite(r2)):
        raise ValueError("mst_groups: the radius must be finite and >= 0 and its square finite")
    keep = int(np.searchsorted(np.asarray(d2, np.float64), r2, "right"))
    parent = list(range(n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r
    for a, b in zip(np.asarray(i)[:keep].tolist(), np.asarray(j)[:keep].tolist()):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    label = np.array([find(a) for a in range(n)], np.int32).reshape(n)
    members = np.bincount(label, minlength=n)[label].astype(np.int32)
    return label, members


# NBodyEngine.correlation_f64(): the Landy-Szalay estimate per bin (float64, NaN where rr == 0) and the raw pair counts per bin (int64)
CorrelationResult = collections.namedtuple("CorrelationResult", ("xi", "dd", "dr", "rr"))


def pair_histogram(edges, cumulative):
    """The pairs per bin (edges[b], edges[b + 1]] — the LOWER edge open, the upper closed — from the cumulative counts at the edges
    (pairs with d2 <= edges[b]^2): int64[len(edges) - 1], the differences of consecutive counts.  The edges must ascend (equal
    neighbours give an empty bin)."""
    e = np.asarray(edges, np.float64).reshape(-1)
    c = np.asarray(cumulative, np.int64).reshape(-1)
    if e.shape[0] < 2 or c.shape != e.shape:
        raise ValueError("pair_histogram: at least two edges, and one cumulative count per edge")
    if not np.all(np.diff(e) >= 0.0):                             # (a NaN edge fails too)
        raise ValueError("pair_histogram: the edges must ascend")
    return np.diff(c)


def landy_szalay(dd, dr, rr, n, n_random):
    """xi = (DD - 2 DR + RR) / RR per bin, each term normalised by its number of pairs: DD = dd / (n (n - 1) / 2), DR = dr / (n n_random),
    RR = rr / (n_random (n_random - 1) / 2), for unordered data-data and random-random counts and data-random (point, body) counts.
    float64; NaN where rr == 0 (and everywhere where a normalisation is 0)."""
    dd, dr, rr = (np.asarray(a, np.float64) for a in (dd, dr, rr))
    n, n_random = float(n), float(n_random)
    with np.errstate(invalid="ignore", divide="ignore"):
        DD, DR, RR = dd / (n * (n - 1.0) / 2.0), dr / (n * n_random), rr / (n_random * (n_random - 1.0) / 2.0)
        xi = (DD - 2.0 * DR + RR) / RR
    return np.where(rr == 0.0, np.nan, xi)


LAGRANGE_FRACTIONS = (0.01,0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9)


def radial_profile(order, posm, vel, centre, counts, radii, vcentre=None):
    """The shells of a radial order, in numpy: count, mass, r_in, r_out, density, v_r, sigma_r2, sigma_t2, beta — float64 arrays with
    one entry per shell (count int64).  order: the bodies in radial order about `centre`; posm, vel: [n, >= 4] and [n, >= 3] float64
    in body order; counts: ascending positions c_0 <= c_1 <= ... (a Lagrangian row's `count`), radii: the rows' `radius`.  Shell s
    holds the sorted positions c_(s-1) <= p < c_s (c_(-1) = 0) — its last body is the one the s-th row selected — and lies between
    r_in = radii[s-1] (0 for s = 0) and r_out = radii[s].  With m_i the shell's masses, M = sum m_i, r_i = x_i - centre,
    e_i = r_i / |r_i| (0 where |r_i| = 0), u_i = v_i - vc, vc = `vcentre` or, None, the shell's own (sum m_i v_i) / M:
        density  = M / ((4 pi / 3) (r_out^3 - r_in^3))
        v_r      = (sum m_i (u_i . e_i)) / M                            the mass-weighted mean radial velocity
        sigma_r2 = (sum m_i ((u_i . e_i) - v_r)^2) / M
        sigma_t2 = (sum m_i (|u_i|^2 - (u_i . e_i)^2)) / M              both tangential components together
        beta     = 1 - sigma_t2 / (2 sigma_r2)                         0: isotropic, 1: radial, -inf: circular orbits
    A shell without mass has mass 0 and NaN for what divides by M."""
    order = np.asarray(order, np.int64)
    posm, vel = np.asarray(posm, np.float64), np.asarray(vel, np.float64)
    centre = np.asarray(centre, np.float64).reshape(3)
    counts, radii = np.asarray(counts, np.int64), np.asarray(radii, np.float64)
    k = counts.shape[0]
    out = {f: np.full(k, np.nan) for f in ("mass", "r_in", "r_out", "density", "v_r", "sigma_r2", "sigma_t2", "beta")}
    count = np.zeros(k, np.int64)
    lo, r_in = 0, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(k):
            hi = max(int(counts[s]), lo)
            ids = order[lo:hi]
            m = posm[ids, 3]
            M = np.float64(m.sum())                               # (a numpy scalar: a shell without mass divides to NaN)
            r = posm[ids, :3] - centre
            d = np.linalg.norm(r, axis=1)
            e = np.where(d[:, None] > 0.0, r / d[:, None], 0.0)
            vc = np.asarray(vcentre, np.float64).reshape(3) if vcentre is not None else (m[:, None] * vel[ids, :3]).sum(axis=0) / M
            u = vel[ids, :3] - vc
            ur = (u * e).sum(axis=1)
            v_r = (m * ur).sum() / M
            count[s] = hi - lo
            out["mass"][s], out["r_in"][s], out["r_out"][s] = M, r_in, radii[s]
            out["density"][s] = M / ((4.0 * np.pi / 3.0) * (radii[s] ** 3 - r_in ** 3))
            out["v_r"][s] = v_r
            out["sigma_r2"][s] = (m * (ur - v_r) ** 2).sum() / M
            out["sigma_t2"][s] = (m * ((u * u).sum(axis=1) - ur * ur)).sum() / M
            out["beta"][s] = 1.0 - out["sigma_t2"][s] / (2.0 * out["sigma_r2"][s])
            lo, r_in = hi, radii[s]
    return count, out


def moments_result(count, sums):
    """MomentsResult from the bodies' count and the raw sums (a mapping of MOMENT_FIELDS) — also of sums added over ranks or slices."""
    raw = {k: (float(sums[k]) if k in ("mass", "kinetic", "virial") else np.array(sums[k], np.float64)) for k in MOMENT_FIELDS}
    with np.errstate(divide="ignore", invalid="ignore"):
        com = raw["mx"] / raw["mass"]
        vcom = raw["p"] / raw["mass"]
    return MomentsResult(count=int(count), **raw, com=com, com_velocity=vcom, l_about_com=raw["l"] - np.cross(com, raw["p"]))


def _params(n_total, i_begin=0, i_count=0, device=0, precision="f32", G=REF_G, eps=0.0, tile=0, i_per_thread=0, j_split=0,
            time_kernels=False, zero_mode=0, algorithm=0, theta=0.0, bh_div_mode=0):
    """struct nbody_params from NBodyEngine's keywords."""
    p = Params()
    _lib.lib().nbody_default_params(ctypes.byref(p))
    p.n_total, p.i_begin, p.i_count, p.device = n_total, i_begin, i_count, device
    p.precision = _PREC[precision] if isinstance(precision, str) else int(precision)
    p.G, p.eps = G, eps
    p.tile, p.i_per_thread, p.j_split = tile, i_per_thread, j_split
    p.time_kernels = 1 if time_kernels else 0
    p.zero_mode = zero_mode
    p.algorithm = algorithm
    p.theta = theta
    p.bh_div_mode = bh_div_mode
    return p


_ALGO_NAME = {_lib.ALGO_TILED: "tiled", _lib.ALGO_SYMMETRIC: "symmetric"}


def launch_policy(n_total, *, compute_units=256, device_total_bytes=0, **engine_keywords):
    """What NBodyEngine(n_total, **engine_keywords) would report on a device with `compute_units` CUs and `device_total_bytes` of
    memory (0: unknown, no plan is refused for its size) — host only, no device needed (nbody_launch_policy_describe).  The keys of
    NBodyEngine.launch_config() plus pool_bytes, phases (sym_pool()), exchange_ranks, wave, detector_slots and the symmetric plan's
    sym_slots, sym_k, sym_min_sub.  Raises NBodyError where the creation would fail for its arguments or its plan."""
    L = _lib.lib()
    p = _params(n_total, **engine_keywords)
    out = _lib.LaunchPolicy()
    out.struct_size = ctypes.sizeof(out)
    rc = L.nbody_launch_policy_describe(ctypes.byref(p), compute_units, device_total_bytes, ctypes.byref(out))
    if rc:
        raise NBodyError(rc, L.nbody_last_error(None).decode())
    cfg = {k: getattr(out, k) for k in ("tile", "i_per_thread", "j_split", "blocks", "threads")}
    cfg["algorithm"] = _ALGO_NAME[out.algorithm]
    cfg["super_tile"] = out.super_tile
    cfg["kernel"] = out.kernel.decode()
    cfg["plan"] = ("even" if out.plan_is_even else "guided") if cfg["algorithm"] == "symmetric" else None
    for k in ("pool_bytes", "phases", "exchange_ranks", "wave", "detector_slots", "sym_slots", "sym_k", "sym_min_sub"):
        cfg[k] = getattr(out, k)
    return cfg


def device_count():
    return int(_lib.lib().nbody_device_count())


class NBodyEngine:
    """One context = one GPU's share [i_begin, i_begin+i_count) of an n_total-body system."""

    def __init__(self, n_total, *, i_begin=0, i_count=0, device=0, precision="f32", G=REF_G, eps=0.0, tile=0,
                 i_per_thread=0, j_split=0, time_kernels=False, zero_mode=0, algorithm=0, theta=0.0, devices=None, bh_div_mode=0):
        L = _lib.lib()
        p = _params(n_total, i_begin, i_count, device, precision, G, eps, tile, i_per_thread, j_split, time_kernels, zero_mode,
                    algorithm, theta, bh_div_mode)
        h = ctypes.c_void_p()
        if devices is not None:
            # one context over several GPUs, driven from this thread (nbody_create_multi: RCCL between the devices)
            devs = (ctypes.c_int32 * len(devices))(*devices)
            rc = L.nbody_create_multi(ctypes.byref(p), devs, len(devices), ctypes.byref(h))
        else:
            rc = L.nbody_create(ctypes.byref(p), ctypes.byref(h))
        if rc:
            raise NBodyError(rc, L.nbody_last_error(None).decode())
        self._L, self._h = L, h
        self.n_total = n_total
        self.i_begin = i_begin
        self.i_count = i_count if i_count else n_total - i_begin
        self.f64 = p.precision == _lib.PREC_F64
        self._G = float(p.G)   # (binaries_f64's elements)
        self._device = device  # (correlation_f64's temporary engine)
        self._keep = []   # externally bound tensors kept alive

    # -- plumbing --
    def _check(self, rc):
        if rc:
            raise NBodyError(rc, self._L.nbody_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.nbody_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state in --
    def set_particles(self, particles):
        a = np.ascontiguousarray(particles)
        assert a.dtype.itemsize >= 40
        self._check(self._L.nbody_set_particles(self._h, a.ctypes.data, a.dtype.itemsize, a.shape[0]))

    def set_state(self, posm, vel):
        if np.asarray(posm).dtype == np.float64:
            p = np.ascontiguousarray(posm, np.float64); v = np.ascontiguousarray(vel, np.float64)
            if p.ndim != 2 or p.shape[1] != 4 or v.shape != p.shape:
                raise ValueError("posm and vel must both be [n, 4]")
            self._check(self._L.nbody_set_state_soa_f64(self._h, _dp(p), _dp(v), p.shape[0]))
        else:
            p = np.ascontiguousarray(posm, np.float32); v = np.ascontiguousarray(vel, np.float32)
            if p.ndim != 2 or p.shape[1] != 4 or v.shape != p.shape:
                raise ValueError("posm and vel must both be [n, 4]")
            self._check(self._L.nbody_set_state_soa(self._h, _fp(p), _fp(v), p.shape[0]))

    # -- hot path --
    def compute_forces(self):
        self._check(self._L.nbody_compute_forces(self._h))

    def step(self, dt=REF_DT, nsteps=1):
        self._check(self._L.nbody_step(self._h, dt, nsteps))

    def step_begin(self):
        """Force pass of the owned bodies (first phase of a step driven by a multi-GPU host)."""
        self._check(self._L.nbody_step_begin(self._h))

    def step_begin_local(self):
        """First go of step_begin: what needs the OWNED slice of the positions only (nbody_step_begin_local)."""
        self._check(self._L.nbody_step_begin_local(self._h))

    def step_begin_remote(self):
        """Second go: the rest of the force pass, once all positions are in (nbody_step_begin_remote)."""
        self._check(self._L.nbody_step_begin_remote(self._h))

    def step_end(self, dt=REF_DT):
        """Kick-drift of the owned bodies (dt <= 0: only store the accelerations)."""
        self._check(self._L.nbody_step_end(self._h, dt))

    def exchange_ranks(self):
        """Number of ranks in the all-to-all between step_begin and step_end (0: no exchange)."""
        n = ctypes.c_int32()
        self._check(self._L.nbody_exchange_info(self._h, None, None, None, ctypes.byref(n)))
        return n.value

    def bind_exchange(self, send, recv):
        """Caller-owned device tensors for the exchange: send [n_total,4], recv [ranks*i_count,4] fp32."""
        self._keep += [send, recv]
        self._check(self._L.nbody_bind_exchange(self._h, ctypes.c_void_p(send.data_ptr()), ctypes.c_void_p(recv.data_ptr())))

    def exchange_read_send(self):
        out = np.empty((self.n_total, 4), np.float64 if self.f64 else np.float32)
        self._check(self._L.nbody_exchange_read_send(self._h, out.ctypes.data))
        return out

    def exchange_write_recv(self, recv):
        r = np.ascontiguousarray(recv, np.float64 if self.f64 else np.float32)
        assert r.shape == (self.exchange_ranks() * self.i_count, 4)
        self._check(self._L.nbody_exchange_write_recv(self._h, r.ctypes.data))

    def set_theta(self, theta):
        """Barnes-Hut opening angle (0 = exact all-pairs; the reference ships 1.0, OctreeSearch.cpp:85)."""
        self._check(self._L.nbody_set_theta(self._h, theta))

    def theta(self):
        """The opening angle in force (a checkpoint brings its own: nbody_load_checkpoint)."""
        v = ctypes.c_float()
        self._check(self._L.nbody_get_theta(self._h, ctypes.byref(v)))
        return v.value

    def set_bh_max_depth(self, levels):
        """The deepest Barnes-Hut tree a frame may build, 42 .. 200 (default 42); a deeper frame is refused (include/nbody.h)."""
        self._check(self._L.nbody_set_bh_max_depth(self._h, int(levels)))

    def bh_max_depth(self):
        v = ctypes.c_int32()
        self._check(self._L.nbody_get_bh_max_depth(self._h, ctypes.byref(v)))
        return v.value

    def bh_stats(self):
        n, l = ctypes.c_int32(), ctypes.c_int32()
        com = np.zeros(3, np.float32)
        self._check(self._L.nbody_bh_stats(self._h, ctypes.byref(n), ctypes.byref(l), _fp(com)))
        return {"nodes": n.value, "levels": l.value, "root_com": com}

    def bh_leaf_boxes(self):
        """[n,4]: (Origin, Size) of the leaf holding each body in the last Barnes-Hut tree."""
        out = np.empty((self.n_total, 4), np.float32)
        self._check(self._L.nbody_bh_leaf_boxes(self._h, _fp(out), 16))
        return out

    def bh_leaf_order(self):
        """order[k] = the body in the k-th occupied leaf of a depth-first walk (children 0..7) of the last tree: the order in
        which the reference's DrawOctreeBoxes draws (OctreeSearch.cpp:36-45)."""
        out = np.empty(self.n_total, np.int32)
        self._check(self._L.nbody_bh_leaf_order(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out

    # -- the field at points that are not bodies --
    def field_at(self, points):
        """Acceleration the bodies exert on a massless point, for every row of `points` (nbody_field_at): [n,3] float32.  points: an
        [n,3] (or [n,>=3]) float32 array with any row stride — e.g. the Position field of a PARTICLE_DTYPE array, read in place —
        or anything np.asarray turns into one.  theta > 0: the walk of the last tree built (include/nbody.h)."""
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] < 3:
            raise ValueError("field_at: points must be [n, >= 3]")
        p = p[:, :3]
        if p.dtype != np.float32 or p.shape[0] < 2 or p.strides[1] != 4 or p.strides[0] < 12:
            p = np.ascontiguousarray(p, np.float32)
        out = np.empty((p.shape[0], 3), np.float32)
        self._check(self._L.nbody_field_at(self._h, p.ctypes.data, max(p.strides[0], 12), p.shape[0], out.ctypes.data, 12))
        return out

    # -- the potential --
    def potential_at(self, points):
        """The bodies' gravitational potential at every row of `points` (nbody_potential_at): [n] float32.  points: as for field_at.
        theta > 0: the walk of the last tree built (include/nbody.h)."""
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] < 3:
            raise ValueError("potential_at: points must be [n, >= 3]")
        p = p[:, :3]
        if p.dtype != np.float32 or p.shape[0] < 2 or p.strides[1] != 4 or p.strides[0] < 12:
            p = np.ascontiguousarray(p, np.float32)
        out = np.empty(p.shape[0], np.float32)
        self._check(self._L.nbody_potential_at(self._h, p.ctypes.data, max(p.strides[0], 12), p.shape[0], out.ctypes.data, 4))
        return out

    def potentials(self):
        """Every body's potential from all other bodies at the current positions (nbody_get_potentials): [n_total] float32.
        theta > 0: builds the tree of the current positions first — side effects as after compute_forces()."""
        out = np.empty(self.n_total, np.float32)
        self._check(self._L.nbody_get_potentials(self._h, out.ctypes.data, 4))
        return out

    def energy_fast(self):
        """(ke, pe) from the per-body potentials (nbody_energy_fast): at theta > 0 about one force pass instead of all pairs.
        Side effects as potentials()."""
        ke, pe = ctypes.c_double(), ctypes.c_double()
        self._check(self._L.nbody_energy_fast(self._h, ctypes.byref(ke), ctypes.byref(pe)))
        return ke.value, pe.value

    # -- the tidal tensor --
    def tidal_at(self, points):
        """The bodies' tidal tensor T_ab = d a_a / d x_b at every row of `points` (nbody_tidal_at): [n,6] float32 — xx, yy, zz, xy, xz,
        yz.  points: as for field_at.  theta > 0: the walk of the last tree built (include/nbody.h)."""
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] < 3:
            raise ValueError("tidal_at: points must be [n, >= 3]")
        p = p[:, :3]
        if p.dtype != np.float32 or p.shape[0] < 2 or p.strides[1] != 4 or p.strides[0] < 12:
            p = np.ascontiguousarray(p, np.float32)
        out = np.empty((p.shape[0], 6), np.float32)
        self._check(self._L.nbody_tidal_at(self._h, p.ctypes.data, max(p.strides[0], 12), p.shape[0], out.ctypes.data, 24))
        return out

    def tidal(self):
        """Every body's tidal tensor from all other bodies at the current positions (nbody_get_tidal): [n_total,6] float32.
        theta > 0: builds the tree of the current positions first — side effects as after compute_forces()."""
        out = np.empty((self.n_total, 6), np.float32)
        self._check(self._L.nbody_get_tidal(self._h, out.ctypes.data, 24))
        return out

    def tidal_time(self):
        """(t_min, body): the smallest tidal time scale ||T_i||_F^(-1/2) over the bodies and the body that attains it
        (nbody_tidal_time).  Side effects as tidal()."""
        t, body = ctypes.c_double(), ctypes.c_int32()
        self._check(self._L.nbody_tidal_time(self._h, ctypes.byref(t), ctypes.byref(body)))
        return t.value, body.value

    # -- the jerk --
    def jerk_at(self, points, vel=None):
        """(acc, jerk): the bodies' acceleration and its time derivative j = da/dt at every row of `points` moving with `vel`
        (nbody_jerk_at): two [n,3] float32 arrays.  points, vel: as for field_at; vel None = at rest (the bits an array of zeros gives).
        The pair sum over all bodies at EVERY theta — no tree is read or built, nothing a getter shows changes, and at theta > 0 `acc` is
        not the monopole walk's.  The bodies' velocities are the stored ones: after step() the staggered v_(n+1/2).  eps == 0: a point
        exactly on a body drops that pair from both sums; eps > 0: it feels G m w / eps^3 in the jerk, nothing in acc.  fp32-state
        contexts (f32, f32_kahan) on one device owning all bodies; fp64, slice and multi-device contexts: ERR_UNSUPPORTED."""
        def rows(a, what):
            a = np.asarray(a)
            if a.ndim != 2 or a.shape[1] < 3:
                raise ValueError(f"jerk_at: {what} must be [n, >= 3]")
            a = a[:, :3]
            if a.dtype != np.float32 or a.shape[0] < 2 or a.strides[1] != 4 or a.strides[0] < 12:
                a = np.ascontiguousarray(a, np.float32)
            return a
        p = rows(points, "points")
        v = None if vel is None else rows(vel, "vel")
        if v is not None and v.shape != p.shape:
            raise ValueError("jerk_at: points and vel differ in shape")
        acc = np.empty((p.shape[0], 3), np.float32)
        jerk = np.empty((p.shape[0], 3), np.float32)
        self._check(self._L.nbody_jerk_at(self._h, p.ctypes.data, max(p.strides[0], 12), None if v is None else v.ctypes.data,
                                          12 if v is None else max(v.strides[0], 12), p.shape[0], acc.ctypes.data, 12, jerk.ctypes.data, 12))
        return acc, jerk

    def jerk(self, dtype=np.float32):
        """(acc, jerk): every body's acceleration and jerk from all OTHER bodies (itself left out by index; bodies on the same point are
        skipped when eps == 0, felt when eps > 0) at the current positions and the stored velocities — after step() the staggered
        v_(n+1/2) — as two [n_total,3] arrays (nbody_get_jerk / nbody_get_jerk_f64).  dtype np.float64: the unrounded fp64 results (the
        fp64 fold on fp32-state contexts, the fp64 sums on fp64 contexts); np.float32: those rounded once.  The pair sum at EVERY theta,
        as jerk_at; all three precisions on one device owning all bodies; slice and multi-device contexts: ERR_UNSUPPORTED."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("jerk: dtype must be float32 or float64")
        acc = np.empty((self.n_total, 3), dt)
        jerk = np.empty((self.n_total, 3), dt)
        f = self._L.nbody_get_jerk if dt.itemsize == 4 else self._L.nbody_get_jerk_f64
        self._check(f(self._h, acc.ctypes.data, 3 * dt.itemsize, jerk.ctypes.data, 3 * dt.itemsize))
        return acc, jerk

    def jerk_time(self):
        """(t_min, body): the smallest |a_i| / |j_i| over the bodies, from the unrounded vectors of jerk(np.float64), and the lowest
        body index that attains it (nbody_jerk_time); +inf for a single body.  Contexts and side effects (none) as jerk()."""
        t, body = ctypes.c_double(), ctypes.c_int32()
        self._check(self._L.nbody_jerk_time(self._h, ctypes.byref(t), ctypes.byref(body)))
        return t.value, body.value

    # -- fourth-order Hermite stepping (fp64 contexts) --
    def hermite_step(self, dt, nsteps=1):
        """nsteps shared steps of length dt of the fourth-order Hermite predictor-corrector (nbody_hermite_step): one fp64 jerk pass
        per step once the derivatives are cached.  The stored velocities are taken as SYNCHRONISED with the positions — step() leaves
        them staggered.  precision="f64" contexts on one device owning all bodies; everything else: ERR_UNSUPPORTED.  dt <= 0: no-op."""
        self._check(self._L.nbody_hermite_step(self._h, float(dt), int(nsteps)))

    def hermite_timescale(self):
        """(t, body, kind): the shared step's time scale and the body that sets it (nbody_hermite_timescale).  kind 1: Aarseth's
        criterion from the cached a, j, a2, a3 (a step has been taken); kind 0: jerk_time()'s |a| / |j| (none has)."""
        t, body, kind = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.nbody_hermite_timescale(self._h, ctypes.byref(t), ctypes.byref(body), ctypes.byref(kind)))
        return t.value, body.value, kind.value

    def hermite_advance(self, t_span, eta=0.02, eta_start=0.01, dt_max=float("inf"), max_steps=2 ** 31):
        """(t_done, steps): shared adaptive Hermite steps, dt = min(dt_max, sqrt(eta) t) — eta_start t for a step without cached
        derivatives —, until t_span has passed (t_done == t_span exactly) or max_steps have been taken (nbody_hermite_advance)."""
        t, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self._L.nbody_hermite_advance(self._h, float(t_span), float(eta), float(eta_start), float(dt_max), int(max_steps),
                                                  ctypes.byref(t), ctypes.byref(n)))
        return t.value, n.value

    def hermite_state(self):
        """(a, j, a2, a3): the cached derivatives of the stored state, four [n_total,3] float64 arrays (nbody_hermite_get); a2 and a3
        are zeros until a step has been taken.  ERR_STATE while nothing is cached for the stored state."""
        out = np.empty((self.n_total, 12), np.float64)
        self._check(self._L.nbody_hermite_get(self._h, out.ctypes.data, 96))
        return tuple(np.ascontiguousarray(out[:, 3 * k:3 * k + 3]) for k in range(4))

    def hermite_restart(self):
        """Forget the cached derivatives: the next Hermite call starts from the stored (x, v) alone, as a resumed run does
        (nbody_hermite_restart)."""
        self._check(self._L.nbody_hermite_restart(self._h))

    def hermite_block_begin(self, dt_max, levels, eta=0.02, eta_start=0.01, level_in=None):
        """Start a session of Hermite BLOCK time steps at tick 0 (nbody_hermite_block_begin): every body steps by its own
        dt_max 2^-level, level 0 .. levels, and lands on every multiple of dt_max — a frame end, where the state is synchronised.
        level_in: n_total levels to start from (how a run resumes: checkpoints hold none); None: from eta_start |a| / |j| per body.
        The contexts of hermite_step(); everything else: ERR_UNSUPPORTED."""
        lv = None
        if level_in is not None:
            lv = np.ascontiguousarray(level_in, np.int32)
            if lv.shape != (self.n_total,):
                raise ValueError(f"level_in must hold {self.n_total} levels")
        self._check(self._L.nbody_hermite_block_begin(self._h, float(dt_max), int(levels), float(eta), float(eta_start),
                                                      lv.ctypes.data if lv is not None else None))

    def hermite_block_advance(self, frames=1, max_block_steps=2 ** 62):
        """Block steps until `frames` more frame ends have been reached or max_block_steps have been taken
        (nbody_hermite_block_advance); a stop in mid-frame leaves every body at its own time.  Returns the session's totals since begin as
        a dict: ticks, frames_done, block_steps, body_steps, pairs, floor_hits, level_min, level_max, synchronised."""
        st = _lib.HermiteBlockStats()
        st.struct_size = ctypes.sizeof(st)
        self._check(self._L.nbody_hermite_block_advance(self._h, int(frames), int(max_block_steps), ctypes.byref(st)))
        out = {name: int(getattr(st, name)) for name, _ in st._fields_ if name != "struct_size"}
        out["synchronised"] = bool(out["synchronised"])
        return out

    def hermite_block_state(self):
        """(ticks [n_total] int64, levels [n_total] int32): every body's own time and level (nbody_hermite_block_get)."""
        ticks, level = np.empty(self.n_total, np.int64), np.empty(self.n_total, np.int32)
        self._check(self._L.nbody_hermite_block_get(self._h, ticks.ctypes.data, level.ctypes.data))
        return ticks, level

    # -- the snap and sixth-order Hermite stepping (fp64 contexts) --
    def snap(self, acc_in=None):
        """(acc, jerk, snap): every body's acceleration, jerk and snap s = d^2 a / dt^2 from all OTHER bodies, three [n_total,3] float64
        arrays (nbody_get_snap_f64).  acc_in: the [n_total,3] accelerations the snap's pair term takes differences of; None: the live
        state's own unrounded accelerations, from one fp64 jerk pass first — the result is then the physical snap of the stored state.
        acc and jerk equal jerk(np.float64) in every bit whatever acc_in holds.  precision="f64" contexts on one device owning all bodies;
        everything else: ERR_UNSUPPORTED.  Changes nothing a getter shows and leaves both Hermite caches alone."""
        ain = None
        if acc_in is not None:
            ain = np.ascontiguousarray(acc_in, np.float64)
            if ain.shape != (self.n_total, 3):
                raise ValueError(f"snap: acc_in must be [{self.n_total},3]")
        out = [np.empty((self.n_total, 3), np.float64) for _ in range(3)]
        self._check(self._L.nbody_get_snap_f64(self._h, None if ain is None else ain.ctypes.data, 24, out[0].ctypes.data, 24,
                                               out[1].ctypes.data, 24, out[2].ctypes.data, 24))
        return tuple(out)

    def hermite6_step(self, dt, nsteps=1):
        """nsteps shared steps of length dt of the sixth-order Hermite predictor-corrector (nbody_hermite6_step): one fp64 snap pass per
        step once the derivatives are cached.  Contexts, the synchronised-velocities rule and dt <= 0 as hermite_step()."""
        self._check(self._L.nbody_hermite6_step(self._h, float(dt), int(nsteps)))

    def hermite6_timescale(self):
        """(t, body, kind): the sixth-order step's time scale and the body that sets it (nbody_hermite6_timescale).  kind 1: from the
        cached a, j, s, a3, a4, a5, t = ((|a||s| + |j|^2) / (|a3||a5| + |a4|^2))^(1/6); kind 0: jerk_time()'s |a| / |j| (no step taken)."""
        t, body, kind = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.nbody_hermite6_timescale(self._h, ctypes.byref(t), ctypes.byref(body), ctypes.byref(kind)))
        return t.value, body.value, kind.value

    def hermite6_advance(self, t_span, eta=0.5, eta_start=0.01, dt_max=float("inf"), max_steps=2 ** 31):
        """(t_done, steps): shared adaptive sixth-order steps, dt = min(dt_max, eta t) — eta times t itself, NO square root as in
        hermite_advance; eta_start t for a step without cached derivatives —, until t_span has passed (t_done == t_span exactly) or
        max_steps have been taken (nbody_hermite6_advance)."""
        t, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self._L.nbody_hermite6_advance(self._h, float(t_span), float(eta), float(eta_start), float(dt_max), int(max_steps),
                                                   ctypes.byref(t), ctypes.byref(n)))
        return t.value, n.value

    def hermite6_state(self):
        """(a, j, s, a3, a4, a5): the sixth-order cache of the stored state, six [n_total,3] float64 arrays (nbody_hermite6_get); a3, a4
        and a5 are zeros until a step has been taken.  ERR_STATE while nothing is cached for the stored state."""
        out = np.empty((self.n_total, 18), np.float64)
        self._check(self._L.nbody_hermite6_get(self._h, out.ctypes.data, 144))
        return tuple(np.ascontiguousarray(out[:, 3 * k:3 * k + 3]) for k in range(6))

    def hermite6_block_begin(self, dt_max, levels, eta=0.5, eta_start=0.01, level_in=None):
        """Start a session of SIXTH-order Hermite block time steps at tick 0 (nbody_hermite6_block_begin): hermite_block_begin()'s ticks,
        levels and frames around the sixth-order predictor, snap evaluation and corrector.  eta multiplies the sixth-root time scale
        directly, as in hermite6_advance(): 0.3 .. 1 here does what 0.01 .. 0.04 does for hermite_block_begin().  level_in: n_total
        levels to start from; None: from eta_start |a| / |j| per body.  The contexts of hermite6_step(); everything else: ERR_UNSUPPORTED."""
        lv = None
        if level_in is not None:
            lv = np.ascontiguousarray(level_in, np.int32)
            if lv.shape != (self.n_total,):
                raise ValueError(f"level_in must hold {self.n_total} levels")
        self._check(self._L.nbody_hermite6_block_begin(self._h, float(dt_max), int(levels), float(eta), float(eta_start),
                                                       lv.ctypes.data if lv is not None else None))

    def hermite6_block_advance(self, frames=1, max_block_steps=2 ** 62):
        """Sixth-order block steps until `frames` more frame ends have been reached or max_block_steps have been taken
        (nbody_hermite6_block_advance).  Returns the session's totals since begin as hermite_block_advance() does."""
        st = _lib.HermiteBlockStats()
        st.struct_size = ctypes.sizeof(st)
        self._check(self._L.nbody_hermite6_block_advance(self._h, int(frames), int(max_block_steps), ctypes.byref(st)))
        out = {name: int(getattr(st, name)) for name, _ in st._fields_ if name != "struct_size"}
        out["synchronised"] = bool(out["synchronised"])
        return out

    def hermite6_block_state(self):
        """(ticks [n_total] int64, levels [n_total] int32): every body's own time and level (nbody_hermite6_block_get)."""
        ticks, level = np.empty(self.n_total, np.int64), np.empty(self.n_total, np.int32)
        self._check(self._L.nbody_hermite6_block_get(self._h, ticks.ctypes.data, level.ctypes.data))
        return ticks, level

    def set_tracers(self, pos, vel=None):
        """Massless tracers the engine advances with the bodies (nbody_set_tracers).  pos, vel: [n,3] or [n,4] float32 (a 4th column is
        ignored); vel None = at rest; an empty pos removes them.  Replaces any earlier set."""
        def four(a):
            a = np.asarray(a, np.float32)
            a = a.reshape(-1, a.shape[-1] if a.ndim == 2 else 3)
            if a.shape[1] not in (3, 4):
                raise ValueError("set_tracers: [n,3] or [n,4]")
            b = np.zeros((a.shape[0], 4), np.float32)
            b[:, :a.shape[1]] = a
            return b
        p = four(pos)
        v = None if vel is None else four(vel)
        if v is not None and v.shape != p.shape:
            raise ValueError("set_tracers: pos and vel must have the same number of rows")
        self._check(self._L.nbody_set_tracers(self._h, _fp(p), None if v is None else _fp(v), p.shape[0]))

    @property
    def tracer_count(self):
        n = ctypes.c_int32()
        self._check(self._L.nbody_tracer_count(self._h, ctypes.byref(n)))
        return n.value

    def tracers(self):
        """(pos, vel, acc) of the tracers, [n,4] float32 each (nbody_get_tracers; synchronises).  Feeding pos and vel back to
        set_tracers restores them bit for bit."""
        n = self.tracer_count
        p, v, a = (np.zeros((n, 4), np.float32) for _ in range(3))
        self._check(self._L.nbody_get_tracers(self._h, _fp(p), _fp(v), _fp(a)))
        return p, v, a

    # -- fp64 point queries and fp64 tracers on the shared-step Hermite calls (fp64 contexts) --
    @staticmethod
    def _rows64(a, who, what):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError(f"{who}: {what} must be [n, >= 3]")
        return np.ascontiguousarray(a[:, :3], np.float64)

    def jerk_at_f64(self, points, vel=None):
        """(acc, jerk): the bodies' acceleration and jerk at every row of `points` moving with `vel` (nbody_jerk_at_f64): two [n,3]
        float64 arrays, the unrounded fp64 pair sums over ALL bodies from the live positions and velocities.  vel None = at rest (the
        bits an array of zeros gives).  No pair is dropped by index: a body asked about at its own (x, v) gets jerk(np.float64)'s row in
        every bit.  eps == 0: a point exactly on a body drops that pair; eps > 0: it feels G m w / eps^3 in the jerk, nothing in acc.
        precision="f64" contexts on one device owning all bodies; everything else: ERR_UNSUPPORTED.  Changes nothing a getter shows."""
        p = self._rows64(points, "jerk_at_f64", "points")
        v = None if vel is None else self._rows64(vel, "jerk_at_f64", "vel")
        if v is not None and v.shape != p.shape:
            raise ValueError("jerk_at_f64: points and vel differ in shape")
        acc = np.empty((p.shape[0], 3), np.float64)
        jerk = np.empty((p.shape[0], 3), np.float64)
        self._check(self._L.nbody_jerk_at_f64(self._h, p.ctypes.data, 24, None if v is None else v.ctypes.data, 24, p.shape[0],
                                              acc.ctypes.data, 24, jerk.ctypes.data, 24))
        return acc, jerk

    # -- the fp64 potential, tidal tensor and snap at points (fp64 contexts) --
    def potential_at_f64(self, points):
        """The bodies' gravitational potential phi = -sum G m / s at every row of `points` (nbody_potential_at_f64): [n] float64, the
        unrounded fp64 pair sums over ALL bodies from the live positions.  No pair is dropped by index: with eps == 0 a body asked about
        at its own position gets potentials_f64()'s row in every bit and a point exactly on a body drops that pair; with eps > 0 such a
        point feels -G m / eps of it.  precision="f64" contexts on one device owning all bodies; everything else: ERR_UNSUPPORTED.
        Changes nothing a getter shows and leaves the Hermite caches, the fp64 tracers and any block session alone."""
        p = self._rows64(points, "potential_at_f64", "points")
        out = np.empty(p.shape[0], np.float64)
        self._check(self._L.nbody_potential_at_f64(self._h, p.ctypes.data, 24, p.shape[0], out.ctypes.data, 8))
        return out

    def potentials_f64(self):
        """Every body's potential from all OTHER bodies (itself left out by index; bodies on the same point are skipped when eps == 0,
        felt when eps > 0) at the current positions (nbody_get_potentials_f64): [n_total] float64, unrounded.  Contexts and side
        effects (none) as potential_at_f64()."""
        out = np.empty(self.n_total, np.float64)
        self._check(self._L.nbody_get_potentials_f64(self._h, out.ctypes.data, 8))
        return out

    def tidal_at_f64(self, points):
        """The bodies' tidal tensor T_ab = d a_a / d x_b at every row of `points` (nbody_tidal_at_f64): [n,6] float64 — xx, yy, zz, xy,
        xz, yz —, the unrounded fp64 pair sums over ALL bodies.  No pair is dropped by index: with eps == 0 a point exactly on a body
        drops that pair; with eps > 0 it feels -G m / eps^3 of it on the diagonal.  Contexts and side effects (none) as
        potential_at_f64()."""
        p = self._rows64(points, "tidal_at_f64", "points")
        out = np.empty((p.shape[0], 6), np.float64)
        self._check(self._L.nbody_tidal_at_f64(self._h, p.ctypes.data, 24, p.shape[0], out.ctypes.data, 48))
        return out

    def tidal_f64(self):
        """Every body's tidal tensor from all OTHER bodies at the current positions (nbody_get_tidal_f64): [n_total,6] float64,
        unrounded.  Contexts and side effects (none) as potential_at_f64()."""
        out = np.empty((self.n_total, 6), np.float64)
        self._check(self._L.nbody_get_tidal_f64(self._h, out.ctypes.data, 48))
        return out

    def tidal_time_f64(self):
        """(t_min, body): the smallest tidal time scale ||T_i||_F^(-1/2) over the bodies, from the tensors of tidal_f64(), and the lowest
        body index that attains it (nbody_tidal_time_f64: tidal_time()'s rule); +inf for a single body.  Contexts and side effects
        (none) as potential_at_f64()."""
        t, body = ctypes.c_double(), ctypes.c_int32()
        self._check(self._L.nbody_tidal_time_f64(self._h, ctypes.byref(t), ctypes.byref(body)))
        return t.value, body.value

    def snap_at_f64(self, points, vel=None):
        """(acc, jerk, snap): the bodies' acceleration, jerk and physical snap s = d^2 a / dt^2 at every row of `points` moving with
        `vel` (nbody_snap_at_f64): three [n,3] float64 arrays.  vel None = at rest (the bits an array of zeros gives).  Three passes: the
        bodies' own accelerations (as snap() with acc_in None), the points' own, then the point snap pass; a body asked about at its
        own (x, v) gets snap()'s row in every bit.  Contexts and side effects (none) as potential_at_f64()."""
        p = self._rows64(points, "snap_at_f64", "points")
        v = None if vel is None else self._rows64(vel, "snap_at_f64", "vel")
        if v is not None and v.shape != p.shape:
            raise ValueError("snap_at_f64: points and vel differ in shape")
        out = [np.empty((p.shape[0], 3), np.float64) for _ in range(3)]
        self._check(self._L.nbody_snap_at_f64(self._h, p.ctypes.data, 24, None if v is None else v.ctypes.data, 24, p.shape[0],
                                              out[0].ctypes.data, 24, out[1].ctypes.data, 24, out[2].ctypes.data, 24))
        return tuple(out)

    # -- the fp64 pair census: nearest body, most-bound partner, binaries (fp64 contexts) --
    def nearest_f64(self):
        """(index, d2): every body's nearest OTHER body and the squared distance to it (nbody_get_nearest_f64): [n_total] int32 and
        float64.  d2 = fma(dx, dx, fma(dy, dy, dz dz)) is never softened; the smallest under strict <, the lowest index among equals; a
        coincident body (d2 == 0) is the nearest; zero-mass bodies count; a body whose d2 is NaN or +inf is never chosen.  Nobody to
        choose (a single body): -1 and +inf.  d2[i] == d2[index[i]] in every bit where the two are mutual.  precision="f64" contexts on
        one device owning all bodies; everything else: ERR_UNSUPPORTED.  One pass; changes nothing a getter shows and leaves the Hermite
        caches, the fp64 tracers and any block session alone."""
        index, d2 = np.empty(self.n_total, np.int32), np.empty(self.n_total, np.float64)
        self._check(self._L.nbody_get_nearest_f64(self._h, index.ctypes.data, d2.ctypes.data))
        return index, d2

    def nearest_at_f64(self, points):
        """(index, d2): the body nearest to every row of `points` (nbody_nearest_at_f64): [n] int32 and float64.  No body is dropped by
        index: a point exactly on a body gets that body at d2 = 0.  A row depends on its point and the bodies alone.  Rules, contexts
        and side effects (none) as nearest_f64()."""
        p = self._rows64(points, "nearest_at_f64", "points")
        index, d2 = np.empty(p.shape[0], np.int32), np.empty(p.shape[0], np.float64)
        self._check(self._L.nbody_nearest_at_f64(self._h, p.ctypes.data, 24, p.shape[0], index.ctypes.data, d2.ctypes.data))
        return index, d2

    def closest_pair_f64(self):
        """(i, j, d2): the closest pair of bodies, i < j (nbody_closest_pair_f64): the smallest d2 of nearest_f64() and the lowest body
        that attains it, reduced on the device in a fixed order; (-1, -1, +inf) when there is none."""
        i, j, d2 = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        self._check(self._L.nbody_closest_pair_f64(self._h, ctypes.byref(i), ctypes.byref(j), ctypes.byref(d2)))
        return i.value, j.value, d2.value

    def partners_f64(self):
        """(index, energy, d2): every body's most-bound partner — the OTHER body j with the smallest specific orbital energy
        e = 0.5 |v_j - v_i|^2 - G (m_i + m_j) / sqrt(d2 + eps^2) of the pair, under the context's own pair law —, that energy and the
        pair's unsoftened d2 (nbody_get_partners_f64): [n_total] int32, float64, float64.  Strict <, the lowest index among equals; with
        eps == 0 a coincident body contributes 0.5 |w|^2 alone; a candidate whose e is NaN or whose d2 is not finite is never chosen;
        nobody to choose: -1, +inf, +inf.  e is symmetric in every bit, so index[index[i]] == i marks a mutual pair; e < 0: bound.
        Contexts and side effects (none) as nearest_f64()."""
        index, e, d2 = np.empty(self.n_total, np.int32), np.empty(self.n_total, np.float64), np.empty(self.n_total, np.float64)
        self._check(self._L.nbody_get_partners_f64(self._h, index.ctypes.data, e.ctypes.data, d2.ctypes.data))
        return index, e, d2

    def partner_at_f64(self, points, vel=None):
        """(index, energy, d2): the body every row of `points`, moving with `vel`, is most bound to as a massless point: the smallest
        e = 0.5 |v_j - v|^2 - G m_j / sqrt(d2 + eps^2) (nbody_partner_at_f64).  vel None = at rest (the bits an array of zeros gives).
        No body is dropped by index.  Rules, contexts and side effects (none) as partners_f64()."""
        p = self._rows64(points, "partner_at_f64", "points")
        v = None if vel is None else self._rows64(vel, "partner_at_f64", "vel")
        if v is not None and v.shape != p.shape:
            raise ValueError("partner_at_f64: points and vel differ in shape")
        index, e, d2 = np.empty(p.shape[0], np.int32), np.empty(p.shape[0], np.float64), np.empty(p.shape[0], np.float64)
        self._check(self._L.nbody_partner_at_f64(self._h, p.ctypes.data, 24, None if v is None else v.ctypes.data, 24, p.shape[0],
                                                 index.ctypes.data, e.ctypes.data, d2.ctypes.data))
        return index, e, d2

    def hardest_pair_f64(self):
        """(i, j, energy, d2): the pair with the lowest specific orbital energy, i < j (nbody_hardest_pair_f64): the smallest e of
        partners_f64() and the lowest body that attains it, reduced on the device in a fixed order; (-1, -1, +inf, +inf) when there
        is none."""
        i, j, e, d2 = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double(), ctypes.c_double()
        self._check(self._L.nbody_hardest_pair_f64(self._h, ctypes.byref(i), ctypes.byref(j), ctypes.byref(e), ctypes.byref(d2)))
        return i.value, j.value, e.value, d2.value

    def pair_time_f64(self):
        """(t_min, i, j): the free-fall scale sqrt(d2 sqrt(d2) / (G (m_i + m_j))) of the closest pair (nbody_pair_time_f64) — what a
        host compares with dt_max 2^-levels; +inf for a massless or missing pair."""
        t, i, j = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.nbody_pair_time_f64(self._h, ctypes.byref(t), ctypes.byref(i), ctypes.byref(j)))
        return t.value, i.value, j.value

    BINARY_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("energy", np.float64), ("a", np.float64), ("ecc", np.float64)])

    def binaries_f64(self):
        """The bound mutual pairs: a structured array (i, j, energy, a, ecc), i < j, of the pairs with partner[partner[i]] == i and
        energy < 0 from partners_f64().  a = -G (m_i + m_j) / (2 energy); ecc = |(w x (r x w)) / (G (m_i + m_j)) - r / |r|| from the
        relative state r = x_j - x_i, w = v_j - v_i of state(np.float64), in numpy.  Keplerian elements for eps == 0: with softening
        the energy is the softened pair law's and a, ecc only approximate the orbit.  Python only; one pass and one state read."""
        index, energy, _ = self.partners_f64()
        i = np.arange(self.n_total, dtype=np.int32)
        ok = index >= 0
        mutual = np.zeros(self.n_total, bool)
        mutual[ok] = (index[index[ok]] == i[ok]) & (i[ok] < index[ok]) & (energy[ok] < 0.0)
        out = np.zeros(int(mutual.sum()), self.BINARY_DTYPE)
        out["i"], out["j"], out["energy"] = i[mutual], index[mutual], energy[mutual]
        if out.size:
            posm, vel, _ = self.state(np.float64)
            r = posm[out["j"], :3] - posm[out["i"], :3]
            w = vel[out["j"], :3] - vel[out["i"], :3]
            mu = self._G * (posm[out["i"], 3] + posm[out["j"], 3])
            out["a"] = -mu / (2.0 * out["energy"])
            ev = np.cross(w, np.cross(r, w)) / mu[:, None] - r / np.linalg.norm(r, axis=1)[:, None]
            out["ecc"] = np.linalg.norm(ev, axis=1)
        return out

    # -- the fp64 neighbour census: k nearest bodies, local density, density centre and core radius (fp64 contexts) --
    @staticmethod
    def _k(k):
        """(k, the columns to allocate): a k out of range is the library's to refuse (ERR_INVALID), before it writes anything"""
        k = int(k)
        return k, min(max(k, 1), _lib.NEIGHBOURS_MAX)

    def neighbours_f64(self, k=6):
        """(index, d2): every body's k nearest OTHER bodies and the squared distances to them (nbody_get_neighbours_f64): [n_total, k]
        int32 and float64, each row sorted ascending in lexicographic (d2, index) order.  d2 = fma(dx, dx, fma(dy, dy, dz dz)) is never
        softened; strict <, the lowest index among equals; coincident bodies (d2 == 0) come first; zero-mass bodies count; a body whose
        d2 is NaN or +inf is never listed.  Slots with nobody to list (n_total <= k): -1 and +inf.  k = 1 .. 8; the answer for k is the
        first k columns of the answer for any larger k in every byte, and k = 1 is nearest_f64()'s.  precision="f64" contexts on one
        device owning all bodies; everything else: ERR_UNSUPPORTED.  One pass; changes nothing a getter shows and leaves the Hermite
        caches, the fp64 tracers and any block session alone."""
        k, cols = self._k(k)
        index, d2 = np.empty((self.n_total, cols), np.int32), np.empty((self.n_total, cols), np.float64)
        self._check(self._L.nbody_get_neighbours_f64(self._h, k, index.ctypes.data, d2.ctypes.data))
        return index, d2

    def neighbours_at_f64(self, points, k=6):
        """(index, d2): the k bodies nearest to every row of `points` (nbody_neighbours_at_f64): [n, k] int32 and float64.  No body is
        dropped by index: a point exactly on a body gets that body at d2 = 0.  A row depends on its point and the bodies alone.  Rules,
        contexts and side effects (none) as neighbours_f64()."""
        k, cols = self._k(k)
        p = self._rows64(points, "neighbours_at_f64", "points")
        index, d2 = np.empty((p.shape[0], cols), np.int32), np.empty((p.shape[0], cols), np.float64)
        self._check(self._L.nbody_neighbours_at_f64(self._h, p.ctypes.data, 24, p.shape[0], k, index.ctypes.data, d2.ctypes.data))
        return index, d2

    def density_f64(self, k=6):
        """(rho, rk2): every body's local density after Casertano & Hut (1985) and the squared distance of its k-th neighbour
        (nbody_get_density_f64): [n_total] float64 each.  rho = msum / ((4 pi / 3) (rk2 sqrt(rk2))) with msum the raw masses of the
        k - 1 nearest added in neighbour order — the k-th sets the sphere and is left out of the mass, as is the body itself; every
        bracket one rounded fp64 operation, so numpy reproduces rho in every bit from neighbours_f64(k) and the masses.  k = 2 .. 8.
        n_total <= k: rho = 0, rk2 = +inf; a NaN quotient becomes 0; rk2 == 0 with msum > 0 gives +inf.  Contexts and side effects
        (none) as neighbours_f64()."""
        k, _ = self._k(k)
        rho, rk2 = np.empty(self.n_total, np.float64), np.empty(self.n_total, np.float64)
        self._check(self._L.nbody_get_density_f64(self._h, k, rho.ctypes.data, rk2.ctypes.data))
        return rho, rk2

    def core_f64(self, k=6):
        """The density centre and core radius in NBODY6's convention (nbody_density_centre_f64): a CoreResult.  With w = rho of
        density_f64(k) where 0 < rho < +inf, else 0: centre = sum w x / sum w, core_radius = sqrt(sum w^2 |x - centre|^2 / sum w^2), both
        sums on the device in a fixed order (the same bits every run); rho_sum = sum w, rho2_sum = sum w^2; rho_max, densest: the largest
        w and the lowest body that attains it; used: the bodies with w > 0.  used == 0: centre and core_radius NaN, densest -1,
        rho_max 0.  core_mass, core_count (Python only): the mass and the bodies within core_radius of the centre, from mass_within()
        (0 and 0 when used == 0).  One pass; contexts and side effects (none) as neighbours_f64()."""
        k, _ = self._k(k)
        c = _lib.Core()
        c.struct_size = ctypes.sizeof(c)
        self._check(self._L.nbody_density_centre_f64(self._h, k, ctypes.byref(c)))
        centre = np.array(list(c.centre), np.float64)
        mass, count = 0.0, 0
        if c.used > 0:
            ms, ns = self.mass_within(centre, [c.core_radius])
            mass, count = float(ms[0]), int(ns[0])
        return CoreResult(k=c.k, used=c.used, densest=c.densest, rho_max=c.rho_max, centre=centre, core_radius=c.core_radius,
                          rho_sum=c.rho_sum, rho2_sum=c.rho2_sum, core_mass=mass, core_count=count)

    # -- the fp64 radial census: the bodies in radial order, the cumulative mass, Lagrangian radii (fp64 contexts) --
    @staticmethod
    def _centre(centre, who):
        c = np.ascontiguousarray(np.asarray(centre, np.float64).reshape(-1))
        if c.shape != (3,):
            raise ValueError(f"{who}: centre must be 3 numbers")
        return c

    def radial_order_f64(self, centre):
        """(order, d2, mass_cum, n_finite): the bodies in radial order about `centre` (nbody_radial_order_f64): int32[n_total],
        float64[n_total], float64[n_total] and an int.  d2 = (dx*dx + dy*dy) + dz*dz without contraction — mass_within()'s; the order
        is ascending in lexicographic (d2, index): np.argsort(d2, kind="stable"), finite d2 first, then +inf, then NaN (n_finite: the
        finite ones).  mass_cum adds the raw masses in that order in blocks of 256, left to right inside a block, then the blocks'
        offsets in order (include/nbody.h: numpy reproduces every bit); a non-finite d2 adds nothing.  precision="f64" contexts on one
        device owning all bodies; everything else: ERR_UNSUPPORTED.  A sort on the device, no pair pass; changes nothing a getter shows
        and leaves the Hermite caches, the fp64 tracers and any block session alone."""
        c = self._centre(centre, "radial_order_f64")
        order, d2, cum = np.empty(self.n_total, np.int32), np.empty(self.n_total, np.float64), np.empty(self.n_total, np.float64)
        nf = ctypes.c_int32()
        self._check(self._L.nbody_radial_order_f64(self._h, _dp(c), order.ctypes.data, d2.ctypes.data, cum.ctypes.data, ctypes.byref(nf)))
        return order, d2, cum, nf.value

    def _default_centre(self, k):
        core = self.core_f64(k)
        return core.centre if core.used > 0 else np.array(self.moments().com, np.float64)

    def lagrange_f64(self, fractions=LAGRANGE_FRACTIONS, centre=None, k=6):
        """The Lagrangian radii about `centre` (nbody_lagrange_radii_f64): a LagrangeResult — the centre used, total_mass and, per
        fraction f (each in (0, 1], at most 64, any order), the row (fraction, r2, radius, mass, body, count): the FIRST position p of
        radial_order_f64() with mass_cum[p] >= f * total_mass, r2 = d2[p] (exact: compares with mass_within()'s threshold), radius =
        sqrt(r2), mass = mass_cum[p], body = order[p], count = p + 1.  Where total_mass is not > 0: (f, NaN, NaN, NaN, -1, 0).
        centre=None: core_f64(k).centre, or — when that has used == 0 — the centre of mass from moments().  Contexts and side effects
        (none) as radial_order_f64()."""
        f = np.ascontiguousarray(np.asarray(fractions, np.float64).reshape(-1))
        c = self._default_centre(k) if centre is None else self._centre(centre, "lagrange_f64")
        rows = (_lib.Lagrange * min(max(f.shape[0], 1), _lib.LAGRANGE_MAX))()
        total = ctypes.c_double()
        self._check(self._L.nbody_lagrange_radii_f64(self._h, _dp(c), _dp(f), f.shape[0], rows, ctypes.byref(total)))
        a = np.frombuffer(rows, np.dtype([("fraction", "<f8"), ("r2", "<f8"), ("radius", "<f8"), ("mass", "<f8"), ("body", "<i4"),
                                          ("count", "<i4")]))
        return LagrangeResult(centre=c, total_mass=total.value, **{n: a[n].copy() for n in a.dtype.names})

    def radial_profile_f64(self, fractions=LAGRANGE_FRACTIONS, centre=None, vcentre=None, k=6):
        """The shells between consecutive Lagrangian positions: a RadialProfileResult with, per fraction (strictly increasing), the
        shell that ENDS at its row — count, mass, r_in, r_out, density, v_r, sigma_r2, sigma_t2, beta; the formulas are
        radial_profile()'s, in numpy on radial_order_f64() and state(np.float64):
            density = mass / ((4 pi / 3) (r_out^3 - r_in^3));  v_r = <u . e>;  sigma_r2 = <(u . e - v_r)^2>;
            sigma_t2 = <|u|^2 - (u . e)^2>;  beta = 1 - sigma_t2 / (2 sigma_r2)
        with <.> the mass-weighted mean over the shell, e the unit vector from the centre, u = v - vcentre; vcentre=None: the shell's
        own mass-weighted mean velocity.  centre=None as lagrange_f64().  Python only; one sort and one state read."""
        f = np.asarray(fractions, np.float64).reshape(-1)
        if f.shape[0] > 1 and not np.all(np.diff(f) > 0.0):
            raise ValueError("radial_profile_f64: fractions must be strictly increasing")
        c = self._default_centre(k) if centre is None else self._centre(centre, "radial_profile_f64")
        lag = self.lagrange_f64(f, c)
        order, _, _, _ = self.radial_order_f64(c)
        posm, vel, _ = self.state(np.float64)
        count, cols = radial_profile(order, posm, vel, c, lag.count, lag.radius, vcentre)
        return RadialProfileResult(centre=c, total_mass=lag.total_mass, fraction=lag.fraction, count=count, **cols)

    # -- the fp64 group census: radius counts and friends-of-friends groups (fp64 contexts) --
    def radius_counts_f64(self, radius):
        """count: the number of OTHER bodies within `radius` of every body (nbody_get_radius_counts_f64): int32[n_total].  Body j is
        counted iff d2 <= radius * radius with d2 = (dx*dx + dy*dy) + dz*dz without contraction — mass_within()'s expression; a NaN or
        +inf d2 never is; zero-mass bodies count.  radius finite and >= 0 with a finite square, else ERR_INVALID.  precision="f64"
        contexts on one device owning all bodies; everything else: ERR_UNSUPPORTED.  One pass; changes nothing a getter shows and
        leaves the Hermite caches, the fp64 tracers and any block session alone."""
        count = np.empty(self.n_total, np.int32)
        self._check(self._L.nbody_get_radius_counts_f64(self._h, float(radius), count.ctypes.data))
        return count

    def radius_counts_at_f64(self, points, radius):
        """count: the number of bodies within `radius` of every row of `points` (nbody_radius_counts_at_f64): int32[n].  No body is
        dropped by index: a point exactly on a body counts that body, and one point c gives mass_within(c, [radius])'s count exactly.
        Rules, contexts and side effects (none) as radius_counts_f64()."""
        p = self._rows64(points, "radius_counts_at_f64", "points")
        count = np.empty(p.shape[0], np.int32)
        self._check(self._L.nbody_radius_counts_at_f64(self._h, p.ctypes.data, 24, p.shape[0], float(radius), count.ctypes.data))
        return count

    def groups_f64(self, radius):
        """The friends-of-friends groups at linking length `radius` (nbody_get_groups_f64): a GroupsResult (label, members, degree,
        summary).  Bodies i != j are linked iff d2 <= radius * radius (d2 as radius_counts_f64()); degree[i] = the bodies linked to
        i; label[i] = the lowest index of i's connected component; members[i] = its size: int32[n_total] each.  summary: groups (the
        components, singles included), multiples (those of two or more), largest (the label of the one with the most members, the
        lowest among ties), largest_members, rounds (the pair passes the device took), links (sum of degree / 2).  Everything but
        rounds is a function of the positions and the radius alone.  Contexts and side effects (none) as radius_counts_f64()."""
        label, members, degree = (np.empty(self.n_total, np.int32) for _ in range(3))
        s = _lib.Groups()
        self._check(self._L.nbody_get_groups_f64(self._h, float(radius), label.ctypes.data, members.ctypes.data, degree.ctypes.data,
                                                 ctypes.byref(s)))
        return GroupsResult(label, members, degree, GroupsSummary(*(int(getattr(s, f)) for f in GroupsSummary._fields)))

    def group_table_f64(self, radius, min_members=2):
        """One row per group of at least `min_members` bodies, in label order: a structured array (label, count, mass, com, velocity,
        r_rms, sigma) from groups_f64(radius) and state(np.float64), in numpy.  Over the bodies i of a group:
            mass = M = sum m_i;  com = sum m_i x_i / M;  velocity = sum m_i v_i / M
            r_rms = sqrt(sum m_i |x_i - com|^2 / M);  sigma = sqrt(sum m_i |v_i - velocity|^2 / M)
        (sigma is the three-dimensional dispersion; a group of zero mass has NaN there).  Python only; the passes of groups_f64() and
        one state read."""
        label = self.groups_f64(radius).label
        posm, vel, _ = self.state(np.float64)
        return group_table(label, posm, vel, min_members)

    # -- the fp64 separation census: pair counts at many radii in one pass (fp64 contexts) --
    def _pair_counts(self, radii, call):
        r = np.ascontiguousarray(radii, np.float64)
        flat = r.reshape(-1)
        count = np.zeros(flat.shape[0], np.int64)
        for lo in range(0, max(flat.shape[0], 1), _lib.PAIR_RADII_MAX):
            part = np.ascontiguousarray(flat[lo:lo + _lib.PAIR_RADII_MAX])
            c = np.zeros(part.shape[0], np.int64)
            self._check(call(_dp(part), part.shape[0], c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            count[lo:lo + part.shape[0]] = c
        return count.reshape(r.shape)

    def pair_counts_f64(self, radii):
        """count: the number of UNORDERED pairs of bodies {i, j}, i != j by index, within each of `radii` (nbody_get_pair_counts_f64):
        an int64 array shaped like radii.  A pair counts iff d2 <= radius * radius with d2 as radius_counts_f64(); coincident bodies
        count at radius 0; a NaN or +inf d2 never counts.  The radii may come in any order and with repeats, each finite and >= 0 with
        a finite square (else ERR_INVALID); any number of them, 64 to a call, 16 distinct ones to an N^2 pass — where one
        radius_counts_f64() pass answers one.  count == groups_f64(r).summary.links == radius_counts_f64(r).sum() // 2 exactly.
        Contexts and side effects (none) as radius_counts_f64()."""
        return self._pair_counts(radii, lambda r, k, c: self._L.nbody_get_pair_counts_f64(self._h, r, k, c))

    def pair_counts_at_f64(self, points, radii):
        """count: the number of (point, body) pairs within each of `radii`, over every row of `points` and every body
        (nbody_pair_counts_at_f64): an int64 array shaped like radii.  No body is dropped by index: a point exactly on a body counts
        that body.  count == radius_counts_at_f64(points, r).sum() exactly; no points: zeros.  Rules, contexts and side effects (none)
        as pair_counts_f64()."""
        p = self._rows64(points, "pair_counts_at_f64", "points")
        return self._pair_counts(radii, lambda r, k, c: self._L.nbody_pair_counts_at_f64(self._h, p.ctypes.data, 24, p.shape[0], r, k, c))

    def pair_histogram_f64(self, edges):
        """The pair-separation histogram: the unordered pairs of bodies whose separation lies in (edges[b], edges[b + 1]] — the LOWER
        edge is open, the upper closed; a pair at separation exactly edges[0] is in no bin — for ascending `edges`:
        int64[len(edges) - 1], the differences of pair_counts_f64(edges) (pair_histogram()), in numpy."""
        e = np.asarray(edges, np.float64).reshape(-1)
        if e.shape[0] < 2 or not np.all(np.diff(e) >= 0.0):
            raise ValueError("pair_histogram_f64: at least two edges, ascending")
        return pair_histogram(e, self.pair_counts_f64(e))

    def correlation_f64(self, edges, randoms):
        """The two-point correlation function of the bodies in the bins of pair_histogram_f64(edges), by the Landy-Szalay estimator
        against the rows of `randoms` ([n_random, >= 3]): a CorrelationResult (xi, dd, dr, rr).  dd: the bodies' pairs per bin
        (pair_histogram_f64); dr: the (random, body) pairs per bin from pair_counts_at_f64(randoms, edges); rr: the randoms' own pairs
        per bin, from a temporary fp64 engine on the same device that holds them.  xi = (DD - 2 DR + RR) / RR with DD = dd / (n (n - 1)
        / 2), DR = dr / (n n_random), RR = rr / (n_random (n_random - 1) / 2) (landy_szalay()); NaN where rr == 0."""
        e = np.asarray(edges, np.float64).reshape(-1)
        if e.shape[0] < 2 or not np.all(np.diff(e) >= 0.0):
            raise ValueError("correlation_f64: at least two edges, ascending")
        r = self._rows64(randoms, "correlation_f64", "randoms")
        if r.shape[0] < 2:
            raise ValueError("correlation_f64: at least two randoms")
        dd = pair_histogram(e, self.pair_counts_f64(e))
        dr = pair_histogram(e, self.pair_counts_at_f64(r, e))
        posm = np.ones((r.shape[0], 4), np.float64)
        posm[:, :3] = r
        with NBodyEngine(r.shape[0], device=self._device, precision="f64") as other:
            other.set_state(posm, np.zeros_like(posm))
            rr = pair_histogram(e, other.pair_counts_f64(e))
        return CorrelationResult(landy_szalay(dd, dr, rr, self.n_total, r.shape[0]), dd, dr, rr)

    # -- the fp64 minimum spanning tree (fp64 contexts) --
    def mst_f64(self):
        """The Euclidean minimum spanning tree of the bodies (nbody_get_mst_f64): an MstResult (i, j, d2, component, summary).  The
        weight of the pair i < j is d2 = (dx*dx + dy*dy) + dz*dz without contraction — groups_f64()'s expression —, an edge only
        where it is finite: bodies with a NaN or infinite coordinate end in components of their own, and the result is a forest.  Edges
        compare by (d2, i, j), a strict total order, so the forest is unique and the same bytes every run.  i, j, d2: the
        summary.edges = n_total - summary.components edges in ascending order of that key; component[n_total]: the lowest index of
        each body's component.  summary: edges, components, rounds (the pair passes the device took, at most ceil(log2 n_total) + 1),
        length (= np.cumsum(np.sqrt(d2))[-1], 0.0 with no edge) and longest_d2 (the last edge's, 0.0 with none).  Contexts and side
        effects (none) as radius_counts_f64()."""
        n = self.n_total
        i, j = (np.empty(max(n - 1, 0), np.int32) for _ in range(2))
        d2 = np.empty(max(n - 1, 0), np.float64)
        component = np.empty(n, np.int32)
        s = _lib.Mst()
        self._check(self._L.nbody_get_mst_f64(self._h, i.ctypes.data, j.ctypes.data, d2.ctypes.data, component.ctypes.data, ctypes.byref(s)))
        summary = MstSummary(int(s.edges), int(s.components), int(s.rounds), float(s.length), float(s.longest_d2))
        return MstResult(i[:summary.edges].copy(), j[:summary.edges].copy(), d2[:summary.edges].copy(), component, summary)

    @staticmethod
    def mst_groups_f64(mst, radius):
        """(label, members) of the friends-of-friends groups at linking length `radius` from an MstResult, in numpy: a union-find over
        the edges with d2 <= radius * radius, the lower root winning.  label[i] = the lowest index of i's group, members[i] = its
        size (int32[n_total] each): byte for byte groups_f64(radius)'s, for any number of radii from one mst_f64() call."""
        return mst_groups(mst.i, mst.j, mst.d2, len(mst.component), radius)

    def set_tracers_f64(self, pos, vel=None):
        """Massless fp64 tracers that hermite_step(), hermite_advance(), hermite6_step() and hermite6_advance() carry beside the bodies
        (nbody_set_tracers_f64); step(), tick() and compute_forces() leave them where they are.  pos, vel: [n, >= 3] float64; vel None =
        at rest; an empty pos removes them.  Replaces any earlier set.  Tracers never act on the bodies or on each other and do not
        enter the shared step (hermite_tracers_timescale() tells what step they would ask for); hermite_block_begin_tracers() and
        hermite6_block_begin_tracers() start block sessions that carry them."""
        p = self._rows64(np.zeros((0, 3)) if pos is None or np.size(pos) == 0 else pos, "set_tracers_f64", "pos")
        v = None if vel is None or p.shape[0] == 0 else self._rows64(vel, "set_tracers_f64", "vel")
        if v is not None and v.shape != p.shape:
            raise ValueError("set_tracers_f64: pos and vel must have the same number of rows")
        self._check(self._L.nbody_set_tracers_f64(self._h, p.ctypes.data if p.shape[0] else None, 24,
                                                  None if v is None else v.ctypes.data, 24, p.shape[0]))

    @property
    def tracer_count_f64(self):
        n = ctypes.c_int32()
        self._check(self._L.nbody_tracer_count_f64(self._h, ctypes.byref(n)))
        return n.value

    def tracers_f64(self):
        """(pos, vel) of the fp64 tracers, [n,3] float64 each (nbody_get_tracers_f64; synchronises).  Feeding them back to
        set_tracers_f64 restores the tracers bit for bit."""
        n = self.tracer_count_f64
        p, v = np.zeros((n, 3), np.float64), np.zeros((n, 3), np.float64)
        self._check(self._L.nbody_get_tracers_f64(self._h, p.ctypes.data, 24, v.ctypes.data, 24))
        return p, v

    def hermite_tracers_state(self):
        """(a, j, a2, a3): the fp64 tracers' fourth-order cache, four [n,3] float64 arrays (nbody_hermite_tracers_get); a2 and a3 are
        zeros until a step has been taken.  ERR_STATE while nothing is cached for the stored tracers."""
        out = np.empty((self.tracer_count_f64, 12), np.float64)
        self._check(self._L.nbody_hermite_tracers_get(self._h, out.ctypes.data, 96))
        return tuple(np.ascontiguousarray(out[:, 3 * k:3 * k + 3]) for k in range(4))

    def hermite6_tracers_state(self):
        """(a, j, s, a3, a4, a5): the fp64 tracers' sixth-order cache, six [n,3] float64 arrays (nbody_hermite6_tracers_get); a3, a4 and
        a5 are zeros until a step has been taken.  ERR_STATE while nothing is cached for the stored tracers."""
        out = np.empty((self.tracer_count_f64, 18), np.float64)
        self._check(self._L.nbody_hermite6_tracers_get(self._h, out.ctypes.data, 144))
        return tuple(np.ascontiguousarray(out[:, 3 * k:3 * k + 3]) for k in range(6))

    def hermite_tracers_timescale(self):
        """(t, tracer, kind): hermite_timescale()'s criterion over the fp64 tracers and the tracer that sets it
        (nbody_hermite_tracers_timescale).  The shared step ignores it: cap dt_max with it if the tracers should limit the step."""
        t, at, kind = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.nbody_hermite_tracers_timescale(self._h, ctypes.byref(t), ctypes.byref(at), ctypes.byref(kind)))
        return t.value, at.value, kind.value

    def hermite6_tracers_timescale(self):
        """(t, tracer, kind): hermite6_timescale()'s criterion over the fp64 tracers (nbody_hermite6_tracers_timescale)."""
        t, at, kind = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.nbody_hermite6_tracers_timescale(self._h, ctypes.byref(t), ctypes.byref(at), ctypes.byref(kind)))
        return t.value, at.value, kind.value

    # -- block sessions that carry the fp64 tracers --
    def _block_begin_tracers(self, fn, dt_max, levels, eta, eta_start, level_in, tracer_level_in):
        def levels_of(a, count, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.int32)
            if a.shape != (count,):
                raise ValueError(f"{name} must hold {count} levels")
            return a
        lv = levels_of(level_in, self.n_total, "level_in")
        tl = None if tracer_level_in is None else np.ascontiguousarray(tracer_level_in, np.int32)
        if tl is not None and tl.ndim != 1:
            raise ValueError("tracer_level_in must be one-dimensional")
        if tl is not None and self.tracer_count_f64 and tl.shape != (self.tracer_count_f64,):
            raise ValueError(f"tracer_level_in must hold {self.tracer_count_f64} levels")
        self._check(fn(self._h, float(dt_max), int(levels), float(eta), float(eta_start), None if lv is None else lv.ctypes.data,
                       None if tl is None else tl.ctypes.data))

    def _block_tracers_state(self, fn):
        st = _lib.HermiteBlockTracerStats()
        st.struct_size = ctypes.sizeof(st)
        self._check(fn(self._h, None, None, ctypes.byref(st)))       # how many the SESSION carries
        ticks, level = np.empty(st.carried, np.int64), np.empty(st.carried, np.int32)
        if st.carried:
            self._check(fn(self._h, ticks.ctypes.data, level.ctypes.data, None))
        return ticks, level, {name: int(getattr(st, name)) for name, _ in st._fields_ if name != "struct_size"}

    def hermite_block_begin_tracers(self, dt_max, levels, eta=0.02, eta_start=0.01, level_in=None, tracer_level_in=None):
        """hermite_block_begin() for a context that holds fp64 tracers (nbody_hermite_block_begin_tracers): the session carries them with
        levels of their own.  One block step takes T_next over bodies AND tracers, predicts everything, and evaluates and corrects the
        due bodies, then the due tracers in the field of the bodies' predicted state: (m_b + m_t) N pairs.  tracer_level_in: a level per
        tracer, 0 .. levels; None: from eta_start |a| / |j| of each tracer's own (a0, j0).  Without tracers it is hermite_block_begin()."""
        self._block_begin_tracers(self._L.nbody_hermite_block_begin_tracers, dt_max, levels, eta, eta_start, level_in, tracer_level_in)

    def hermite6_block_begin_tracers(self, dt_max, levels, eta=0.5, eta_start=0.01, level_in=None, tracer_level_in=None):
        """hermite6_block_begin() for a context that holds fp64 tracers (nbody_hermite6_block_begin_tracers); see
        hermite_block_begin_tracers()."""
        self._block_begin_tracers(self._L.nbody_hermite6_block_begin_tracers, dt_max, levels, eta, eta_start, level_in, tracer_level_in)

    def hermite_block_tracers_state(self):
        """(ticks [M] int64, levels [M] int32, stats): every carried tracer's own time and level, and the tracers' totals since begin as
        a dict: carried, tracer_steps, pairs, tracer_only_steps, floor_hits, level_min, level_max (nbody_hermite_block_tracers_get)."""
        return self._block_tracers_state(self._L.nbody_hermite_block_tracers_get)

    def hermite6_block_tracers_state(self):
        """hermite_block_tracers_state() of a sixth-order session (nbody_hermite6_block_tracers_get)."""
        return self._block_tracers_state(self._L.nbody_hermite6_block_tracers_get)

    def synchronize(self):
        self._check(self._L.nbody_synchronize(self._h))

    def bounds(self):
        s = ctypes.c_float()
        self._check(self._L.nbody_get_bounds(self._h, ctypes.byref(s)))
        return s.value

    def energy(self):
        ke, pe = ctypes.c_double(), ctypes.c_double()
        self._check(self._L.nbody_energy(self._h, ctypes.byref(ke), ctypes.byref(pe)))
        return ke.value, pe.value

    def moments(self):
        """Bulk sums over the owned bodies in one O(N) device pass (nbody_get_moments): a MomentsResult — the raw fp64 sums about the
        origin (they add over slices and ranks) and the derived com, com_velocity, l_about_com.  virial, force and torque use the
        STORED accelerations: call compute_forces() first for the ones of the current positions."""
        m = _lib.Moments()
        m.struct_size = ctypes.sizeof(m)
        self._check(self._L.nbody_get_moments(self._h, ctypes.byref(m)))
        return moments_result(m.count, {k: (getattr(m, k) if k in ("mass", "kinetic", "virial") else list(getattr(m, k)))
                                        for k in MOMENT_FIELDS})

    def mass_within(self, centre, radii):
        """(mass, count) of the owned bodies within each of `radii` of `centre` (nbody_mass_within; d^2 <= r^2 in fp64): float64 and
        int64 arrays shaped like radii.  Any number of radii, 64 to a call — one pass over the positions each."""
        c = np.ascontiguousarray(centre, np.float64)
        if c.shape != (3,):
            raise ValueError("mass_within: centre must be 3 numbers")
        r = np.ascontiguousarray(radii, np.float64)
        flat = r.reshape(-1)
        mass = np.zeros(flat.shape[0], np.float64)
        count = np.zeros(flat.shape[0], np.int64)
        for lo in range(0, flat.shape[0], _lib.MASS_WITHIN_MAX):
            part = np.ascontiguousarray(flat[lo:lo + _lib.MASS_WITHIN_MAX])
            k = part.shape[0]
            m, n = np.zeros(k, np.float64), np.zeros(k, np.int64)
            self._check(self._L.nbody_mass_within(self._h, _dp(c), _dp(part), k, _dp(m), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            mass[lo:lo + k], count[lo:lo + k] = m, n
        return mass.reshape(r.shape), count.reshape(r.shape)

    # -- state out --
    def positions(self, first=0, count=None, out=None):
        """Positions [count,3] (what the renderer reads each frame).  `out`: a C-contiguous float32 array to fill — if it
        was handed to `pin()` the copy is one DMA from the device into it."""
        count = self.n_total - first if count is None else count
        if out is None:
            out = np.empty((count, 3), np.float32)
        elif out.dtype != np.float32 or out.shape != (count, 3) or not out.flags.c_contiguous:
            raise ValueError("positions: out must be a C-contiguous float32 [count,3] array")
        self._check(self._L.nbody_get_positions(self._h, _fp(out), 12, first, count))
        return out

    def particles(self, out=None):
        if out is None:
            out = np.zeros(self.i_count, PARTICLE_DTYPE)
        elif out.dtype != PARTICLE_DTYPE or out.shape != (self.i_count,) or not out.flags.c_contiguous:
            raise ValueError("particles: out must be a C-contiguous PARTICLE_DTYPE [i_count] array")
        self._check(self._L.nbody_get_particles(self._h, out.ctypes.data, PARTICLE_DTYPE.itemsize))
        return out

    def tick(self, dt=REF_DT, out=None):
        """One frame of AOctreeSearch::Tick with a single host synchronisation (nbody_tick): returns (Size of the
        positions before the step — None when dt <= 0 —, the owned FParticle records after it)."""
        if out is None:
            out = np.zeros(self.i_count, PARTICLE_DTYPE)
        elif out.dtype != PARTICLE_DTYPE or out.shape != (self.i_count,) or not out.flags.c_contiguous:
            raise ValueError("tick: out must be a C-contiguous PARTICLE_DTYPE [i_count] array")
        size = ctypes.c_float(0.0)
        self._check(self._L.nbody_tick(self._h, dt, ctypes.byref(size), out.ctypes.data, PARTICLE_DTYPE.itemsize))
        return (size.value if dt > 0 else None), out

    def pin(self, array):
        """Page-lock a caller-owned numpy array for this context (nbody_pin_host_buffer): `positions(out=array)` /
        `particles(out=array)` then land in it with a single device-to-destination copy.  Keep the array alive until
        `unpin(array)` or `close()`."""
        self._check(self._L.nbody_pin_host_buffer(self._h, array.ctypes.data, array.nbytes))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(array)

    def unpin(self, array):
        self._check(self._L.nbody_unpin_host_buffer(self._h, array.ctypes.data))
        self._pinned = [a for a in getattr(self, "_pinned", []) if a is not array]

    def state(self, dtype=np.float32):
        """(posm, vel, acc) of the owned bodies, [i_count,4] each."""
        n = self.i_count
        if dtype == np.float64:
            p, v, a = (np.empty((n, 4), np.float64) for _ in range(3))
            self._check(self._L.nbody_get_state_soa_f64(self._h, _dp(p), _dp(v), _dp(a)))
        else:
            p, v, a = (np.empty((n, 4), np.float32) for _ in range(3))
            self._check(self._L.nbody_get_state_soa(self._h, _fp(p), _fp(v), _fp(a)))
        return p, v, a

    def accelerations(self, dtype=np.float32):
        return self.state(dtype)[2][:, :3]

    # -- checkpoint / resume --
    def save_checkpoint(self, path):
        self._check(self._L.nbody_save_checkpoint(self._h, os.fsencode(path)))

    def load_checkpoint(self, path):
        n = ctypes.c_int64()
        self._check(self._L.nbody_load_checkpoint(self._h, os.fsencode(path), ctypes.byref(n)))
        return n.value

    def steps_done(self):
        n = ctypes.c_int64()
        self._check(self._L.nbody_steps_done(self._h, ctypes.byref(n)))
        return n.value

    # -- device plumbing --
    def set_stream(self, hip_stream_handle):
        self._check(self._L.nbody_set_stream(self._h, ctypes.c_void_p(hip_stream_handle)))

    def device_ptr(self, which):
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.nbody_device_ptr(self._h, which, ctypes.byref(ptr), ctypes.byref(nbytes)))
        return ptr.value, nbytes.value

    def bind_device_state(self, posm=None, vel=None, acc=None):
        """Use caller-owned device buffers (objects with .data_ptr(), e.g. torch tensors)."""
        ptrs = []
        for t in (posm, vel, acc):
            ptrs.append(ctypes.c_void_p(t.data_ptr()) if t is not None else None)
            if t is not None:
                self._keep.append(t)
        self._check(self._L.nbody_bind_device_state(self._h, *ptrs))

    def kernel_time(self, which=_lib.KERNEL_FORCES):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self._L.nbody_kernel_time(self._h, which, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def kernel_time_reset(self):
        self._check(self._L.nbody_kernel_time_reset(self._h))

    def kernel_clock(self):
        """(shader clock in MHz the timed force kernels ran at since the last reset — 0.0 if none of them is instrumented —,
        compute units of the device): nbody_kernel_clock.  Needs time_kernels."""
        mhz, cus = ctypes.c_double(), ctypes.c_int32()
        self._check(self._L.nbody_kernel_clock(self._h, ctypes.byref(mhz), ctypes.byref(cus)))
        return mhz.value, cus.value

    def push_particles(self, particles):
        """Records of the RUNNING simulation edited by the host (nbody_push_particles): like set_particles, but the step count
        and the Barnes-Hut root centre stay."""
        a = np.ascontiguousarray(particles)
        assert a.dtype.itemsize >= 40
        self._check(self._L.nbody_push_particles(self._h, a.ctypes.data, a.dtype.itemsize, a.shape[0]))

    def equal_mass_form(self):
        """Did the last force pass run the equal-mass form of the fp32 symmetric kernel (nbody.h)?"""
        v = ctypes.c_int32()
        self._check(self._L.nbody_equal_mass_form(self._h, ctypes.byref(v)))
        return bool(v.value)

    def sym_pool(self):
        """(bytes of the symmetric pass's partial-sum pool, phases sharing its j-side area) — (0, 0) on the one-sided kernels."""
        b, ph = ctypes.c_uint64(), ctypes.c_int32()
        self._check(self._L.nbody_sym_pool_info(self._h, ctypes.byref(b), ctypes.byref(ph)))
        return b.value, ph.value

    def launch_config(self):
        v = [ctypes.c_int32() for _ in range(5)]
        self._check(self._L.nbody_get_launch_config(self._h, *[ctypes.byref(x) for x in v]))
        cfg = dict(zip(("tile", "i_per_thread", "j_split", "blocks", "threads"), (x.value for x in v)))
        algo, st = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.nbody_get_algorithm(self._h, ctypes.byref(algo), ctypes.byref(st)))
        cfg["algorithm"] = _ALGO_NAME[algo.value]
        cfg["super_tile"] = st.value
        cfg["kernel"] = self._L.nbody_force_kernel_name(self._h).decode()
        cfg["plan"] = ("even" if self._L.nbody_sym_plan_is_even(self._h) else "guided") if cfg["algorithm"] == "symmetric" else None
        return cfg
