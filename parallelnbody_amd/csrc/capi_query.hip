// The fp32 queries of the C-ABI (include/nbody.h), the older twin of capi_query64.hip: the field, potential and tidal tensor at points
// that are not bodies and per body, the jerk (at float points on fp32 state; per body on every precision) and the engine-stepped fp32
// tracers.  Host C++ like capi.hip; shared with the other host units: capi_common.h.  A query's points travel through the staging pair
// (ensure_stage) like the fp64 queries', and like every user of the pair it waits for its own work before it returns.
#include <cmath>
#include <cstring>

#include "bh_driver.h"
#include "capi_common.h"
#include "ctx.h"

namespace {
using nbody::check_ready; using nbody::ensure_floor; using nbody::ensure_probe_part; using nbody::ensure_rows64; using nbody::ensure_stage; using nbody::fail; using nbody::multi_unsupported; using nbody::queue_body_jerk; using nbody::queue_probe;
using nbody::read_energy; using nbody::run_forces; using nbody::run_update; using nbody::scatter_records; using nbody::stage_to_host; using nbody::tidal_time_out; using nbody::timed_launch; using nbody::use_device;

// ---- the field at points that are not bodies: queries (nbody_field_at) and engine-stepped tracers ----
// where they exist: plain fp32 contexts on one device that own all bodies
int probes_supported(nbody_ctx *c, const char *who) {
  if (c->p.precision != NBODY_PREC_F32)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: plain fp32 contexts only (NBODY_PREC_F32)", who);
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  return NBODY_OK;
}

// ... and when: one device, a state set
int probes_ready(nbody_ctx *c, const char *who) {
  if (c && c->multi) return multi_unsupported(c, who);
  if (int rc = check_ready(c)) return rc;
  return probes_supported(c, who);
}

// theta > 0: is there a tree a query may walk?  (`what`: "field", "potential", "tidal tensor")
int probe_tree_ready(nbody_ctx *c, const char *who, const char *what) {
  if (!c->bh || !c->bh_tree_valid || c->bh_tree_theta != c->theta)
    return fail(c, NBODY_ERR_STATE, "%s: theta > 0 walks the last tree built, and there is none for this opening angle "
                "(none built yet, the last frame refused, or theta changed since): call nbody_compute_forces, nbody_step or nbody_tick first", who);
  if (nbody::bh_last_deep(c->bh))
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: the last tree was built deeper than 42 levels (nbody_set_bh_max_depth); "
                "such trees answer no %s queries", who, what);
  return NBODY_OK;
}

// theta == 0: the potential of the bodies at their CURRENT positions at m points, queued (G and eps the context's; eps == 0: the exact
// d == 0 rule whatever its zero_mode is).  probe == nullptr: at the bodies themselves (m == n_total).
int queue_pot(nbody_ctx *c, const void *probe, int m, double *phi64, float *phif) {
  nbody::PotLaunch L;
  L.posm = c->posm; L.probe = probe; L.part = c->probe_part; L.phi64 = phi64; L.phif = phif;
  L.n_total = c->p.n_total; L.m = m; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps; L.clk = c->clk;
  HIP_TRY(c, nbody::launch_pot(L, c->stream));
  return NBODY_OK;
}

// theta == 0: the tidal tensor of the bodies at their CURRENT positions at m points, queued (G and eps the context's; eps == 0: the
// potential's d == 0 rule, whatever the zero_mode).  probe == nullptr: at the bodies themselves (m == n_total).
int queue_tidal(nbody_ctx *c, const void *probe, int m, double *t64, float *tf) {
  nbody::TidalLaunch L;
  L.posm = c->posm; L.probe = probe; L.part = c->probe_part; L.t64 = t64; L.tf = tf;
  L.n_total = c->p.n_total; L.m = m; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps; L.clk = c->clk;
  HIP_TRY(c, nbody::launch_tidal(L, c->stream));
  return NBODY_OK;
}

// The bodies' potentials (tidal: their tidal tensors) at their CURRENT positions, queued on the stream as one pass under
// NBODY_KERNEL_FORCES: r64 ([n_total] double, tidal: [n_total][6]; device) and / or rf (the same in floats).  theta > 0: first exactly
// what nbody_compute_forces runs (the tree of the current positions, the stored accelerations, the tracers'), then the walk of that tree
// from every body.
int queue_body_rows(nbody_ctx *c, const char *who, bool tidal, double *r64, float *rf) {
  int rc;
  const int n = c->p.n_total;
  if (c->theta > 0.0f) {
    if ((rc = run_forces(c, true, 0, 0.0f))) return rc;            // (a refused frame: its error, no rows)
    if ((rc = run_update(c, 0.0f))) return rc;
    if ((rc = probe_tree_ready(c, who, tidal ? "tidal tensor" : "potential"))) return rc;
    return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
      const float eps2 = (float)(c->p.eps * c->p.eps);
      HIP_TRY(c, tidal ? nbody::bh_tidal_walk(c->bh, c->posm, nullptr, r64, rf, n, c->p.G, eps2, c->stream)
                       : nbody::bh_pot_walk(c->bh, c->posm, nullptr, r64, rf, n, c->p.G, eps2, c->stream));
      return NBODY_OK;
    });
  }
  if ((rc = ensure_probe_part(c, n, tidal ? 2 : 1))) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return tidal ? queue_tidal(c, nullptr, n, r64, rf) : queue_pot(c, nullptr, n, r64, rf); });
}

// nbody_get_potentials / nbody_get_tidal: n_total rows of 4 / 24 bytes
int body_rows_get(nbody_ctx *c, const char *who, bool tidal, float *out, size_t stride) {
  int rc = probes_ready(c, who);
  if (rc) return rc;
  const size_t n = (size_t)c->p.n_total, rec = tidal ? 24 : 4;
  if (!out || stride < rec) return fail(c, NBODY_ERR_INVALID, "%s: null buffer or stride < %d", who, (int)rec);
  if ((rc = ensure_stage(c, n * rec))) return rc;
  if ((rc = queue_body_rows(c, who, tidal, nullptr, (float *)c->d_stage))) return rc;
  if ((rc = stage_to_host(c, 0, n * rec))) return rc;
  scatter_records(out, stride, c->h_stage, rec, n);
  return NBODY_OK;
}

// ---- the jerk: a pair sum over all bodies at every theta, on every precision (kernels_jerk.hip) ----
// where it exists: contexts on one device that own all bodies; at caller-given points (float arrays) those whose state is fp32 as well —
// and when: a state set
int jerk_ready(nbody_ctx *c, const char *who, bool points) {
  if (c && c->multi) return multi_unsupported(c, who);
  if (int rc = check_ready(c)) return rc;
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  if (points && c->p.precision == NBODY_PREC_F64)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on an fp64 context (its points would have to be doubles); nbody_get_jerk_f64 answers at the bodies", who);
  return NBODY_OK;
}

// (a, j) of the bodies' LIVE buffers — c->posm is the current one of the one-launch step's two, c->vel every path's velocities, as
// nbody_get_moments reads them — at m points, queued (the partial rows are the caller's to provide).  probe == nullptr: at the bodies themselves.
// eps == 0: the potential's d == 0 rule, whatever the zero_mode.  No tree is read or built.
int launch_jerk_on(nbody_ctx *c, const void *probe, const void *pvel, int m, double *aj64, float *ajf) {
  nbody::JerkLaunch L;
  L.posm = c->posm; L.vel = c->vel; L.probe = probe; L.pvel = pvel; L.part = c->probe_part; L.aj64 = aj64; L.ajf = ajf;
  L.n_total = c->p.n_total; L.m = m; L.precision = c->p.precision; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
  HIP_TRY(c, nbody::launch_jerk(L, c->stream));
  return NBODY_OK;
}

// One query at points that are not bodies: n points from (xyz, stride) in, `width` floats each out to (out, out_stride) — the
// arguments' checks (`bad_args`: the message of a bad one), the tree or the partial rows the launch needs, the points as float4
// through the staging pair, launch(d_pts, d_out) timed as a pass under NBODY_KERNEL_FORCES, the values back (d_out: a float4 per
// point for width 3, `width` floats otherwise).  floor: the query follows the context's NBODY_ZERO_FLOOR.  part_width: the float4 of a
// point in a chunk's partial row (theta == 0).
// `pair` (the jerk): a second input array — 3 floats per point, staged as float4 behind the points (d_pts + 4 n); NULL: zeros — and a
// second output of `width` floats behind the first in the point's device record (2 * width floats, packed); either output may be NULL,
// not both.  Such a query is a pair sum at every theta (no tree is asked for) and is served where jerk_ready says.
struct PointPair { const float *in; size_t in_stride; float *out; size_t out_stride; };
template <class Launch>
int query_points(nbody_ctx *c, const char *who, const char *what, const char *bad_args, bool floor, const float *xyz, size_t stride,
                 int32_t n, float *out, size_t out_stride, int width, int part_width, Launch launch, const PointPair *pair = nullptr) {
  int rc = pair ? jerk_ready(c, who, true) : probes_ready(c, who);
  if (rc) return rc;
  const size_t out_min = 4 * (size_t)width;
  bool bad = n < 0 || !xyz || stride < 12;
  if (pair) bad = bad || (pair->in && pair->in_stride < 12) || (!out && !pair->out) || (out && out_stride < out_min) ||
                  (pair->out && pair->out_stride < out_min);
  else      bad = bad || !out || out_stride < out_min;
  if (bad) return fail(c, NBODY_ERR_INVALID, "%s: %s", who, bad_args);
  if (n == 0) return NBODY_OK;
  if (c->theta > 0.0f && !pair) {
    if ((rc = probe_tree_ready(c, who, what))) return rc;
  } else {
    if (floor && (rc = ensure_floor(c))) return rc;
    if ((rc = ensure_probe_part(c, n, part_width))) return rc;
  }
  const size_t out_floats = pair ? 2 * (size_t)width : (width == 3 ? 4 : (size_t)width);
  const size_t in_floats = pair ? 8 : 4;
  const size_t in_bytes = (size_t)n * in_floats * 4, out_bytes = (size_t)n * out_floats * 4;
  if ((rc = ensure_stage(c, in_bytes + out_bytes))) return rc;
  float *h_pts = (float *)c->h_stage, *h_out = h_pts + in_floats * (size_t)n;
  float *d_pts = (float *)c->d_stage, *d_out = d_pts + in_floats * (size_t)n;
  nbody::gather4(h_pts, xyz, stride, (size_t)n);
  if (pair) nbody::gather4(h_pts + 4 * (size_t)n, pair->in, pair->in_stride, (size_t)n);
  HIP_TRY(c, hipMemcpyAsync(d_pts, h_pts, in_bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return launch(d_pts, d_out); }))) return rc;
  if ((rc = stage_to_host(c, in_bytes, out_bytes))) return rc;
  if (out) scatter_records(out, out_stride, h_out, out_min, (size_t)n, 4 * out_floats);
  if (pair && pair->out) scatter_records(pair->out, pair->out_stride, h_out + width, out_min, (size_t)n, 4 * out_floats);
  return NBODY_OK;
}

// nbody_get_jerk / nbody_get_jerk_f64: T = float / double
template <typename T>
int get_jerk(nbody_ctx *c, const char *who, T *acc, size_t acc_stride, T *jerk, size_t jerk_stride) {
  int rc = jerk_ready(c, who, false);
  if (rc) return rc;
  if ((!acc && !jerk) || (acc && acc_stride < 3 * sizeof(T)) || (jerk && jerk_stride < 3 * sizeof(T)))
    return fail(c, NBODY_ERR_INVALID, "%s: both outputs are null, or a stride < %d", who, (int)(3 * sizeof(T)));
  const size_t n = (size_t)c->p.n_total, rec = 6 * sizeof(T);
  if ((rc = ensure_stage(c, n * rec))) return rc;
  if constexpr (sizeof(T) == 8) {
    if ((rc = ensure_rows64(c, &c->jerk64, 6))) return rc;
    if ((rc = queue_body_jerk(c, (double *)c->jerk64, nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->jerk64, n * rec, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    if ((rc = queue_body_jerk(c, nullptr, (float *)c->d_stage))) return rc;
    if ((rc = stage_to_host(c, 0, n * rec))) return rc;
  }
  if (acc) scatter_records(acc, acc_stride, c->h_stage, rec / 2, n, rec);
  if (jerk) scatter_records(jerk, jerk_stride, (const char *)c->h_stage + rec / 2, rec / 2, n, rec);
  return NBODY_OK;
}
}  // namespace

// The bodies' own (a, j), as one pass under NBODY_KERNEL_FORCES; the partial rows in the staging area the point queries use: two
// float4 per body and chunk, six doubles on fp64 state.
int nbody::queue_body_jerk(nbody_ctx *c, double *aj64, float *ajf) {
  const int n = c->p.n_total;
  if (int rc = ensure_probe_part(c, n, c->p.precision == NBODY_PREC_F64 ? 3 : 2)) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return launch_jerk_on(c, nullptr, nullptr, n, aj64, ajf); });
}

int nbody::ensure_rows64(nbody_ctx *c, void **buf, int width) {
  const size_t n = (size_t)c->p.n_total;
  if (!*buf) HIP_TRY(c, hipMalloc(buf, ((size_t)width * n + 2 * (size_t)nbody::energy_fast_slots((int)n)) * sizeof(double)));
  return NBODY_OK;
}

int nbody::tidal_time_out(nbody_ctx *c, double *t_min, int32_t *body) {
  const int n = c->p.n_total;
  double *t64 = (double *)c->tidal64, *partials = t64 + 6 * (size_t)n;
  HIP_TRY(c, nbody::launch_tidal_time(t64, n, partials, (double *)c->scratch, c->stream));
  double n2 = 0.0, at = 0.0;
  if (int rc = read_energy(c, &n2, &at)) return rc;            // (the scratch's two doubles: the largest n2, its body)
  // t = ||T||_F^(-1/2) = n2^(-1/4)
  if (t_min) *t_min = n2 == 0.0 ? HUGE_VAL : (std::isfinite(n2) ? 1.0 / std::sqrt(std::sqrt(n2)) : 0.0);
  if (body) *body = (int32_t)at;
  return NBODY_OK;
}

extern "C" {

int nbody_field_at(nbody_ctx *c, const float *xyz, size_t stride, int32_t n, float *acc, size_t acc_stride) {
  return query_points(c, "nbody_field_at", "field", "null buffer, n < 0 or a stride < 12", true, xyz, stride, n, acc, acc_stride, 3,
                      1, [&](float *d_pts, float *d_acc) -> int {
    if (!(c->theta > 0.0f)) return queue_probe(c, d_pts, nullptr, d_acc, n, 0.0f);
    HIP_TRY(c, nbody::bh_probe_walk(c->bh, d_pts, nullptr, d_acc, n, c->p.G, (float)(c->p.eps * c->p.eps), 0.0f, c->stream));
    return NBODY_OK;
  });
}

// (no ensure_floor: the potential's d == 0 rule is the same under every zero_mode)
int nbody_potential_at(nbody_ctx *c, const float *xyz, size_t stride, int32_t n, float *phi, size_t phi_stride) {
  return query_points(c, "nbody_potential_at", "potential", "null buffer, n < 0, a point stride < 12 or a potential stride < 4", false, xyz,
                      stride, n, phi, phi_stride, 1, 1, [&](float *d_pts, float *d_phi) -> int {
    if (!(c->theta > 0.0f)) return queue_pot(c, d_pts, n, nullptr, d_phi);
    HIP_TRY(c, nbody::bh_pot_walk(c->bh, c->posm, d_pts, nullptr, d_phi, n, c->p.G, (float)(c->p.eps * c->p.eps), c->stream));
    return NBODY_OK;
  });
}

int nbody_get_potentials(nbody_ctx *c, float *phi, size_t stride) { return body_rows_get(c, "nbody_get_potentials", false, phi, stride); }

int nbody_energy_fast(nbody_ctx *c, double *ke, double *pe) {
  int rc = probes_ready(c, "nbody_energy_fast");
  if (rc) return rc;
  const int n = c->p.n_total;
  if ((rc = ensure_rows64(c, &c->pot64, 1))) return rc;
  double *phi64 = (double *)c->pot64, *partials = phi64 + n;
  if ((rc = queue_body_rows(c, "nbody_energy_fast", false, phi64, nullptr))) return rc;
  HIP_TRY(c, nbody::launch_energy_fast(c->posm, c->vel, phi64, n, partials, (double *)c->scratch, c->stream));
  return read_energy(c, ke, pe);
}

int nbody_tidal_at(nbody_ctx *c, const float *xyz, size_t stride, int32_t n, float *t, size_t t_stride) {
  return query_points(c, "nbody_tidal_at", "tidal tensor", "null buffer, n < 0, a point stride < 12 or a tensor stride < 24", false, xyz,
                      stride, n, t, t_stride, 6, 2, [&](float *d_pts, float *d_t) -> int {
    if (!(c->theta > 0.0f)) return queue_tidal(c, d_pts, n, nullptr, d_t);
    HIP_TRY(c, nbody::bh_tidal_walk(c->bh, c->posm, d_pts, nullptr, d_t, n, c->p.G, (float)(c->p.eps * c->p.eps), c->stream));
    return NBODY_OK;
  });
}

int nbody_get_tidal(nbody_ctx *c, float *t, size_t stride) { return body_rows_get(c, "nbody_get_tidal", true, t, stride); }

int nbody_tidal_time(nbody_ctx *c, double *t_min, int32_t *body) {
  int rc = probes_ready(c, "nbody_tidal_time");
  if (rc) return rc;
  if (!t_min && !body) return fail(c, NBODY_ERR_INVALID, "nbody_tidal_time: both outputs are null");
  if ((rc = ensure_rows64(c, &c->tidal64, 6))) return rc;
  if ((rc = queue_body_rows(c, "nbody_tidal_time", true, (double *)c->tidal64, nullptr))) return rc;
  return tidal_time_out(c, t_min, body);
}

int nbody_jerk_at(nbody_ctx *c, const float *xyz, size_t stride, const float *vel, size_t vel_stride, int32_t n, float *acc,
                  size_t acc_stride, float *jerk, size_t jerk_stride) {
  const PointPair pair{vel, vel_stride, jerk, jerk_stride};
  return query_points(c, "nbody_jerk_at", "jerk", "null points, n < 0, both outputs null, or a stride < 12", false, xyz, stride, n, acc,
                      acc_stride, 3, 2, [&](float *d_pts, float *d_aj) -> int {
    return launch_jerk_on(c, d_pts, d_pts + 4 * (size_t)n, n, nullptr, d_aj);
  }, &pair);
}

int nbody_get_jerk(nbody_ctx *c, float *acc, size_t acc_stride, float *jerk, size_t jerk_stride) {
  return get_jerk<float>(c, "nbody_get_jerk", acc, acc_stride, jerk, jerk_stride);
}

int nbody_get_jerk_f64(nbody_ctx *c, double *acc, size_t acc_stride, double *jerk, size_t jerk_stride) {
  return get_jerk<double>(c, "nbody_get_jerk_f64", acc, acc_stride, jerk, jerk_stride);
}

int nbody_jerk_time(nbody_ctx *c, double *t_min, int32_t *body) {
  int rc = jerk_ready(c, "nbody_jerk_time", false);
  if (rc) return rc;
  if (!t_min && !body) return fail(c, NBODY_ERR_INVALID, "nbody_jerk_time: both outputs are null");
  const int n = c->p.n_total;
  if ((rc = ensure_rows64(c, &c->jerk64, 6))) return rc;
  double *aj64 = (double *)c->jerk64, *partials = aj64 + 6 * (size_t)n;
  if ((rc = queue_body_jerk(c, aj64, nullptr))) return rc;
  HIP_TRY(c, nbody::launch_jerk_time(aj64, n, partials, (double *)c->scratch, c->stream));
  double k = 0.0, at = 0.0;
  if ((rc = read_energy(c, &k, &at))) return rc;               // (the scratch's two doubles: the largest |j|^2 / |a|^2, its body)
  if (t_min) *t_min = k == 0.0 ? HUGE_VAL : (std::isfinite(k) ? 1.0 / std::sqrt(k) : 0.0);
  if (body) *body = (int32_t)at;
  return NBODY_OK;
}

int nbody_set_tracers(nbody_ctx *c, const float *pos4, const float *vel4, int32_t n) {
  if (c && c->multi) return multi_unsupported(c, "nbody_set_tracers");
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = probes_supported(c, "nbody_set_tracers")) return rc;
  if (n < 0 || (n > 0 && !pos4)) return fail(c, NBODY_ERR_INVALID, "nbody_set_tracers: n < 0 or null positions");
  if (n > 0 && c->bh_max_depth > 42)
    return fail(c, NBODY_ERR_UNSUPPORTED, "nbody_set_tracers: this context builds trees deeper than 42 levels (nbody_set_bh_max_depth), "
                "which do not carry tracers");
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (void **q : {&c->tr_pos, &c->tr_vel, &c->tr_acc}) { if (*q) (void)hipFree(*q); *q = nullptr; }
  c->tr_n = 0;
  if (n == 0) return NBODY_OK;
  const size_t bytes = (size_t)n * 16;
  HIP_TRY(c, hipMalloc(&c->tr_pos, bytes));
  HIP_TRY(c, hipMalloc(&c->tr_vel, bytes));
  HIP_TRY(c, hipMalloc(&c->tr_acc, bytes));
  HIP_TRY(c, hipMemcpyAsync(c->tr_pos, pos4, bytes, hipMemcpyHostToDevice, c->stream));
  if (vel4) HIP_TRY(c, hipMemcpyAsync(c->tr_vel, vel4, bytes, hipMemcpyHostToDevice, c->stream));
  else      HIP_TRY(c, hipMemsetAsync(c->tr_vel, 0, bytes, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->tr_acc, 0, bytes, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));                     // the caller's arrays are its own again
  c->tr_n = n;
  return NBODY_OK;
}

int nbody_get_tracers(nbody_ctx *c, float *pos4, float *vel4, float *acc4) {
  if (c && c->multi) return multi_unsupported(c, "nbody_get_tracers");
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t bytes = (size_t)c->tr_n * 16;
  if (bytes == 0) return NBODY_OK;
  if (pos4) HIP_TRY(c, hipMemcpy(pos4, c->tr_pos, bytes, hipMemcpyDeviceToHost));
  if (vel4) HIP_TRY(c, hipMemcpy(vel4, c->tr_vel, bytes, hipMemcpyDeviceToHost));
  if (acc4) HIP_TRY(c, hipMemcpy(acc4, c->tr_acc, bytes, hipMemcpyDeviceToHost));
  return NBODY_OK;
}

int nbody_tracer_count(nbody_ctx *c, int32_t *n) {
  if (c && c->multi) return multi_unsupported(c, "nbody_tracer_count");
  if (!c || !n) return NBODY_ERR_INVALID;
  *n = c->tr_n;
  return NBODY_OK;
}

}  // extern "C"
