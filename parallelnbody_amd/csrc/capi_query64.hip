// The fp64 queries of the C-ABI (include/nbody.h) on fp64 contexts that are not Hermite stepping: the potential and tidal tensor
// (kernels_pot64.hip), the pair census (kernels_census64.hip), the neighbour census (kernels_neighbours64.hip), the radial census
// (kernels_radial64.hip), the group census (kernels_groups64.hip), the separation census (kernels_pairs64.hip) and the minimum spanning forest (kernels_mst64.hip).  Host C++ like capi.hip; what it shares with the other host units: capi_common.h.
// Written once here: the row pass (row_pass64) every N^2 query is queued through, and the staged points (Staged64) of every *_at_f64 call.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi_common.h"
#include "ctx.h"

namespace nbody {

// where the points exist — the contexts that answer nbody_hermite_step: fp64 state, one device, all bodies — and when: a state set, no step half done
int points64_ready(nbody_ctx *c, const char *who) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return multi_unsupported(c, who);
  if (c->p.precision != NBODY_PREC_F64)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context whose state is fp32 (NBODY_PREC_F32, NBODY_PREC_F32_KAHAN): its points are doubles "
                "in the field of fp64 bodies; create the context with NBODY_PREC_F64 (fp32 contexts have nbody_jerk_at and nbody_set_tracers)", who);
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  if (int rc = check_ready(c)) return rc;
  if (c->step_open || c->step_local) return fail(c, NBODY_ERR_STATE, "%s: a step is open (nbody_step_end first)", who);
  return NBODY_OK;
}

int stage_points64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, bool with_vel, size_t m,
                   size_t result_bytes, Staged64 *s) {
  s->m = m; s->skip = (with_vel ? 8 : 4) * m;
  if (int rc = ensure_stage(c, s->skip * sizeof(double) + result_bytes)) return rc;
  s->h = (double *)c->h_stage; s->d = (double *)c->d_stage;
  gather4(s->h, pos, pos_stride, m);
  if (with_vel) gather4(s->h + 4 * m, vel, vel_stride, m);
  HIP_TRY(c, hipMemcpyAsync(s->d, s->h, s->skip * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return NBODY_OK;
}

int stage_to_host(nbody_ctx *c, size_t first, size_t bytes) {
  HIP_TRY(c, hipMemcpyAsync((char *)c->h_stage + first, (const char *)c->d_stage + first, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

int points64_part_holds(nbody_ctx *c, int m, int width, const char *what) {
  const size_t need = probe_part_elems(c->p.n_total, m, width);
  if (c->probe_part && c->probe_part_elems >= need) return NBODY_OK;
  return fail(c, NBODY_ERR_STATE, "%s: the partial rows of %d points need %zu float4, the staging area holds %zu", what, m, need, c->probe_part_elems);
}

}  // namespace nbody

namespace {

using nbody::check_ready; using nbody::ensure_probe_part; using nbody::ensure_rows64; using nbody::tidal_time_out; using nbody::ensure_stage; using nbody::fail; using nbody::points64_part_holds; using nbody::points64_ready; using nbody::read_energy; using nbody::scatter_records; using nbody::stage_points64; using nbody::stage_to_host; using nbody::Staged64; using nbody::timed_launch;

// ---- the row pass: every N^2 query of this unit (kernels.h: RowScan64Launch) ----
// rows — m points (ppos: double4 each, device) or, ppos == nullptr, the bodies themselves with each left out by index — against the LIVE
// state: one pass under NBODY_KERNEL_FORCES, never queued into a staging area that does not hold a slab's partial rows of `width`
// float4.  L holds what is the pass's own; run(L) launches it.
template <class Launch, class Run>
int row_pass64(nbody_ctx *c, int width, const char *what, const void *ppos, int m, Launch L, Run run) {
  if (int rc = ensure_probe_part(c, m, width)) return rc;
  if (int rc = points64_part_holds(c, m, width, what)) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
    L.posm = c->posm; L.ppos = ppos; L.part = c->probe_part; L.part_elems = c->probe_part_elems; L.n_total = c->p.n_total; L.m = m;
    HIP_TRY(c, run(L));
    return NBODY_OK;
  });
}

// ---- the fp64 potential and tidal tensor (kernels_pot64.hip) ----
// phi ([m]) or the tensors ([m][6]) into out (device) — at m points (ppos: double4 each, device) or, ppos == nullptr, at the bodies
// themselves
int pot64_pass(nbody_ctx *c, bool tidal, const void *ppos, int m, double *out) {
  nbody::Pot64Launch L;
  L.out = out; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
  return row_pass64(c, tidal ? nbody::kTidal64Width : nbody::kPot64Width, tidal ? "the fp64 tidal pass" : "the fp64 potential pass", ppos, m, L,
                    [&](const nbody::Pot64Launch &P) { return tidal ? nbody::launch_tidal_f64(P, c->stream) : nbody::launch_pot_f64(P, c->stream); });
}

// nbody_potential_at_f64 / nbody_tidal_at_f64: n points in, `doubles` (1 / 6) per point out
int pot64_at(nbody_ctx *c, const char *who, bool tidal, const double *pos, size_t pos_stride, int32_t n, double *out, size_t out_stride) {
  const size_t doubles = tidal ? 6 : 1;
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (n < 0 || !pos || pos_stride < 24 || !out || out_stride < doubles * 8)
    return fail(c, NBODY_ERR_INVALID, "%s: null buffer, n < 0, a point stride < 24 or an output stride < %d", who, (int)(doubles * 8));
  if (n == 0) return NBODY_OK;
  Staged64 s;
  if ((rc = stage_points64(c, pos, pos_stride, nullptr, 0, false, (size_t)n, (size_t)n * doubles * 8, &s))) return rc;
  if ((rc = pot64_pass(c, tidal, s.d, n, s.d + s.skip))) return rc;
  if ((rc = stage_to_host(c, s.skip * 8, s.m * doubles * 8))) return rc;
  scatter_records(out, out_stride, s.h + s.skip, doubles * 8, s.m);
  return NBODY_OK;
}

// nbody_get_potentials_f64 / nbody_get_tidal_f64: n_total rows
int pot64_get(nbody_ctx *c, const char *who, bool tidal, double *out, size_t stride) {
  const size_t doubles = tidal ? 6 : 1;
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!out || stride < doubles * 8) return fail(c, NBODY_ERR_INVALID, "%s: null buffer or stride < %d", who, (int)(doubles * 8));
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * doubles * 8))) return rc;
  if ((rc = pot64_pass(c, tidal, nullptr, (int)n, (double *)c->d_stage))) return rc;
  if ((rc = stage_to_host(c, 0, n * doubles * 8))) return rc;
  scatter_records(out, stride, c->h_stage, doubles * 8, n);
  return NBODY_OK;
}

// ---- the fp64 pair census (kernels_census64.hip) ----
// per row the nearest body (index, value = d2) or, bound, the most-bound partner (index, value = e, d2) into device arrays — at m points
// (ppos, pvel: double4 each, device) or, ppos == nullptr, at the bodies themselves
int census64_pass(nbody_ctx *c, bool bound, const void *ppos, const void *pvel, int m, int *index, double *value, double *d2) {
  nbody::Census64Launch L;
  L.vel = c->vel; L.pvel = pvel; L.index = index; L.value = value; L.d2 = d2; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
  return row_pass64(c, bound ? nbody::kPartner64Width : nbody::kNearest64Width, bound ? "the fp64 partner pass" : "the fp64 nearest pass", ppos, m, L,
                    [&](const nbody::Census64Launch &P) { return bound ? nbody::launch_partner_f64(P, c->stream) : nbody::launch_nearest_f64(P, c->stream); });
}

// the results of m rows behind `skip` doubles of the staging pair: value [m], d2 [m], index [m] (int32)
struct CensusRows { double *value, *d2; int *index; };
CensusRows census_rows(void *stage, size_t skip, size_t m) {
  double *v = (double *)stage + skip;
  return CensusRows{v, v + m, (int *)(v + 2 * m)};
}
constexpr size_t kCensusRowBytes = 20;   // of the staging pair, per row

// rows m of the staging pair to the caller's arrays: value and d2 are the nearest form's one array (d2), the partner form's two
int census64_out(nbody_ctx *c, bool bound, size_t skip, size_t m, int32_t *index, double *energy, double *d2) {
  if (int rc = stage_to_host(c, skip * 8, m * kCensusRowBytes)) return rc;
  const CensusRows h = census_rows(c->h_stage, skip, m);
  if (index) memcpy(index, h.index, m * 4);
  if (bound) {
    if (energy) memcpy(energy, h.value, m * 8);
    if (d2) memcpy(d2, h.d2, m * 8);
  } else if (d2) {
    memcpy(d2, h.value, m * 8);
  }
  return NBODY_OK;
}

// nbody_get_nearest_f64 / nbody_get_partners_f64: n_total rows
int census64_get(nbody_ctx *c, const char *who, bool bound, int32_t *index, double *energy, double *d2) {
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!index && !energy && !d2) return fail(c, NBODY_ERR_INVALID, "%s: every output is null", who);
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * kCensusRowBytes))) return rc;
  const CensusRows d = census_rows(c->d_stage, 0, n);
  if ((rc = census64_pass(c, bound, nullptr, nullptr, (int)n, d.index, d.value, d.d2))) return rc;
  return census64_out(c, bound, 0, n, index, energy, d2);
}

// nbody_nearest_at_f64 / nbody_partner_at_f64: n points in (bound: moving with vel, NULL = at rest)
int census64_at(nbody_ctx *c, const char *who, bool bound, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n,
                int32_t *index, double *energy, double *d2) {
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (n < 0 || !pos || pos_stride < 24 || (vel && vel_stride < 24) || (!index && !energy && !d2))
    return fail(c, NBODY_ERR_INVALID, "%s: null points, n < 0, every output null, or a stride < 24", who);
  if (n == 0) return NBODY_OK;
  Staged64 s;
  if ((rc = stage_points64(c, pos, pos_stride, vel, vel_stride, bound, (size_t)n, (size_t)n * kCensusRowBytes, &s))) return rc;
  const CensusRows d = census_rows(c->d_stage, s.skip, s.m);
  if ((rc = census64_pass(c, bound, s.d, bound ? s.d + 4 * s.m : nullptr, n, d.index, d.value, d.d2))) return rc;
  return census64_out(c, bound, s.skip, s.m, index, energy, d2);
}

// nbody_closest_pair_f64 / nbody_hardest_pair_f64: the per-body pass, then its smallest value and the lowest row that attains it,
// reduced on the device in a fixed order — r = (value, i, j = that row's index, d2), (+inf, -1, -1, +inf) where there is none
int census64_pair(nbody_ctx *c, bool bound, double (&r)[4]) {
  const size_t n = (size_t)c->p.n_total, slots = (size_t)nbody::energy_fast_slots((int)n);
  const size_t skip = 2 * slots + 4;                             // the reduction's partials and its four doubles, ahead of the rows
  int rc = ensure_stage(c, skip * sizeof(double) + n * kCensusRowBytes);
  if (rc) return rc;
  double *partials = (double *)c->d_stage, *out = partials + 2 * slots;
  const CensusRows d = census_rows(c->d_stage, skip, n);
  if ((rc = census64_pass(c, bound, nullptr, nullptr, (int)n, d.index, d.value, d.d2))) return rc;
  HIP_TRY(c, nbody::launch_census_pair(d.value, d.index, bound ? d.d2 : nullptr, (int)n, partials, out, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, out, sizeof(r), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(r, c->h_stage, sizeof(r));
  return NBODY_OK;
}

// ---- the fp64 neighbour census (kernels_neighbours64.hip) ----
// per row the k nearest bodies (index, d2: rows of k) and, at the bodies with 2 <= k, the local density (rho, rk2) into device arrays
// (each may be null) — at m points (ppos: double4, device) or, ppos == nullptr, at the bodies themselves
int neighbours64_pass(nbody_ctx *c, int k, const void *ppos, int m, int *index, double *d2, double *rho, double *rk2) {
  nbody::Neighbours64Launch L;
  L.index = index; L.d2 = d2; L.rho = rho; L.rk2 = rk2; L.k = k; L.G = c->p.G;
  return row_pass64(c, nbody::neighbours64_width(k), "the fp64 neighbour pass", ppos, m, L,
                    [&](const nbody::Neighbours64Launch &P) { return nbody::launch_neighbours_f64(P, c->stream); });
}

// the lists of m rows behind `skip` doubles of the staging pair — d2 [m * k], index [m * k] (int32) — to the caller's arrays
int neighbours64_lists(nbody_ctx *c, int k, const void *ppos, size_t skip, size_t m, int32_t *index, double *d2) {
  double *dd2 = (double *)c->d_stage + skip;
  int *dindex = (int *)(dd2 + m * k);
  if (int rc = neighbours64_pass(c, k, ppos, (int)m, dindex, dd2, nullptr, nullptr)) return rc;
  if (int rc = stage_to_host(c, skip * 8, m * k * 12)) return rc;
  const double *hd2 = (const double *)c->h_stage + skip;
  if (d2) memcpy(d2, hd2, m * k * 8);
  if (index) memcpy(index, hd2 + m * k, m * k * 4);
  return NBODY_OK;
}

// k within lo .. NBODY_NEIGHBOURS_MAX
static_assert(nbody::kNeighbours64Max == NBODY_NEIGHBOURS_MAX, "the widest compiled list is the largest k of the C-ABI");
int neighbours64_k(nbody_ctx *c, const char *who, int32_t k, int lo) {
  if (k >= lo && k <= NBODY_NEIGHBOURS_MAX) return NBODY_OK;
  return fail(c, NBODY_ERR_INVALID, "%s: k = %d is outside %d .. %d", who, (int)k, lo, NBODY_NEIGHBOURS_MAX);
}

// ---- the fp64 radial census (kernels_radial64.hip) ----
static_assert(sizeof(nbody_lagrange) == 40 && nbody::kRadialFractionsMax == NBODY_LAGRANGE_MAX, "include/nbody.h and kernels.h agree");

// The order about `centre`, the cumulative mass in it and, k > 0, the rows of k fractions, queued on the stream from the LIVE positions
// and left in the staging area on the device: *W says where.  Not a pair pass: no kernel timer counts it (as nbody_get_moments').
// NBODY_RADIAL_PHASES=1 (read at every call; tools/radial_f64_measure.py): event pairs round the four phases, waited for and printed
// to stderr.
int radial64_run(nbody_ctx *c, const double centre[3], const double *fractions, int k, nbody::Radial64Work *W) {
  *W = nbody::radial64_work(c->p.n_total);
  if (int rc = ensure_stage(c, W->bytes)) return rc;
  if (c->radial_resident == 0) HIP_TRY(c, nbody::radial64_resident(&c->radial_resident));
  nbody::Radial64Launch L;
  L.posm = c->posm; L.n_total = c->p.n_total;
  L.centre[0] = centre[0]; L.centre[1] = centre[1]; L.centre[2] = centre[2];
  L.fractions = fractions; L.k = k; L.resident = c->radial_resident; L.work = c->d_stage;
  const char *env = getenv("NBODY_RADIAL_PHASES");
  if (!(env && env[0] == '1')) {
    HIP_TRY(c, nbody::launch_radial_f64(L, c->stream));
    return NBODY_OK;
  }
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t err = hipSuccess;
  for (int q = 0; q < 5 && err == hipSuccess; ++q) err = hipEventCreate(&ev[q]);
  L.events = ev;
  if (err == hipSuccess) err = nbody::launch_radial_f64(L, c->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
  float ms[4] = {0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < 4 && err == hipSuccess; ++q) err = hipEventElapsedTime(&ms[q], ev[q], ev[q + 1]);
  for (int q = 0; q < 5; ++q) if (ev[q]) (void)hipEventDestroy(ev[q]);
  HIP_TRY(c, err);
  fprintf(stderr, "radial_f64 phases: n %d k %d keys %.4f sort %.4f scan %.4f select %.4f ms\n", c->p.n_total, k, ms[0], ms[1], ms[2], ms[3]);
  return NBODY_OK;
}

bool radial64_centre_ok(const double centre[3]) {
  return centre && std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2]);
}

// ---- the fp64 group census (kernels_groups64.hip) ----
static_assert(sizeof(nbody_groups) == 32, "include/nbody.h: 32 bytes");

// radius finite and >= 0, r2 = radius * radius (one fp64 multiply) finite
int groups64_r2(nbody_ctx *c, const char *who, double radius, double *r2) {
  *r2 = radius * radius;
  if (std::isfinite(radius) && radius >= 0.0 && std::isfinite(*r2)) return NBODY_OK;
  return fail(c, NBODY_ERR_INVALID, "%s: the radius must be finite and >= 0 and its square finite", who);
}

// parent == nullptr: count = the linked bodies per row — at m points (ppos: double4 each, device) or, ppos == nullptr, at the bodies
// themselves —; else the bodies' minimum parent into mn and, first round, their degree into count
int groups64_pass(nbody_ctx *c, double r2, const void *ppos, int m, const int *parent, bool first_round, int *mn, int *count) {
  nbody::Groups64Launch L;
  L.parent = parent; L.mn = mn; L.count = count; L.r2 = r2;
  return row_pass64(c, nbody::kGroups64Width, parent ? "the fp64 groups pass" : "the fp64 radius-count pass", ppos, m, L,
                    [&](const nbody::Groups64Launch &P) {
                      return parent ? nbody::launch_groups_pass_f64(P, first_round, c->stream) : nbody::launch_radius_counts_f64(P, c->stream);
                    });
}

// ---- the fp64 separation census (kernels_pairs64.hip) ----
static_assert(nbody::kPairs64Group == NBODY_PAIR_RADII_PER_PASS && NBODY_PAIR_RADII_MAX % NBODY_PAIR_RADII_PER_PASS == 0,
              "include/nbody.h states the thresholds of a pass");

// The k radii of a call as the passes take them: r2 the `distinct` DISTINCT squares ascending, kPairs64Group to a pass, and slot[q] =
// where radius q's square stands in r2.  Plain host code, no context: false where a radius is not finite and >= 0 or its square not
// finite (`*bad_q`: which).
struct PairRadii {
  double r2[NBODY_PAIR_RADII_MAX];
  int slot[NBODY_PAIR_RADII_MAX];
  int distinct = 0;
};
bool pair_radii_plan(const double *radii, int k, PairRadii *P, int *bad_q) {
  double sq[NBODY_PAIR_RADII_MAX];
  for (int q = 0; q < k; ++q) {
    sq[q] = radii[q] * radii[q];
    if (!(std::isfinite(radii[q]) && radii[q] >= 0.0 && std::isfinite(sq[q]))) { *bad_q = q; return false; }
    P->r2[q] = sq[q];
  }
  std::sort(P->r2, P->r2 + k);
  P->distinct = (int)(std::unique(P->r2, P->r2 + k) - P->r2);
  for (int q = 0; q < k; ++q) P->slot[q] = (int)(std::lower_bound(P->r2, P->r2 + P->distinct, sq[q]) - P->r2);
  return true;
}

// what both calls check of their radii and output before anything is written; the plan into *P
int pairs64_plan(nbody_ctx *c, const char *who, const double *radii, int32_t k, const int64_t *count, PairRadii *P) {
  if (!radii || !count) return fail(c, NBODY_ERR_INVALID, "%s: null radii or output", who);
  if (k < 1 || k > NBODY_PAIR_RADII_MAX) return fail(c, NBODY_ERR_INVALID, "%s: k = %d outside 1 .. %d", who, (int)k, NBODY_PAIR_RADII_MAX);
  int bad_q = 0;
  if (!pair_radii_plan(radii, k, P, &bad_q))
    return fail(c, NBODY_ERR_INVALID, "%s: radius %d must be finite and >= 0 and its square finite", who, bad_q);
  return NBODY_OK;
}

// the bytes of the staging pair behind `first` a call needs: the P.distinct totals, then the workgroups' slots of a pass
int pairs64_lanes() { return nbody::env_int("NBODY_PAIRS64_LANES", 0); }   // tests: 1 or 2 points per lane, read at every call; it enters no count
size_t pairs64_bytes(nbody_ctx *c, const PairRadii &P, bool self, int m) {
  return ((size_t)P.distinct + nbody::pairs64_partial_words(c->p.n_total, m, self, pairs64_lanes())) * 8;
}

// ceil(P.distinct / kPairs64Group) passes — over m points (ppos: double4 each, device) or, ppos == nullptr, over the ordered pairs of
// the bodies — add into the P.distinct words at `dcount` (device, inside the staging pair at byte `first`), cleared here; then read
// back in one copy and handed out in the caller's order, halved where the rows are the bodies
int pairs64_run(nbody_ctx *c, const PairRadii &P, const void *ppos, int m, size_t first, int32_t k, int64_t *count) {
  unsigned long long *dcount = (unsigned long long *)((char *)c->d_stage + first);
  const int lanes = pairs64_lanes();
  const size_t words = nbody::pairs64_partial_words(c->p.n_total, m, ppos == nullptr, lanes);
  HIP_TRY(c, hipMemsetAsync(dcount, 0, (size_t)P.distinct * 8, c->stream));
  for (int g = 0; g < P.distinct; g += nbody::kPairs64Group) {
    nbody::Pairs64Launch L;
    L.k = std::min(nbody::kPairs64Group, P.distinct - g); L.count = dcount + g;
    for (int q = 0; q < L.k; ++q) L.r2[q] = P.r2[g + q];
    L.lanes = lanes; L.partial = dcount + P.distinct; L.partial_words = words;
    if (int rc = row_pass64(c, nbody::kPairs64Width, "the fp64 pair-count pass", ppos, m, L,
                            [&](const nbody::Pairs64Launch &Q) { return nbody::launch_pair_counts_f64(Q, c->stream); }))
      return rc;
  }
  if (int rc = stage_to_host(c, first, (size_t)P.distinct * 8)) return rc;
  const unsigned long long *h = (const unsigned long long *)((const char *)c->h_stage + first);
  for (int q = 0; q < k; ++q) count[q] = (int64_t)(ppos ? h[P.slot[q]] : h[P.slot[q]] / 2);
  return NBODY_OK;
}

// ---- the fp64 minimum spanning forest (kernels_mst64.hip) ----
static_assert(sizeof(nbody_mst) == 32, "include/nbody.h: 32 bytes");

// every body's nearest body under another label: one pass
int mst64_pass(nbody_ctx *c, int n, const nbody::Mst64Work &W) {
  nbody::Mst64Launch L;
  L.label = W.label; L.index = W.near_j; L.d2 = W.near_d2;
  return row_pass64(c, nbody::kMst64Width, "the fp64 spanning-tree pass", nullptr, n, L,
                    [&](const nbody::Mst64Launch &P) { return nbody::launch_mst_pass_f64(P, c->stream); });
}

// the work area of n bodies, mst64_bytes(n) of them, carved from `base` (the staging pair's device or host side): the 8-byte arrays first.
// *out_first, *out_bytes: edge_d2, edge_i, edge_j and component, adjacent
size_t mst64_bytes(size_t n) { return 4 * n * 8 + (7 * n + 1) * 4; }
nbody::Mst64Work mst64_work(void *base, size_t n, size_t *out_first, size_t *out_bytes) {
  nbody::Mst64Work W;
  double *d = (double *)base;
  W.near_d2 = d; W.best = (unsigned long long *)(d + n); W.pair = W.best + n; W.edge_d2 = d + 3 * n;
  int *q = (int *)(d + 4 * n);
  W.edge_i = q; W.edge_j = q + n; W.component = q + 2 * n; W.label = q + 3 * n; W.near_j = q + 4 * n; W.succ = q + 5 * n; W.lowest = q + 6 * n;
  W.cursor = q + 7 * n;
  *out_first = 3 * n * 8; *out_bytes = n * 8 + 3 * n * 4;
  return W;
}

// ceil(log2 n) + 1: the components with an edge at least halve every round, and one last pass may find none
int mst64_round_bound(size_t n) {
  int bits = 0;
  while (((size_t)1 << bits) < n) ++bits;
  return bits + 1;
}

}  // namespace

extern "C" {

int nbody_potential_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, int32_t n, double *phi, size_t phi_stride) {
  return pot64_at(c, "nbody_potential_at_f64", false, pos, pos_stride, n, phi, phi_stride);
}
int nbody_get_potentials_f64(nbody_ctx *c, double *phi, size_t stride) { return pot64_get(c, "nbody_get_potentials_f64", false, phi, stride); }

int nbody_tidal_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, int32_t n, double *t6, size_t t_stride) {
  return pot64_at(c, "nbody_tidal_at_f64", true, pos, pos_stride, n, t6, t_stride);
}
int nbody_get_tidal_f64(nbody_ctx *c, double *t6, size_t stride) { return pot64_get(c, "nbody_get_tidal_f64", true, t6, stride); }

int nbody_tidal_time_f64(nbody_ctx *c, double *t_min, int32_t *body) {
  const char *who = "nbody_tidal_time_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!t_min && !body) return fail(c, NBODY_ERR_INVALID, "%s: both outputs are null", who);
  if ((rc = ensure_rows64(c, &c->tidal64, 6))) return rc;
  if ((rc = pot64_pass(c, true, nullptr, c->p.n_total, (double *)c->tidal64))) return rc;
  return tidal_time_out(c, t_min, body);
}

int nbody_get_nearest_f64(nbody_ctx *c, int32_t *index, double *d2) { return census64_get(c, "nbody_get_nearest_f64", false, index, nullptr, d2); }
int nbody_nearest_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, int32_t n, int32_t *index, double *d2) {
  return census64_at(c, "nbody_nearest_at_f64", false, pos, pos_stride, nullptr, 0, n, index, nullptr, d2);
}
int nbody_get_partners_f64(nbody_ctx *c, int32_t *index, double *energy, double *d2) {
  return census64_get(c, "nbody_get_partners_f64", true, index, energy, d2);
}
int nbody_partner_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n, int32_t *index,
                         double *energy, double *d2) {
  return census64_at(c, "nbody_partner_at_f64", true, pos, pos_stride, vel, vel_stride, n, index, energy, d2);
}

int nbody_closest_pair_f64(nbody_ctx *c, int32_t *i, int32_t *j, double *d2) {
  const char *who = "nbody_closest_pair_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!i && !j && !d2) return fail(c, NBODY_ERR_INVALID, "%s: all three outputs are null", who);
  double r[4];
  if ((rc = census64_pair(c, false, r))) return rc;
  if (i) *i = (int32_t)r[1];
  if (j) *j = (int32_t)r[2];
  if (d2) *d2 = r[0];
  return NBODY_OK;
}

int nbody_hardest_pair_f64(nbody_ctx *c, int32_t *i, int32_t *j, double *energy, double *d2) {
  const char *who = "nbody_hardest_pair_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!i && !j && !energy && !d2) return fail(c, NBODY_ERR_INVALID, "%s: all four outputs are null", who);
  double r[4];
  if ((rc = census64_pair(c, true, r))) return rc;
  if (i) *i = (int32_t)r[1];
  if (j) *j = (int32_t)r[2];
  if (energy) *energy = r[0];
  if (d2) *d2 = r[3];
  return NBODY_OK;
}

int nbody_pair_time_f64(nbody_ctx *c, double *t_min, int32_t *i, int32_t *j) {
  const char *who = "nbody_pair_time_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!t_min && !i && !j) return fail(c, NBODY_ERR_INVALID, "%s: all three outputs are null", who);
  double r[4];
  if ((rc = census64_pair(c, false, r))) return rc;
  const int32_t bi = (int32_t)r[1], bj = (int32_t)r[2];
  double t = HUGE_VAL;                                             // no pair, or a massless one
  if (bi >= 0 && bj >= 0) {                                        // the free-fall scale of the closest pair, formed here from d2 and the two masses
    double *h = (double *)c->h_stage;
    HIP_TRY(c, hipMemcpyAsync(h, (const double *)c->posm + 4 * (size_t)bi + 3, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h + 1, (const double *)c->posm + 4 * (size_t)bj + 3, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double gm = c->p.G * (h[0] + h[1]);
    if (gm > 0.0) t = std::sqrt(r[0] * std::sqrt(r[0]) / gm);
  }
  if (t_min) *t_min = t;
  if (i) *i = bi;
  if (j) *j = bj;
  return NBODY_OK;
}

int nbody_get_neighbours_f64(nbody_ctx *c, int32_t k, int32_t *index, double *d2) {
  const char *who = "nbody_get_neighbours_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if ((rc = neighbours64_k(c, who, k, 1))) return rc;
  if (!index && !d2) return fail(c, NBODY_ERR_INVALID, "%s: every output is null", who);
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * k * 12))) return rc;
  return neighbours64_lists(c, k, nullptr, 0, n, index, d2);
}

int nbody_neighbours_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, int32_t n, int32_t k, int32_t *index, double *d2) {
  const char *who = "nbody_neighbours_at_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if ((rc = neighbours64_k(c, who, k, 1))) return rc;
  if (n < 0 || !pos || pos_stride < 24 || (!index && !d2))
    return fail(c, NBODY_ERR_INVALID, "%s: null points, n < 0, every output null, or a stride < 24", who);
  if (n == 0) return NBODY_OK;
  Staged64 s;
  if ((rc = stage_points64(c, pos, pos_stride, nullptr, 0, false, (size_t)n, (size_t)n * k * 12, &s))) return rc;
  return neighbours64_lists(c, k, s.d, s.skip, s.m, index, d2);
}

int nbody_get_density_f64(nbody_ctx *c, int32_t k, double *rho, double *rk2) {
  const char *who = "nbody_get_density_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if ((rc = neighbours64_k(c, who, k, 2))) return rc;
  if (!rho && !rk2) return fail(c, NBODY_ERR_INVALID, "%s: every output is null", who);
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * 16))) return rc;
  double *d = (double *)c->d_stage;
  if ((rc = neighbours64_pass(c, k, nullptr, (int)n, nullptr, nullptr, d, d + n))) return rc;
  if ((rc = stage_to_host(c, 0, n * 16))) return rc;
  if (rho) memcpy(rho, c->h_stage, n * 8);
  if (rk2) memcpy(rk2, (const double *)c->h_stage + n, n * 8);
  return NBODY_OK;
}

int nbody_density_centre_f64(nbody_ctx *c, int32_t k, nbody_core *out) {
  const char *who = "nbody_density_centre_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if ((rc = neighbours64_k(c, who, k, 2))) return rc;
  if (!out || out->struct_size != sizeof(nbody_core)) return fail(c, NBODY_ERR_INVALID, "%s: null output or struct_size != sizeof(nbody_core)", who);
  const size_t n = (size_t)c->p.n_total, slots = (size_t)nbody::energy_fast_slots((int)n);
  const size_t skip = 8 * slots + 16;                            // the reductions' partials and their nine doubles, ahead of the densities
  if ((rc = ensure_stage(c, (skip + n) * sizeof(double)))) return rc;
  double *partials = (double *)c->d_stage, *red = partials + 8 * slots, *rho = partials + skip;
  if ((rc = neighbours64_pass(c, k, nullptr, (int)n, nullptr, nullptr, rho, nullptr))) return rc;
  HIP_TRY(c, nbody::launch_density_centre(c->posm, rho, (int)n, partials, red, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, red, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double *r = (const double *)c->h_stage;
  out->k = k; out->used = (int32_t)r[4]; out->densest = (int32_t)r[6];
  out->rho_max = r[5];
  out->centre[0] = r[1]; out->centre[1] = r[2]; out->centre[2] = r[3];
  out->core_radius = r[8]; out->rho_sum = r[0]; out->rho2_sum = r[7];
  return NBODY_OK;
}

int nbody_radial_order_f64(nbody_ctx *c, const double centre[3], int32_t *order, double *d2, double *mass_cum, int32_t *n_finite) {
  const char *who = "nbody_radial_order_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!radial64_centre_ok(centre)) return fail(c, NBODY_ERR_INVALID, "%s: null centre or a centre that is not finite", who);
  if (!order && !d2 && !mass_cum && !n_finite) return fail(c, NBODY_ERR_INVALID, "%s: every output is null", who);
  nbody::Radial64Work W;
  if ((rc = radial64_run(c, centre, nullptr, 0, &W))) return rc;
  const size_t n = (size_t)c->p.n_total;
  const char *d = (const char *)c->d_stage;
  char *h = (char *)c->h_stage;
  if (order) HIP_TRY(c, hipMemcpyAsync(h + W.idx[0], d + W.idx[0], n * 4, hipMemcpyDeviceToHost, c->stream));
  if (d2) HIP_TRY(c, hipMemcpyAsync(h + W.key[0], d + W.key[0], n * 8, hipMemcpyDeviceToHost, c->stream));
  if (mass_cum) HIP_TRY(c, hipMemcpyAsync(h + W.cum, d + W.cum, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (n_finite) HIP_TRY(c, hipMemcpyAsync(h + W.n_finite, d + W.n_finite, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (order) memcpy(order, h + W.idx[0], n * 4);
  if (d2) memcpy(d2, h + W.key[0], n * 8);                         // (the sorted keys are the bit patterns of d2; a NaN reads all ones)
  if (mass_cum) memcpy(mass_cum, h + W.cum, n * 8);
  if (n_finite) memcpy(n_finite, h + W.n_finite, 4);
  return NBODY_OK;
}

int nbody_lagrange_radii_f64(nbody_ctx *c, const double centre[3], const double *fractions, int32_t k, nbody_lagrange *rows,
                             double *total_mass) {
  const char *who = "nbody_lagrange_radii_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!radial64_centre_ok(centre)) return fail(c, NBODY_ERR_INVALID, "%s: null centre or a centre that is not finite", who);
  if (!fractions || !rows) return fail(c, NBODY_ERR_INVALID, "%s: null fractions or rows", who);
  if (k < 1 || k > NBODY_LAGRANGE_MAX) return fail(c, NBODY_ERR_INVALID, "%s: k = %d outside 1 .. %d", who, k, NBODY_LAGRANGE_MAX);
  for (int q = 0; q < k; ++q)
    if (!(fractions[q] > 0.0 && fractions[q] <= 1.0))              // (a NaN fails both)
      return fail(c, NBODY_ERR_INVALID, "%s: fraction %d is outside (0, 1]", who, q);
  nbody::Radial64Work W;
  if ((rc = radial64_run(c, centre, fractions, k, &W))) return rc;
  const char *d = (const char *)c->d_stage;
  char *h = (char *)c->h_stage;
  HIP_TRY(c, hipMemcpyAsync(h + W.rows, d + W.rows, (size_t)k * sizeof(nbody_lagrange), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + W.total, d + W.total, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(rows, h + W.rows, (size_t)k * sizeof(nbody_lagrange));
  if (total_mass) memcpy(total_mass, h + W.total, 8);
  return NBODY_OK;
}

int nbody_get_radius_counts_f64(nbody_ctx *c, double radius, int32_t *count) {
  const char *who = "nbody_get_radius_counts_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  double r2;
  if ((rc = groups64_r2(c, who, radius, &r2))) return rc;
  if (!count) return fail(c, NBODY_ERR_INVALID, "%s: null output", who);
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * 4))) return rc;
  if ((rc = groups64_pass(c, r2, nullptr, (int)n, nullptr, false, nullptr, (int *)c->d_stage))) return rc;
  if ((rc = stage_to_host(c, 0, n * 4))) return rc;
  memcpy(count, c->h_stage, n * 4);
  return NBODY_OK;
}

int nbody_radius_counts_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, int32_t n, double radius, int32_t *count) {
  const char *who = "nbody_radius_counts_at_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  double r2;
  if ((rc = groups64_r2(c, who, radius, &r2))) return rc;
  if (n < 0 || !pos || pos_stride < 24 || !count) return fail(c, NBODY_ERR_INVALID, "%s: null points or output, n < 0, or a stride < 24", who);
  if (n == 0) return NBODY_OK;
  Staged64 s;
  if ((rc = stage_points64(c, pos, pos_stride, nullptr, 0, false, (size_t)n, (size_t)n * 4, &s))) return rc;
  if ((rc = groups64_pass(c, r2, s.d, n, nullptr, false, nullptr, (int *)(s.d + s.skip)))) return rc;
  if ((rc = stage_to_host(c, s.skip * 8, s.m * 4))) return rc;
  memcpy(count, s.h + s.skip, s.m * 4);
  return NBODY_OK;
}

// The rounds are driven from here: pass and fold, hook, compress, then a 4-byte read-back of `changed`.  The first round that changes
// nothing is the last.  Every round but the last merges at least two components, so there are at most n of them.
int nbody_get_groups_f64(nbody_ctx *c, double radius, int32_t *label, int32_t *members, int32_t *degree, nbody_groups *summary) {
  const char *who = "nbody_get_groups_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  double r2;
  if ((rc = groups64_r2(c, who, radius, &r2))) return rc;
  if (!label && !members && !degree && !summary) return fail(c, NBODY_ERR_INVALID, "%s: every output is null", who);
  const size_t n = (size_t)c->p.n_total;
  // ints of the staging pair: label, members, degree (read back together), hooked, mn, size; then four 64-bit sums and `changed`
  const size_t sums = (6 * n + 1) / 2 * 2, flag = sums + 8, ints = flag + 2;
  if ((rc = ensure_stage(c, ints * 4))) return rc;
  int *d = (int *)c->d_stage, *h = (int *)c->h_stage;
  int *parent = d, *dmembers = d + n, *ddegree = d + 2 * n, *hooked = d + 3 * n, *mn = d + 4 * n, *size = d + 5 * n;
  HIP_TRY(c, nbody::launch_groups_identity(parent, (int)n, c->stream));
  size_t rounds = 0;
  for (;;) {
    if (rounds == n) return fail(c, NBODY_ERR_INTERNAL, "%s: no fixed point after %zu rounds of %zu bodies", who, rounds, n);
    if ((rc = groups64_pass(c, r2, nullptr, (int)n, parent, rounds == 0, mn, ddegree))) return rc;
    ++rounds;
    HIP_TRY(c, nbody::launch_groups_merge(parent, mn, hooked, (int)n, d + flag, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h + flag, d + flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h[flag] == 0) break;
  }
  HIP_TRY(c, nbody::launch_groups_members(parent, ddegree, (int)n, size, dmembers, (unsigned long long *)(d + sums), c->stream));
  HIP_TRY(c, hipMemcpyAsync(h, d, 3 * n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + sums, d + sums, 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (label) memcpy(label, h, n * 4);
  if (members) memcpy(members, h + n, n * 4);
  if (degree) memcpy(degree, h + 2 * n, n * 4);
  if (summary) {
    unsigned long long s[4];
    memcpy(s, h + sums, 32);
    summary->groups = (int32_t)s[0]; summary->multiples = (int32_t)s[1];
    summary->largest = (int32_t)(0x7fffffffull - (s[3] & 0xffffffffull)); summary->largest_members = (int32_t)(s[3] >> 32);
    summary->rounds = (int32_t)rounds; summary->reserved = 0;
    summary->links = (int64_t)(s[2] / 2);
  }
  return NBODY_OK;
}

int nbody_get_pair_counts_f64(nbody_ctx *c, const double *radii, int32_t k, int64_t *count) {
  const char *who = "nbody_get_pair_counts_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  PairRadii P;
  if ((rc = pairs64_plan(c, who, radii, k, count, &P))) return rc;
  if ((rc = ensure_stage(c, pairs64_bytes(c, P, true, c->p.n_total)))) return rc;
  return pairs64_run(c, P, nullptr, c->p.n_total, 0, k, count);
}

int nbody_pair_counts_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, int32_t n, const double *radii, int32_t k, int64_t *count) {
  const char *who = "nbody_pair_counts_at_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  PairRadii P;
  if ((rc = pairs64_plan(c, who, radii, k, count, &P))) return rc;
  if (n < 0 || !pos || pos_stride < 24) return fail(c, NBODY_ERR_INVALID, "%s: null points, n < 0, or a stride < 24", who);
  if (n == 0) {
    for (int q = 0; q < k; ++q) count[q] = 0;
    return NBODY_OK;
  }
  Staged64 s;
  if ((rc = stage_points64(c, pos, pos_stride, nullptr, 0, false, (size_t)n, pairs64_bytes(c, P, false, n), &s))) return rc;
  return pairs64_run(c, P, s.d, n, s.skip * 8, k, count);
}

// The Boruvka rounds are driven from here: clear, pass and fold, pick, hook, compress, then a 4-byte read-back of the edges so far.  No
// pass is made once n - 1 edges are there; a round that appends none is the last and is counted.  NBODY_MST_PHASES=1 (read at every call;
// tools/mst_f64_measure.py): the host clock round the rounds, the read-back and the sort, printed to stderr.
int nbody_get_mst_f64(nbody_ctx *c, int32_t *i, int32_t *j, double *d2, int32_t *component, nbody_mst *summary) {
  const char *who = "nbody_get_mst_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!i && !j && !d2 && !component && !summary) return fail(c, NBODY_ERR_INVALID, "%s: every output is null", who);
  const size_t n = (size_t)c->p.n_total;
  size_t out_first, out_bytes;
  if ((rc = ensure_stage(c, mst64_bytes(n)))) return rc;
  const nbody::Mst64Work W = mst64_work(c->d_stage, n, &out_first, &out_bytes);
  const nbody::Mst64Work H = mst64_work(c->h_stage, n, &out_first, &out_bytes);
  const auto clock = [] { return std::chrono::steady_clock::now(); };
  const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  const auto t0 = clock();
  HIP_TRY(c, nbody::launch_mst_begin(W, (int)n, c->stream));
  const int bound = mst64_round_bound(n);
  int rounds = 0;
  size_t edges = 0;
  while (edges + 1 < n) {
    if (rounds == bound) return fail(c, NBODY_ERR_INTERNAL, "%s: %zu components of %zu bodies left after %d rounds", who, n - edges, n, rounds);
    HIP_TRY(c, nbody::launch_mst_clear(W, (int)n, c->stream));
    if ((rc = mst64_pass(c, (int)n, W))) return rc;
    ++rounds;
    HIP_TRY(c, nbody::launch_mst_merge(W, (int)n, c->stream));
    HIP_TRY(c, hipMemcpyAsync(H.cursor, W.cursor, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t now = (size_t)*H.cursor;
    if (now >= n) return fail(c, NBODY_ERR_INTERNAL, "%s: %zu edges among %zu bodies", who, now, n);
    if (now == edges) break;
    edges = now;
  }
  const auto t1 = clock();
  HIP_TRY(c, nbody::launch_mst_components(W, (int)n, c->stream));
  if ((rc = stage_to_host(c, out_first, out_bytes))) return rc;
  const auto t2 = clock();
  struct Edge { double d2; int32_t lo, hi; };
  std::vector<Edge> e(edges);
  for (size_t k = 0; k < edges; ++k) e[k] = Edge{H.edge_d2[k], H.edge_i[k], H.edge_j[k]};
  std::sort(e.begin(), e.end(), [](const Edge &a, const Edge &b) {
    return a.d2 != b.d2 ? a.d2 < b.d2 : a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
  });
  const auto t3 = clock();
  const char *env = getenv("NBODY_MST_PHASES");
  if (env && env[0] == '1')
    fprintf(stderr, "mst_f64 phases: n %zu rounds %d loop %.4f readback %.4f sort %.4f ms\n", n, rounds, ms(t0, t1), ms(t1, t2), ms(t2, t3));
  double length = 0.0;
  for (size_t k = 0; k + 1 < n; ++k) {
    const bool edge = k < edges;
    if (i) i[k] = edge ? e[k].lo : -1;
    if (j) j[k] = edge ? e[k].hi : -1;
    if (d2) d2[k] = edge ? e[k].d2 : HUGE_VAL;
    if (edge) length += std::sqrt(e[k].d2);
  }
  if (component) memcpy(component, H.component, n * 4);
  if (summary) {
    summary->edges = (int32_t)edges; summary->components = (int32_t)(n - edges); summary->rounds = rounds; summary->reserved = 0;
    summary->length = length; summary->longest_d2 = edges ? e[edges - 1].d2 : 0.0;
  }
  return NBODY_OK;
}
}  // extern "C"
