// The Hermite calls of the C-ABI (include/nbody.h) on fp64 contexts: fourth- and sixth-order shared steps, their block sessions and their
// fp64 tracers, beside the snap and the jerk and snap at fp64 points they are built on (the other fp64 queries: capi_query64.hip).  Host
// C++ like capi.hip; what it shares with the other host units: capi_common.h.  One driver, written once as function templates over an order's traits (Order4, Order6: what truly differs between
// the two schemes, each rule with its comment — DESIGN.md has the table); the extern "C" functions pick the instantiation.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_common.h"
#include "ctx.h"
#include "hermite_block_level.h"

namespace {

using nbody::check_ready; using nbody::ensure_rows64; using nbody::ensure_probe_part; using nbody::ensure_stage; using nbody::fail; using nbody::gather4; using nbody::points64_part_holds; using nbody::points64_ready; using nbody::stage_points64; using nbody::stage_to_host; using nbody::Staged64; using nbody::hermite_invalidate; using nbody::hermite_invalidate_order; using nbody::HermiteBlockSession; using nbody::HermiteCache; using nbody::kSnapRowWidth; using nbody::multi_unsupported; using nbody::queue_body_jerk; using nbody::read_energy; using nbody::scatter_records; using nbody::timed_launch;

// where the stepping exists — fp64 state, one device, all bodies (such contexts are at theta == 0) — and when: a state set, no step half done
int hermite_ready(nbody_ctx *c, const char *who) {
  if (c && c->multi) return multi_unsupported(c, who);
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->p.precision != NBODY_PREC_F64)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context whose state is fp32 (NBODY_PREC_F32, NBODY_PREC_F32_KAHAN): the corrector's "
                "differences a0 - a1 need fp64 state; create the context with NBODY_PREC_F64", who);
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  if (c->theta > 0.0f) return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not at theta > 0 (the jerk is a pair sum)", who);
  if (c->step_open || c->step_local) return fail(c, NBODY_ERR_STATE, "%s: a step is open (nbody_step_end first)", who);
  return NBODY_OK;
}

// ---- the evaluation passes, each queued as one pass under NBODY_KERNEL_FORCES ----
// a pass is never queued into a staging area that does not hold its partial rows
int probe_part_holds(nbody_ctx *c, int width, const char *what) {
  const size_t need = nbody::probe_part_elems(c->p.n_total, c->p.n_total, width);
  if (c->probe_part && c->probe_part_elems >= need) return NBODY_OK;
  return fail(c, NBODY_ERR_STATE, "%s: the partial rows need %zu float4, the staging area holds %zu", what, need, c->probe_part_elems);
}

// (a, j) of the bodies at (posm, vel) — the live state or the predicted one — into aj64: nbody_get_jerk_f64's pass and fold with the same
// geometry, a function of n_total alone
int jerk_evaluate(nbody_ctx *c, const void *posm, const void *vel, double *aj64) {
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
    nbody::JerkLaunch L;
    L.posm = posm; L.vel = vel; L.part = c->probe_part; L.aj64 = aj64;
    L.n_total = c->p.n_total; L.m = c->p.n_total; L.precision = NBODY_PREC_F64; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
    HIP_TRY(c, nbody::launch_jerk(L, c->stream));
    return NBODY_OK;
  });
}

// (a, j, s) of the bodies at (posm, vel) given the input accelerations ain into ajs64: the kernel, fold and geometry (a function of
// n_total alone) of nbody_get_snap_f64
int snap_evaluate(nbody_ctx *c, const void *posm, const void *vel, const double *ain, int ain_stride, double *ajs64) {
  if (int rc = probe_part_holds(c, kSnapRowWidth, "the snap pass")) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
    nbody::SnapLaunch L;
    L.posm = posm; L.vel = vel; L.ain = ain; L.ain_stride = ain_stride; L.part = c->probe_part; L.ajs64 = ajs64;
    L.n_total = c->p.n_total; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
    HIP_TRY(c, nbody::launch_snap(L, c->stream));
    return NBODY_OK;
  });
}

// (a, j) at m points (ppos, pvel: double4 each, device) in the field of the bodies at (posm, vel) into aj64 ([m][6])
int points64_jerk(nbody_ctx *c, const void *posm, const void *vel, const void *ppos, const void *pvel, int m, double *aj64) {
  if (int rc = points64_part_holds(c, m, 3, "the point jerk pass")) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
    nbody::Points64Launch L;
    L.posm = posm; L.vel = vel; L.ppos = ppos; L.pvel = pvel; L.part = c->probe_part; L.part_elems = c->probe_part_elems; L.out = aj64;
    L.n_total = c->p.n_total; L.m = m; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
    HIP_TRY(c, nbody::launch_jerk_points_f64(L, c->stream));
    return NBODY_OK;
  });
}

// (a, j, s) the same way, given the bodies' input accelerations (ain) and the points' (pain), into ajs64 ([m][9])
int points64_snap(nbody_ctx *c, const void *posm, const void *vel, const double *ain, int ain_stride, const void *ppos, const void *pvel,
                  const double *pain, int pain_stride, int m, double *ajs64) {
  if (int rc = points64_part_holds(c, m, kSnapRowWidth, "the point snap pass")) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
    nbody::Points64Launch L;
    L.posm = posm; L.vel = vel; L.ain = ain; L.ain_stride = ain_stride; L.ppos = ppos; L.pvel = pvel; L.pain = pain; L.pain_stride = pain_stride;
    L.part = c->probe_part; L.part_elems = c->probe_part_elems; L.out = ajs64;
    L.n_total = c->p.n_total; L.m = m; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
    HIP_TRY(c, nbody::launch_snap_points_f64(L, c->stream));
    return NBODY_OK;
  });
}

// ---- a cache's arrays (the layout: HermiteCache in ctx.h) ----
struct CacheView {
  HermiteCache *h;
  void *pos, *vel, *acc;   // what the cache steps: the bodies' live state, or the tracers' state
  double *pred;            // xp, vp (sixth order: ap), [count] double4 each, side by side
  double *d;               // the higher derivatives, [count] double4 each, side by side
  double *row[2];          // [0]: the evaluated derivatives of the stored state (row `cur`), [1]: the other row
  double *partials;
  int count;
};
template <class O>
CacheView view_of(HermiteCache &h, void *pos, void *vel, void *acc, double *pred, double *d, int count) {
  const size_t m = (size_t)count;
  double *rows = d + 4 * O::kDerivs * m;
  return CacheView{&h, pos, vel, acc, pred, d, {rows + h.cur * O::kRow * m, rows + (h.cur ^ 1) * O::kRow * m}, rows + 2 * O::kRow * m, count};
}
template <class O>
CacheView body_view(nbody_ctx *c) {
  double *b = (double *)c->hm[O::index].buf;
  return view_of<O>(c->hm[O::index], c->posm, c->vel, c->acc, b, b + 4 * O::kPred * (size_t)c->p.n_total, c->p.n_total);
}
// The fp64 tracers (nbody_set_tracers_f64; kernels_points64.hip): massless points with a state and caches of their own.  They are
// predicted with the step's dt, evaluated by the point kernels in the field of the bodies' PREDICTED state — the field the bodies' own
// evaluation uses — and corrected by the bodies' kernels on the tracers' arrays.  Nothing of theirs is read by anything the bodies get.
template <class O>
CacheView tracer_view(nbody_ctx *c) {
  const size_t m = (size_t)c->tr64_n;
  double *t = (double *)c->tr64;                                   // pos, vel, acc, xp, vp, ap
  return view_of<O>(c->trh[O::index], t, t + 4 * m, t + 8 * m, t + 12 * m, (double *)c->trh[O::index].buf, c->tr64_n);
}

// ---- what differs between the two orders ----
struct Order4 {
  static constexpr int index = 0;
  static constexpr int kRow = 6, kDerivs = 2, kPred = 2;           // (a, j) per row; a2, a3; xp, vp
  static constexpr int kPartWidth = 3;                             // the jerk pass's partial rows, in float4
  static constexpr const char *kPrefix = "nbody_hermite", *kOrdinal = "", *kLanesEnv = "NBODY_HERMITE_BLOCK_LANES";
  // A start leaves a2, a3 as they are: nbody_hermite_get substitutes zeros unless `derivs` is set or a session is active, and
  // nbody_hermite_block_begin zeroes them when `derivs` is not set.
  static constexpr bool kStartZeroes = false;
  // nbody_hermite_step, nbody_hermite_advance and nbody_hermite_block_begin forget the sixth-order cache ONCE, after entering.
  static constexpr bool kForgetsOtherEveryStep = false;
  // the tracers' start reads the stored bodies' (x, v) alone: nbody_hermite_tracers_timescale needs no cache of the bodies'
  static constexpr bool kTracerStartReadsCache = false;

  static int reserve_parts(nbody_ctx *c, int m) { return ensure_probe_part(c, m, 3); }
  // (a0, j0) of the stored state: one jerk pass
  static int start(nbody_ctx *c, const CacheView &b) { return jerk_evaluate(c, c->posm, c->vel, b.row[0]); }
  static int start_points(nbody_ctx *c, const CacheView &t) { return points64_jerk(c, c->posm, c->vel, t.pos, t.vel, t.count, t.row[0]); }
  // the predicted state's (a1, j1); the tracers' in the field of the bodies' predicted state
  static int evaluate(nbody_ctx *c, const CacheView &b) { return jerk_evaluate(c, b.pred, b.pred + 4 * (size_t)b.count, b.row[1]); }
  static int evaluate_points(nbody_ctx *c, const CacheView &b, const CacheView &t) {
    return points64_jerk(c, b.pred, b.pred + 4 * (size_t)b.count, t.pred, t.pred + 4 * (size_t)t.count, t.count, t.row[1]);
  }

  using Launch = nbody::HermiteLaunch;
  using BlockLaunch = nbody::HermiteBlockLaunch;
  template <class L>
  static void fill(L &l, const CacheView &v) {
    const size_t n = (size_t)v.count;
    l.posm = v.pos; l.vel = v.vel; l.acc = v.acc; l.xp = v.pred; l.vp = v.pred + 4 * n; l.aj0 = v.row[0]; l.a2 = v.d; l.a3 = v.d + 4 * n;
  }
  static Launch step_launch(const CacheView &v, double dt) { Launch l; fill(l, v); l.aj1 = v.row[1]; l.n = v.count; l.dt = dt; return l; }
  static BlockLaunch block_launch(const CacheView &v, double eta) { BlockLaunch l; fill(l, v); l.root_eta = std::sqrt(eta); return l; }
  static constexpr auto predict = nbody::launch_hermite_predict, correct = nbody::launch_hermite_correct;
  static constexpr auto block_init = nbody::launch_hermite_block_init;
  static constexpr auto block_schedule = nbody::launch_hermite_block_schedule;
  static constexpr auto block_schedule_joint = nbody::launch_hermite_block_schedule_joint;
  static constexpr auto block_evaluate = nbody::launch_hermite_block_evaluate;
  static constexpr auto block_correct = nbody::launch_hermite_block_correct;
  // the rows of the listed tracers P.list[first .. first + m) at the bodies' predicted (xp, vp)
  static hipError_t block_evaluate_points(nbody_ctx *c, const BlockLaunch &B, const BlockLaunch &P, int first, int m, int lanes) {
    nbody::Points64Launch L;
    L.posm = B.xp; L.vel = B.vp; L.ppos = P.xp; L.pvel = P.vp; L.part = c->probe_part; L.part_elems = c->probe_part_elems;
    L.n_total = B.n; L.m = m; L.lanes = lanes; L.G = B.G; L.eps2 = B.eps2;
    return nbody::launch_jerk_points_list_f64(L, P.list + first, c->stream);
  }

  // Aarseth's criterion with a step's a2, a3, |j|^2 / |a|^2 without: k is the inverse square of a time either way, and a step is
  // dt = sqrt(eta) t (at a start: eta_start t)
  static hipError_t launch_time(const CacheView &v, bool derivs, double *out, hipStream_t s) {
    return derivs ? nbody::launch_hermite_time(v.row[0], v.d, v.d + 4 * (size_t)v.count, v.count, v.partials, out, s)
                  : nbody::launch_jerk_time(v.row[0], v.count, v.partials, out, s);
  }
  static double time_of(double k, bool) { return 1.0 / std::sqrt(k); }
  static double dt_factor(double eta) { return std::sqrt(eta); }

  static const char *tick_refused(double tick) { return std::isnormal(tick) ? nullptr : "is not a normal number"; }
  static int block_parts_hold(nbody_ctx *) { return NBODY_OK; }   // (the partial rows of reserve_parts(n))
};

struct Order6 {
  static constexpr int index = 1;
  static constexpr int kRow = 9, kDerivs = 3, kPred = 3;           // (a, j, s) per row; a3, a4, a5; xp, vp, ap
  static constexpr int kPartWidth = kSnapRowWidth;                 // the snap pass's partial rows, in float4
  static constexpr const char *kPrefix = "nbody_hermite6", *kOrdinal = "sixth-order ", *kLanesEnv = "NBODY_HERMITE6_BLOCK_LANES";
  // A start zeroes a3, a4, a5 (the predictor reads a3) and clears `derivs`.
  static constexpr bool kStartZeroes = true;
  // Every sixth-order step forgets the fourth-order cache (nbody_hermite6_block_begin: once).
  static constexpr bool kForgetsOtherEveryStep = true;
  // the tracers' start reads the bodies' cached a0: nbody_hermite6_tracers_timescale enters the bodies' cache first
  static constexpr bool kTracerStartReadsCache = true;

  // the partial rows of BOTH passes a start runs: the staging area only grows, and neither width's need covers the other's (the slabs
  // are whole multiples of 1024 points: at N = 65536 the jerk pass's rows take 16 515 072 float4, the snap pass's 16 384 000)
  static int reserve_parts(nbody_ctx *c, int m) {
    if (int rc = ensure_probe_part(c, m, 3)) return rc;
    return ensure_probe_part(c, m, kSnapRowWidth);
  }
  // (a0, j0, s0) of the stored state: one jerk pass for a — its six doubles per body in the row a step overwrites —, one snap pass with
  // that a as its input
  static int start(nbody_ctx *c, const CacheView &b) {
    if (int rc = probe_part_holds(c, 3, "the jerk pass of a sixth-order start")) return rc;
    if (int rc = jerk_evaluate(c, c->posm, c->vel, b.row[1])) return rc;
    return snap_evaluate(c, c->posm, c->vel, b.row[1], 6, b.row[0]);
  }
  // the same at the tracers — a point jerk pass, then a point snap pass — with the bodies' cached a0 (the input accelerations of the
  // bodies' own next step: at a start the bodies' jerk pass's, in every bit) as the bodies' input: strides 9 and 6
  static int start_points(nbody_ctx *c, const CacheView &t) {
    if (int rc = points64_jerk(c, c->posm, c->vel, t.pos, t.vel, t.count, t.row[1])) return rc;
    return points64_snap(c, c->posm, c->vel, body_view<Order6>(c).row[0], 9, t.pos, t.vel, t.row[1], 6, t.count, t.row[0]);
  }
  // the predicted state's (a1, j1, s1), the predicted accelerations (double4 rows: stride 4) as the input; the tracers' at the bodies'
  // predicted (xp, vp, ap) with their own predicted accelerations
  static int evaluate(nbody_ctx *c, const CacheView &b) {
    const size_t n = (size_t)b.count;
    return snap_evaluate(c, b.pred, b.pred + 4 * n, b.pred + 8 * n, 4, b.row[1]);
  }
  static int evaluate_points(nbody_ctx *c, const CacheView &b, const CacheView &t) {
    const size_t n = (size_t)b.count, m = (size_t)t.count;
    return points64_snap(c, b.pred, b.pred + 4 * n, b.pred + 8 * n, 4, t.pred, t.pred + 4 * m, t.pred + 8 * m, 4, t.count, t.row[1]);
  }

  using Launch = nbody::Hermite6Launch;
  using BlockLaunch = nbody::Hermite6BlockLaunch;
  template <class L>
  static void fill(L &l, const CacheView &v) {
    const size_t n = (size_t)v.count;
    l.posm = v.pos; l.vel = v.vel; l.acc = v.acc; l.xp = v.pred; l.vp = v.pred + 4 * n; l.ap = v.pred + 8 * n; l.ajs0 = v.row[0];
    l.a3 = v.d; l.a4 = v.d + 4 * n; l.a5 = v.d + 8 * n;
  }
  static Launch step_launch(const CacheView &v, double dt) { Launch l; fill(l, v); l.ajs1 = v.row[1]; l.n = v.count; l.dt = dt; return l; }
  static BlockLaunch block_launch(const CacheView &v, double eta) { BlockLaunch l; fill(l, v); l.eta = eta; return l; }
  static constexpr auto predict = nbody::launch_hermite6_predict, correct = nbody::launch_hermite6_correct;
  static constexpr auto block_init = nbody::launch_hermite6_block_init;
  static constexpr auto block_schedule = nbody::launch_hermite6_block_schedule;
  static constexpr auto block_schedule_joint = nbody::launch_hermite6_block_schedule_joint;
  static constexpr auto block_evaluate = nbody::launch_hermite6_block_evaluate;
  static constexpr auto block_correct = nbody::launch_hermite6_block_correct;
  // the rows of the listed tracers P.list[first .. first + m) at the bodies' predicted (xp, vp, ap), each with its own predicted ap
  static hipError_t block_evaluate_points(nbody_ctx *c, const BlockLaunch &B, const BlockLaunch &P, int first, int m, int lanes) {
    nbody::Points64Launch L;
    L.posm = B.xp; L.vel = B.vp; L.ain = (const double *)B.ap; L.ain_stride = 4; L.ppos = P.xp; L.pvel = P.vp;
    L.pain = (const double *)P.ap; L.pain_stride = 4; L.part = c->probe_part; L.part_elems = c->probe_part_elems;
    L.n_total = B.n; L.m = m; L.lanes = lanes; L.G = B.G; L.eps2 = B.eps2;
    return nbody::launch_snap_points_list_f64(L, P.list + first, c->stream);
  }

  // (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2) with a step's derivatives — the inverse SIXTH power of a time —, |j|^2 / |a|^2
  // without; a step is dt = eta t (eta times t itself: no square root in this criterion; at a start: eta_start t)
  static hipError_t launch_time(const CacheView &v, bool derivs, double *out, hipStream_t s) {
    const size_t n = (size_t)v.count;
    return nbody::launch_hermite6_time(v.row[0], v.d, v.d + 4 * n, v.d + 8 * n, v.count, derivs, v.partials, out, s);
  }
  static double time_of(double k, bool derivs) { return derivs ? 1.0 / std::cbrt(std::sqrt(k)) : 1.0 / std::sqrt(k); }
  static double dt_factor(double eta) { return eta; }

  static const char *tick_refused(double tick) {
    return std::isnormal(tick) && std::isnormal((tick * tick) * tick) ? nullptr : "or its cube, which the level rule compares, is not a normal number";
  }
  static int block_parts_hold(nbody_ctx *c) { return probe_part_holds(c, kSnapRowWidth, "the snap pass of a block step"); }
};

// ---- the shared-step driver ----
// A shared-step call, or a new begin, on a context with a block session of either order: in mid-frame the bodies are at times of their
// own and nothing but that session's block_advance can move them on; at a frame end the stored state is synchronised, the cache is every
// body's, and the session simply ends.
template <class O>
int block_leave(nbody_ctx *c, const char *who, bool end = true) {
  HermiteBlockSession &s = c->hb[O::index];
  if (!s.active) return NBODY_OK;
  if (s.ticks & ((1ll << s.levels) - 1))
    return fail(c, NBODY_ERR_STATE, "%s: a %sHermite block session is in mid-frame (tick %lld of frames of %lld): the bodies are at times of "
                "their own; %s_block_advance(ctx, 1, ...) finishes the frame, nbody_hermite_restart abandons the session", who, O::kOrdinal,
                (long long)s.ticks, 1ll << s.levels, O::kPrefix);
  if (end) s.active = false;
  return NBODY_OK;
}
int block_leave_both(nbody_ctx *c, const char *who, bool end = true) {
  if (int rc = block_leave<Order4>(c, who, end)) return rc;
  return block_leave<Order6>(c, who, end);
}

// what every call does at entry: the cache and the partial rows at first use; once somebody else may write the state, nothing cached is
// believed; then the evaluated derivatives of the stored (x, v), if they are not valid
template <class O>
int enter(nbody_ctx *c) {
  HermiteCache &h = c->hm[O::index];
  const size_t n = (size_t)c->p.n_total;
  if (!h.buf) HIP_TRY(c, hipMalloc(&h.buf, ((4 * (O::kPred + O::kDerivs) + 2 * O::kRow) * n + 2 * (size_t)nbody::energy_fast_slots((int)n)) * sizeof(double)));
  if (int rc = O::reserve_parts(c, (int)n)) return rc;
  if (c->hm_external) hermite_invalidate(c);
  if (h.valid) return NBODY_OK;
  const CacheView b = body_view<O>(c);
  if (int rc = O::start(c, b)) return rc;
  if constexpr (O::kStartZeroes) {
    HIP_TRY(c, hipMemsetAsync(b.d, 0, 4 * O::kDerivs * n * sizeof(double), c->stream));
    h.derivs = false;
  }
  h.valid = true;
  return NBODY_OK;
}

// what a shared-step call does for the fp64 tracers behind enter (which has applied the hm_external rule): the cache and the partial rows
// at first use; the evaluated derivatives of the stored tracers in the stored bodies' field when they are not valid, and zeros for the
// higher ones
template <class O>
int tracers_enter(nbody_ctx *c) {
  const int m = c->tr64_n;
  if (m <= 0) return NBODY_OK;
  HermiteCache &h = c->trh[O::index];
  if (!h.buf) HIP_TRY(c, hipMalloc(&h.buf, ((4 * O::kDerivs + 2 * O::kRow) * (size_t)m + 2 * (size_t)nbody::energy_fast_slots(m)) * sizeof(double)));
  if (int rc = O::reserve_parts(c, m)) return rc;
  if (h.valid) return NBODY_OK;
  const CacheView t = tracer_view<O>(c);
  if (int rc = O::start_points(c, t)) return rc;
  HIP_TRY(c, hipMemsetAsync(t.d, 0, 4 * O::kDerivs * (size_t)m * sizeof(double), c->stream));
  h.valid = true;
  h.derivs = false;
  return NBODY_OK;
}

// one P(EC) step from a valid cache, queued: the predictor and the corrector are the two goes of ONE pass under NBODY_KERNEL_UPDATE.
// With fp64 tracers (their cache valid: tracers_enter) the tracers' predictor and corrector ride in the same two goes, and their
// evaluation at the bodies' predicted state is one more pass under NBODY_KERNEL_FORCES.
template <class O>
int one_step(nbody_ctx *c, double dt) {
  const bool tracers = c->tr64_n > 0;
  const CacheView b = body_view<O>(c), t = tracers ? tracer_view<O>(c) : CacheView{};
  const typename O::Launch L = O::step_launch(b, dt), T = tracers ? O::step_launch(t, dt) : typename O::Launch{};
  int rc;
  if ((rc = timed_launch(c, NBODY_KERNEL_UPDATE, [&]() -> int {
        HIP_TRY(c, O::predict(L, c->stream));
        if (tracers) HIP_TRY(c, O::predict(T, c->stream));
        return NBODY_OK;
      }, false))) return rc;
  if ((rc = O::evaluate(c, b))) return rc;
  if (tracers && (rc = O::evaluate_points(c, b, t))) return rc;
  if ((rc = timed_launch(c, NBODY_KERNEL_UPDATE, [&]() -> int {
        HIP_TRY(c, O::correct(L, c->stream));
        if (tracers) HIP_TRY(c, O::correct(T, c->stream));
        return NBODY_OK;
      }))) return rc;
  b.h->cur ^= 1;                                                   // the stored state's row := the predicted state's
  b.h->derivs = true;
  if (tracers) { t.h->cur ^= 1; t.h->derivs = true; }
  if constexpr (O::kForgetsOtherEveryStep) hermite_invalidate_order(c, O::index ^ 1);   // the other order's cache is not this state's
  c->sym_posg_valid = false;
  c->steps_done += 1;
  return NBODY_OK;
}

// ready, and at a frame end: the caches a stepping call starts from.  The state is about to move on without the other order's cache.
template <class O>
int enter_to_step(nbody_ctx *c, const char *who) {
  int rc;
  if ((rc = block_leave_both(c, who))) return rc;
  if ((rc = enter<O>(c))) return rc;
  if ((rc = tracers_enter<O>(c))) return rc;
  if constexpr (!O::kForgetsOtherEveryStep) hermite_invalidate_order(c, O::index ^ 1);
  return NBODY_OK;
}

template <class O>
int step(nbody_ctx *c, const char *who, double dt, int32_t nsteps) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if (!std::isfinite(dt) || nsteps < 0) return fail(c, NBODY_ERR_INVALID, "%s: dt is not finite, or nsteps < 0", who);
  if (!(dt > 0.0) || nsteps == 0) return NBODY_OK;
  if ((rc = enter_to_step<O>(c, who))) return rc;
  for (int s = 0; s < nsteps; ++s)
    if ((rc = one_step<O>(c, dt))) return rc;
  return NBODY_OK;
}

// the time scale of a cache's derivatives — the bodies' or the tracers' —, waited for: *t from the largest criterion value, *at where,
// *kind which criterion
template <class O>
int scale(nbody_ctx *c, const CacheView &v, double *t, int32_t *at, int32_t *kind) {
  const bool derivs = v.h->derivs;
  HIP_TRY(c, O::launch_time(v, derivs, (double *)c->scratch, c->stream));
  double k = 0.0, where = 0.0;
  if (int rc = read_energy(c, &k, &where)) return rc;              // (the scratch's two doubles: the largest k, its body)
  *t = k == 0.0 ? HUGE_VAL : (std::isfinite(k) ? O::time_of(k, derivs) : 0.0);
  *at = (int32_t)where;
  *kind = derivs ? 1 : 0;
  return NBODY_OK;
}
template <class O>
int scale_out(nbody_ctx *c, const CacheView &v, double *t_min, int32_t *at_out, int32_t *kind) {
  double t = 0.0;
  int32_t at = 0, which = 0;
  if (int rc = scale<O>(c, v, &t, &at, &which)) return rc;
  if (t_min) *t_min = t;
  if (at_out) *at_out = at;
  if (kind) *kind = which;
  return NBODY_OK;
}

// (it forgets nothing: the state does not move)
template <class O>
int timescale(nbody_ctx *c, const char *who, double *t_min, int32_t *body, int32_t *kind) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if (!t_min && !body && !kind) return fail(c, NBODY_ERR_INVALID, "%s: all three outputs are null", who);
  if ((rc = block_leave_both(c, who))) return rc;
  if ((rc = enter<O>(c))) return rc;
  return scale_out<O>(c, body_view<O>(c), t_min, body, kind);
}

template <class O>
int advance(nbody_ctx *c, const char *who, double t_span, double eta, double eta_start, double dt_max, int64_t max_steps, double *t_done,
            int64_t *steps) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if (!(eta > 0.0) || !(eta_start > 0.0) || !(dt_max > 0.0) || !(t_span >= 0.0) || !std::isfinite(t_span) || max_steps < 0)
    return fail(c, NBODY_ERR_INVALID, "%s: eta, eta_start and dt_max must be > 0, t_span >= 0 and finite, max_steps >= 0", who);
  double t_acc = 0.0;
  int64_t taken = 0;
  if (t_done) *t_done = 0.0;
  if (steps) *steps = 0;
  if (!(t_acc < t_span) || max_steps == 0) return NBODY_OK;
  if ((rc = enter_to_step<O>(c, who))) return rc;
  const double factor = O::dt_factor(eta);
  while (t_acc < t_span && taken < max_steps) {
    double t = 0.0;
    int32_t at = 0, which = 0;
    if ((rc = scale<O>(c, body_view<O>(c), &t, &at, &which))) return rc;
    double dt = std::min(dt_max, which == 1 ? factor * t : eta_start * t);
    const double rest = t_span - t_acc;
    const bool last = dt >= rest;
    if (last) dt = rest;
    if (!(dt > 0.0) || !std::isfinite(dt))
      return fail(c, NBODY_ERR_STATE, "%s: the time scale of body %d gives dt = %g after %lld steps (t = %.17g); the "
                  "state is that of the last good step", who, (int)at, dt, (long long)taken, t_acc);
    if ((rc = one_step<O>(c, dt))) return rc;
    t_acc = last ? t_span : t_acc + dt;
    taken += 1;
    if (t_done) *t_done = t_acc;
    if (steps) *steps = taken;
  }
  return NBODY_OK;
}

// a valid cache's records — the stored state's row, behind it the higher derivatives, three doubles each (have_d == false: zeros for
// those) — to the caller's array, records `stride` bytes apart: 12 doubles in fourth order, 18 in sixth
template <class O>
int get_records(nbody_ctx *c, const CacheView &v, bool have_d, double *out, size_t stride) {
  constexpr size_t kRec = O::kRow + 3 * O::kDerivs;
  const size_t n = (size_t)v.count;
  if (int rc = ensure_stage(c, n * (O::kRow * 8 + O::kDerivs * 32))) return rc;   // n * 112, n * 168
  double *h_row = (double *)c->h_stage, *h_d = h_row + O::kRow * n;   // (the higher derivatives lie side by side: a double4 per body each)
  HIP_TRY(c, hipMemcpyAsync(h_row, v.row[0], n * O::kRow * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_d, v.d, n * O::kDerivs * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; ++i) {
    double rec[kRec] = {};
    memcpy(rec, h_row + O::kRow * i, O::kRow * 8);
    if (have_d)
      for (size_t k = 0; k < (size_t)O::kDerivs; ++k) memcpy(rec + O::kRow + 3 * k, h_d + 4 * (k * n + i), 24);
    memcpy((char *)out + i * stride, rec, kRec * 8);
  }
  return NBODY_OK;
}

template <class O>
int get(nbody_ctx *c, const char *who, double *out, size_t stride) {
  constexpr int kBytes = (O::kRow + 3 * O::kDerivs) * 8;
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if (!out || stride < (size_t)kBytes) return fail(c, NBODY_ERR_INVALID, "%s: null buffer or stride < %d", who, kBytes);
  const HermiteCache &h = c->hm[O::index];
  if (!h.buf || !h.valid)
    return fail(c, NBODY_ERR_STATE, "%s: no derivatives cached for the stored state (%s_step or %s_timescale first)", who, O::kPrefix, O::kPrefix);
  // (what a start did not zero is a step's only once `derivs` is set; a session keeps zeros where a body has none)
  return get_records<O>(c, body_view<O>(c), O::kStartZeroes || h.derivs || c->hb[O::index].active, out, stride);
}

// ---- Hermite block time steps: a session of per-body power-of-two steps on the order's cache ----
struct BlockBufs { long long *T, *seg_min, *record; unsigned long long *floor_hits; int *level, *list, *seg_cnt; };
BlockBufs block_bufs(void *base, size_t n) {
  int slots;
  (void)nbody::hermite_block_segment((int)n, &slots);
  long long *q = (long long *)base;
  int *w = (int *)(q + n + slots + 3);
  return BlockBufs{q, q + n, q + n + slots, (unsigned long long *)(q + n + slots + 2), w, w + n, w + 2 * n};
}
size_t block_bytes(int n) {
  int slots;
  (void)nbody::hermite_block_segment(n, &slots);
  return ((size_t)n + slots + 3) * 8 + (2 * (size_t)n + slots) * 4;
}

// A session that carries tracers keeps a second set of the scheduler's arrays for them (HermiteBlockSession::tbuf): the joint record in
// front — the bodies' (T_next, m), then the tracers' —, the tracers' BlockBufs behind it.
constexpr size_t kJointRecordBytes = 32;
long long *joint_record(const HermiteBlockSession &s) { return (long long *)s.tbuf; }
BlockBufs tracer_bufs(const HermiteBlockSession &s) { return block_bufs((char *)s.tbuf + kJointRecordBytes, (size_t)s.carried); }

template <class O>
typename O::BlockLaunch block_launch_on(nbody_ctx *c, const CacheView &v, const BlockBufs &q, long long *record) {
  const HermiteBlockSession &s = c->hb[O::index];
  typename O::BlockLaunch L = O::block_launch(v, s.eta);
  L.part = c->probe_part; L.T = q.T; L.level = q.level; L.list = q.list; L.seg_min = q.seg_min; L.seg_cnt = q.seg_cnt; L.record = record;
  L.floor_hits = q.floor_hits; L.n = v.count; L.n_field = c->p.n_total; L.levels = s.levels; L.tick = s.tick; L.dt_max = s.dt_max;
  L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
  return L;
}
template <class O>
typename O::BlockLaunch block_launch(nbody_ctx *c) {
  const HermiteBlockSession &s = c->hb[O::index];
  const BlockBufs q = block_bufs(s.buf, (size_t)c->p.n_total);
  return block_launch_on<O>(c, body_view<O>(c), q, s.carried > 0 ? joint_record(s) : q.record);
}
// the same kernels on the tracers' arrays: their own T, levels, list and floor hits; the partial rows' chunks stay the bodies'
template <class O>
typename O::BlockLaunch tracer_block_launch(nbody_ctx *c) {
  const HermiteBlockSession &s = c->hb[O::index];
  return block_launch_on<O>(c, tracer_view<O>(c), tracer_bufs(s), joint_record(s) + 2);
}

// the totals since begin; the levels' range and the floor hits are read from the device (4 n + 8 bytes): waits for the stream
int block_read_levels(nbody_ctx *c, const BlockBufs &q, size_t n, int64_t *floor_hits, int32_t *level_min, int32_t *level_max) {
  if (int rc = ensure_stage(c, n * 4 + 8)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, q.floor_hits, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync((char *)c->h_stage + 8, q.level, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(floor_hits, c->h_stage, 8);
  const int32_t *lv = (const int32_t *)((const char *)c->h_stage + 8);
  *level_min = *std::min_element(lv, lv + n); *level_max = *std::max_element(lv, lv + n);
  return NBODY_OK;
}
int block_fill(nbody_ctx *c, const HermiteBlockSession &s, nbody_hermite_block_stats *out) {
  out->synchronised = (s.ticks & ((1ll << s.levels) - 1)) == 0 ? 1 : 0;
  out->ticks = s.ticks; out->frames_done = s.ticks >> s.levels; out->block_steps = s.block_steps;
  out->body_steps = s.body_steps; out->pairs = s.pairs;
  const size_t n = (size_t)c->p.n_total;
  return block_read_levels(c, block_bufs(s.buf, n), n, &out->floor_hits, &out->level_min, &out->level_max);
}
// the tracers' totals since begin (the bodies' stay in nbody_hermite_block_stats, untouched by the tracers)
int block_fill_tracers(nbody_ctx *c, const HermiteBlockSession &s, nbody_hermite_block_tracer_stats *out) {
  out->carried = s.carried; out->tracer_steps = s.tracer_steps; out->pairs = s.tracer_pairs; out->tracer_only_steps = s.tracer_only_steps;
  out->floor_hits = 0; out->level_min = out->level_max = 0;
  if (s.carried == 0) return NBODY_OK;
  return block_read_levels(c, tracer_bufs(s), (size_t)s.carried, &out->floor_hits, &out->level_min, &out->level_max);
}

// one block step, from the schedule to the stored bodies; the host waits once, for (T_next, m), to size the evaluation.  An active set
// larger than a slab of partial rows goes through evaluation and corrector slab by slab: the predicted state is in buffers of its own, so
// a corrected slab changes nothing a later slab's evaluation reads.
// A session that carries tracers schedules both sets jointly — T_next over bodies AND tracers, a list each, everything predicted — and
// reads (T_next, m_b, T_next, m_t).  The due bodies are evaluated and corrected as ever; then the due tracers, at the bodies' PREDICTED
// state (the corrector wrote the stored one), through the same staging area on the same stream.  Either set may be empty, not both.
template <class O>
int block_one_step(nbody_ctx *c, const char *who) {
  HermiteBlockSession &s = c->hb[O::index];
  const bool carrying = s.carried > 0;
  const typename O::BlockLaunch L = block_launch<O>(c), P = carrying ? tracer_block_launch<O>(c) : typename O::BlockLaunch{};
  const int n = c->p.n_total;
  const size_t slab = nbody::probe_slab_points(n, O::kPartWidth);
  int rc;
  if ((rc = O::block_parts_hold(c))) return rc;                    // (the partial rows of reserve_parts(n), and of reserve_parts(carried))
  if (carrying && (rc = points64_part_holds(c, (int)std::min(slab, (size_t)s.carried), O::kPartWidth, "the tracers' pass of a block step"))) return rc;
  if ((rc = timed_launch(c, NBODY_KERNEL_UPDATE, [&]() -> int {
        HIP_TRY(c, carrying ? O::block_schedule_joint(L, P, c->stream) : O::block_schedule(L, c->stream));
        return NBODY_OK;
      }, false))) return rc;
  const size_t rec_bytes = carrying ? kJointRecordBytes : 16;
  HIP_TRY(c, hipMemcpyAsync(c->h_scratch, L.record, rec_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  long long rec[4] = {0, 0, 0, 0};
  memcpy(rec, c->h_scratch, rec_bytes);
  const long long t_next = rec[0];
  if (rec[1] < 0 || rec[1] > n || rec[3] < 0 || rec[3] > s.carried || rec[1] + rec[3] < 1 || t_next <= s.ticks || (carrying && rec[2] != t_next))
    return fail(c, NBODY_ERR_STATE, "%s: the schedule gave T_next = %lld, m = %lld (tracers: T_next = %lld, m = %lld) at tick %lld", who,
                t_next, rec[1], rec[2], rec[3], (long long)s.ticks);
  const int m_b = (int)rec[1], m_t = (int)rec[3];
  // the due rows of one set — the bodies (X = L) or the tracers (X = P) —: evaluation and corrector, slab by slab
  const auto pass = [&](const typename O::BlockLaunch &X, int m, bool points, bool last_set) -> int {
    const int lanes = nbody::hermite_block_lanes(m, s.lanes);
    const int rows = (int)std::min(slab, (size_t)X.n);
    for (int first = 0; first < m; first += rows) {
      const int ms = std::min(rows, m - first);
      const bool last = first + ms == m;
      if (int e = timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
            HIP_TRY(c, points ? O::block_evaluate_points(c, L, X, first, ms, lanes) : O::block_evaluate(X, first, ms, lanes, c->stream));
            return NBODY_OK;
          }, last)) return e;
      if (int e = timed_launch(c, NBODY_KERNEL_UPDATE, [&]() -> int { HIP_TRY(c, O::block_correct(X, first, ms, t_next, c->stream)); return NBODY_OK; },
                               last && last_set)) return e;
    }
    return NBODY_OK;
  };
  if (m_b > 0 && (rc = pass(L, m_b, false, m_t == 0))) return rc;
  if (m_t > 0 && (rc = pass(P, m_t, true, true))) return rc;
  s.ticks = t_next;
  s.block_steps += 1; s.body_steps += m_b; s.pairs += (int64_t)m_b * n;
  s.tracer_steps += m_t; s.tracer_pairs += (int64_t)m_t * n; s.tracer_only_steps += m_b == 0 ? 1 : 0;
  if (s.ticks >= (1ll << s.levels)) {                              // a whole frame: every body has stepped, every higher derivative is a step's
    c->hm[O::index].derivs = true;
    if (carrying) c->trh[O::index].derivs = true;
  }
  c->sym_posg_valid = false;
  c->steps_done += 1;
  return NBODY_OK;
}

// carry == false: the plain begin, which refuses a context with fp64 tracers.  carry == true (the order's block_begin_tracers): the same
// begin, and on a context with tracers a session that carries them — their cache filled where it is invalid, T := 0, their levels from
// tracer_level_in or from the start rule on their own (a0, j0), by the bodies' init kernel on the tracers' arrays.
template <class O>
int block_begin(nbody_ctx *c, const char *who, double dt_max, int32_t levels, double eta, double eta_start, const int32_t *level_in,
                bool carry, const int32_t *tracer_level_in) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  const auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
  if (!positive(dt_max) || !positive(eta) || !positive(eta_start) || levels < 0 || levels > nbody::kHermiteBlockMaxLevels)
    return fail(c, NBODY_ERR_INVALID, "%s: dt_max, eta and eta_start must be finite and > 0, levels 0 .. %d", who, nbody::kHermiteBlockMaxLevels);
  const double tick = std::ldexp(dt_max, -levels);
  if (const char *why = O::tick_refused(tick)) return fail(c, NBODY_ERR_INVALID, "%s: the tick dt_max 2^-levels = %g %s", who, tick, why);
  if (!carry && c->tr64_n > 0) {
    if ((rc = block_leave_both(c, who, false))) return rc;         // (a carrying session in mid-frame: that first; the check ends nothing)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: the context holds %d fp64 tracers, which the block scheduler does not "
                "carry (they have no levels of their own); nbody_set_tracers_f64(ctx, NULL, 0, NULL, 0, 0) removes them "
                "(%s_block_begin_tracers starts a session that carries them)", who, c->tr64_n, O::kPrefix);
  }
  const int n = c->p.n_total, m = carry ? c->tr64_n : 0;
  if (level_in)
    for (int i = 0; i < n; ++i)
      if (level_in[i] < 0 || level_in[i] > levels)
        return fail(c, NBODY_ERR_INVALID, "%s: level_in[%d] = %d is outside 0 .. %d", who, i, (int)level_in[i], (int)levels);
  if (tracer_level_in && m == 0) return fail(c, NBODY_ERR_INVALID, "%s: tracer_level_in is not NULL, and the context holds no fp64 tracers", who);
  if (tracer_level_in)
    for (int i = 0; i < m; ++i)
      if (tracer_level_in[i] < 0 || tracer_level_in[i] > levels)
        return fail(c, NBODY_ERR_INVALID, "%s: tracer_level_in[%d] = %d is outside 0 .. %d", who, i, (int)tracer_level_in[i], (int)levels);
  if ((rc = block_leave_both(c, who))) return rc;
  if ((rc = enter<O>(c))) return rc;
  if (m > 0 && (rc = tracers_enter<O>(c))) return rc;
  hermite_invalidate_order(c, O::index ^ 1);                       // (the state moves on without the other order's cache)
  HermiteBlockSession &s = c->hb[O::index];
  if (!s.buf) HIP_TRY(c, hipMalloc(&s.buf, block_bytes(n)));
  if (m > 0 && s.tbuf_n != m) {
    if (s.tbuf) { HIP_TRY(c, hipStreamSynchronize(c->stream)); (void)hipFree(s.tbuf); s.tbuf = nullptr; s.tbuf_n = 0; }
    HIP_TRY(c, hipMalloc(&s.tbuf, kJointRecordBytes + block_bytes(m)));
    s.tbuf_n = m;
  }
  s.levels = levels; s.dt_max = dt_max; s.tick = tick; s.eta = eta;
  s.lanes = nbody::env_int(O::kLanesEnv, 0);
  s.ticks = s.block_steps = s.body_steps = s.pairs = 0;
  s.carried = m; s.tracer_steps = s.tracer_pairs = s.tracer_only_steps = 0;
  const typename O::BlockLaunch L = block_launch<O>(c);
  // the higher derivatives lie side by side, 64 / 96 bytes per body: zeros until a body steps
  if (!c->hm[O::index].derivs) HIP_TRY(c, hipMemsetAsync(body_view<O>(c).d, 0, (size_t)n * O::kDerivs * 32, c->stream));
  HIP_TRY(c, hipMemsetAsync(block_bufs(s.buf, (size_t)n).record, 0, 24, c->stream));   // the record and the floor hits
  if (level_in) HIP_TRY(c, hipMemcpyAsync(L.list, level_in, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, O::block_init(L, level_in ? L.list : nullptr, eta_start, c->stream));
  if (m > 0) {
    const typename O::BlockLaunch P = tracer_block_launch<O>(c);
    if (!c->trh[O::index].derivs) HIP_TRY(c, hipMemsetAsync(tracer_view<O>(c).d, 0, (size_t)m * O::kDerivs * 32, c->stream));
    HIP_TRY(c, hipMemsetAsync(joint_record(s), 0, kJointRecordBytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(tracer_bufs(s).record, 0, 24, c->stream));
    if (tracer_level_in) HIP_TRY(c, hipMemcpyAsync(P.list, tracer_level_in, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, O::block_init(P, tracer_level_in ? P.list : nullptr, eta_start, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));                     // the caller's arrays are its own again
  s.active = true;
  return NBODY_OK;
}

template <class O>
int block_advance(nbody_ctx *c, const char *who, int64_t frames, int64_t max_block_steps, nbody_hermite_block_stats *out) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if (frames < 0 || max_block_steps < 0 || (out && out->struct_size != sizeof(nbody_hermite_block_stats)))
    return fail(c, NBODY_ERR_INVALID, "%s: frames < 0, max_block_steps < 0, or out->struct_size is not "
                "sizeof(nbody_hermite_block_stats) = %d", who, (int)sizeof(nbody_hermite_block_stats));
  const HermiteBlockSession &s = c->hb[O::index];
  if (!s.active)
    return fail(c, NBODY_ERR_STATE, "%s: no %sblock session (%s_block_begin first; uploads, kick-drift steps, handed-out pointers, "
                "shared Hermite steps and nbody_hermite_restart end one)", who, O::kOrdinal, O::kPrefix);
  const int64_t frame_now = s.ticks >> s.levels;
  if (frames >= (1ll << 62 >> s.levels) - frame_now)
    return fail(c, NBODY_ERR_INVALID, "%s: %lld more frames of 2^%d ticks pass 2^62 ticks", who, (long long)frames, s.levels);
  const int64_t target = frames == 0 ? s.ticks : (frame_now + frames) << s.levels;
  for (int64_t taken = 0; s.ticks < target && taken < max_block_steps; ++taken)
    if ((rc = block_one_step<O>(c, who))) return rc;
  return out ? block_fill(c, s, out) : NBODY_OK;
}

template <class O>
int block_get(nbody_ctx *c, const char *who, int64_t *ticks, int32_t *level) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if (!c->hb[O::index].active) return fail(c, NBODY_ERR_STATE, "%s: no %sblock session (%s_block_begin first)", who, O::kOrdinal, O::kPrefix);
  const size_t n = (size_t)c->p.n_total;
  const BlockBufs q = block_bufs(c->hb[O::index].buf, n);
  if ((rc = ensure_stage(c, n * 12))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, q.T, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync((char *)c->h_stage + n * 8, q.level, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (ticks) memcpy(ticks, c->h_stage, n * 8);
  if (level) memcpy(level, (const char *)c->h_stage + n * 8, n * 4);
  return NBODY_OK;
}

// T_i and k_i of the tracers a session carries, and their totals since begin
template <class O>
int block_tracers_get(nbody_ctx *c, const char *who, int64_t *ticks, int32_t *level, nbody_hermite_block_tracer_stats *stats) {
  int rc = hermite_ready(c, who);
  if (rc) return rc;
  if ((!ticks && !level && !stats) || (stats && stats->struct_size != sizeof(nbody_hermite_block_tracer_stats)))
    return fail(c, NBODY_ERR_INVALID, "%s: all three outputs are null, or stats->struct_size is not "
                "sizeof(nbody_hermite_block_tracer_stats) = %d", who, (int)sizeof(nbody_hermite_block_tracer_stats));
  const HermiteBlockSession &s = c->hb[O::index];
  if (!s.active) return fail(c, NBODY_ERR_STATE, "%s: no %sblock session (%s_block_begin_tracers first)", who, O::kOrdinal, O::kPrefix);
  const size_t m = (size_t)s.carried;
  if (m > 0 && (ticks || level)) {
    const BlockBufs q = tracer_bufs(s);
    if ((rc = ensure_stage(c, m * 12))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_stage, q.T, m * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync((char *)c->h_stage + m * 8, q.level, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ticks) memcpy(ticks, c->h_stage, m * 8);
    if (level) memcpy(level, (const char *)c->h_stage + m * 8, m * 4);
  }
  if (stats) return block_fill_tracers(c, s, stats);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

// ---- the snap, the fp64 point queries and the fp64 tracers' public calls ----
// where the snap exists: fp64 state, one device, all bodies
int snap_supported(nbody_ctx *c, const char *who) {
  if (c->p.precision != NBODY_PREC_F64)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context whose state is fp32 (NBODY_PREC_F32, NBODY_PREC_F32_KAHAN): the snap's pair term "
                "takes differences of accelerations, which need fp64 state; create the context with NBODY_PREC_F64", who);
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  return NBODY_OK;
}

template <class O>
int tracers_get(nbody_ctx *c, const char *who, double *out, size_t stride) {
  constexpr int kBytes = (O::kRow + 3 * O::kDerivs) * 8;
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!out || stride < (size_t)kBytes) return fail(c, NBODY_ERR_INVALID, "%s: null buffer or stride < %d", who, kBytes);
  if (c->tr64_n == 0) return NBODY_OK;
  const HermiteCache &h = c->trh[O::index];
  if (!h.buf || !h.valid)
    return fail(c, NBODY_ERR_STATE, "%s: no derivatives cached for the stored tracers (%s_step or %s_tracers_timescale first)", who, O::kPrefix, O::kPrefix);
  return get_records<O>(c, tracer_view<O>(c), true, out, stride);   // (zeros until a step has been taken)
}

template <class O>
int tracers_timescale(nbody_ctx *c, const char *who, double *t_min, int32_t *tracer, int32_t *kind) {
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (!t_min && !tracer && !kind) return fail(c, NBODY_ERR_INVALID, "%s: all three outputs are null", who);
  if (c->tr64_n <= 0) return fail(c, NBODY_ERR_STATE, "%s: the context holds no fp64 tracers (nbody_set_tracers_f64 first)", who);
  if ((rc = block_leave_both(c, who))) return rc;                  // (a session that carries them: the rule of the bodies' timescale)
  if constexpr (O::kTracerStartReadsCache) { if ((rc = enter<O>(c))) return rc; }
  else if (c->hm_external) hermite_invalidate(c);                  // (the rule enter applies, where the bodies' cache is not needed)
  if ((rc = tracers_enter<O>(c))) return rc;
  return scale_out<O>(c, tracer_view<O>(c), t_min, tracer, kind);
}

}  // namespace

extern "C" {

int nbody_hermite_step(nbody_ctx *c, double dt, int32_t nsteps) { return step<Order4>(c, "nbody_hermite_step", dt, nsteps); }
int nbody_hermite6_step(nbody_ctx *c, double dt, int32_t nsteps) { return step<Order6>(c, "nbody_hermite6_step", dt, nsteps); }

int nbody_hermite_timescale(nbody_ctx *c, double *t_min, int32_t *body, int32_t *kind) {
  return timescale<Order4>(c, "nbody_hermite_timescale", t_min, body, kind);
}
int nbody_hermite6_timescale(nbody_ctx *c, double *t_min, int32_t *body, int32_t *kind) {
  return timescale<Order6>(c, "nbody_hermite6_timescale", t_min, body, kind);
}

int nbody_hermite_advance(nbody_ctx *c, double t_span, double eta, double eta_start, double dt_max, int64_t max_steps, double *t_done,
                          int64_t *steps) {
  return advance<Order4>(c, "nbody_hermite_advance", t_span, eta, eta_start, dt_max, max_steps, t_done, steps);
}
int nbody_hermite6_advance(nbody_ctx *c, double t_span, double eta, double eta_start, double dt_max, int64_t max_steps, double *t_done,
                           int64_t *steps) {
  return advance<Order6>(c, "nbody_hermite6_advance", t_span, eta, eta_start, dt_max, max_steps, t_done, steps);
}

int nbody_hermite_get(nbody_ctx *c, double *d12, size_t stride) { return get<Order4>(c, "nbody_hermite_get", d12, stride); }
int nbody_hermite6_get(nbody_ctx *c, double *d18, size_t stride) { return get<Order6>(c, "nbody_hermite6_get", d18, stride); }

int nbody_hermite_restart(nbody_ctx *c) {
  int rc = hermite_ready(c, "nbody_hermite_restart");
  if (rc) return rc;
  hermite_invalidate(c);
  return NBODY_OK;
}

int nbody_hermite_block_level(double dt_c, double dt_max, int32_t levels, int32_t *floor_hit) {
  if (levels < 0 || levels > nbody::kHermiteBlockMaxLevels) return -1;
  int hit = 0;
  const int k = nbody::hermite_block_level(dt_c, dt_max, levels, &hit);
  if (floor_hit) *floor_hit = hit;
  return k;
}
int nbody_hermite6_block_level(double k, double dt_max, int32_t levels, double eta, int32_t *floor_hit) {
  if (levels < 0 || levels > nbody::kHermiteBlockMaxLevels) return -1;
  int hit = 0;
  const int kw = nbody::hermite6_block_level(k, dt_max, levels, eta, &hit);
  if (floor_hit) *floor_hit = hit;
  return kw;
}

int nbody_hermite_block_begin(nbody_ctx *c, double dt_max, int32_t levels, double eta, double eta_start, const int32_t *level_in) {
  return block_begin<Order4>(c, "nbody_hermite_block_begin", dt_max, levels, eta, eta_start, level_in, false, nullptr);
}
int nbody_hermite6_block_begin(nbody_ctx *c, double dt_max, int32_t levels, double eta, double eta_start, const int32_t *level_in) {
  return block_begin<Order6>(c, "nbody_hermite6_block_begin", dt_max, levels, eta, eta_start, level_in, false, nullptr);
}
int nbody_hermite_block_begin_tracers(nbody_ctx *c, double dt_max, int32_t levels, double eta, double eta_start, const int32_t *level_in,
                                      const int32_t *tracer_level_in) {
  return block_begin<Order4>(c, "nbody_hermite_block_begin_tracers", dt_max, levels, eta, eta_start, level_in, true, tracer_level_in);
}
int nbody_hermite6_block_begin_tracers(nbody_ctx *c, double dt_max, int32_t levels, double eta, double eta_start, const int32_t *level_in,
                                       const int32_t *tracer_level_in) {
  return block_begin<Order6>(c, "nbody_hermite6_block_begin_tracers", dt_max, levels, eta, eta_start, level_in, true, tracer_level_in);
}
int nbody_hermite_block_tracers_get(nbody_ctx *c, int64_t *ticks, int32_t *level, nbody_hermite_block_tracer_stats *stats) {
  return block_tracers_get<Order4>(c, "nbody_hermite_block_tracers_get", ticks, level, stats);
}
int nbody_hermite6_block_tracers_get(nbody_ctx *c, int64_t *ticks, int32_t *level, nbody_hermite_block_tracer_stats *stats) {
  return block_tracers_get<Order6>(c, "nbody_hermite6_block_tracers_get", ticks, level, stats);
}

int nbody_hermite_block_advance(nbody_ctx *c, int64_t frames, int64_t max_block_steps, nbody_hermite_block_stats *out) {
  return block_advance<Order4>(c, "nbody_hermite_block_advance", frames, max_block_steps, out);
}
int nbody_hermite6_block_advance(nbody_ctx *c, int64_t frames, int64_t max_block_steps, nbody_hermite_block_stats *out) {
  return block_advance<Order6>(c, "nbody_hermite6_block_advance", frames, max_block_steps, out);
}

int nbody_hermite_block_get(nbody_ctx *c, int64_t *ticks, int32_t *level) { return block_get<Order4>(c, "nbody_hermite_block_get", ticks, level); }
int nbody_hermite6_block_get(nbody_ctx *c, int64_t *ticks, int32_t *level) { return block_get<Order6>(c, "nbody_hermite6_block_get", ticks, level); }

int nbody_hermite_tracers_get(nbody_ctx *c, double *d12, size_t stride) { return tracers_get<Order4>(c, "nbody_hermite_tracers_get", d12, stride); }
int nbody_hermite6_tracers_get(nbody_ctx *c, double *d18, size_t stride) { return tracers_get<Order6>(c, "nbody_hermite6_tracers_get", d18, stride); }

int nbody_hermite_tracers_timescale(nbody_ctx *c, double *t_min, int32_t *tracer, int32_t *kind) {
  return tracers_timescale<Order4>(c, "nbody_hermite_tracers_timescale", t_min, tracer, kind);
}
int nbody_hermite6_tracers_timescale(nbody_ctx *c, double *t_min, int32_t *tracer, int32_t *kind) {
  return tracers_timescale<Order6>(c, "nbody_hermite6_tracers_timescale", t_min, tracer, kind);
}

int nbody_get_snap_f64(nbody_ctx *c, const double *acc_in, size_t acc_in_stride, double *acc, size_t acc_stride, double *jerk,
                       size_t jerk_stride, double *snap, size_t snap_stride) {
  const char *who = "nbody_get_snap_f64";
  if (c && c->multi) return multi_unsupported(c, who);
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = snap_supported(c, who))) return rc;
  if ((!acc && !jerk && !snap) || (acc_in && acc_in_stride < 24) || (acc && acc_stride < 24) || (jerk && jerk_stride < 24) || (snap && snap_stride < 24))
    return fail(c, NBODY_ERR_INVALID, "%s: all three outputs are null, or a stride < 24", who);
  const size_t n = (size_t)c->p.n_total, rec = 9 * sizeof(double);
  if ((rc = ensure_stage(c, n * rec))) return rc;
  if (!c->snap64) HIP_TRY(c, hipMalloc(&c->snap64, 13 * n * sizeof(double)));
  if ((rc = ensure_probe_part(c, (int)n, kSnapRowWidth))) return rc;
  double *ajs = (double *)c->snap64, *ain = ajs + 9 * n;
  int ain_stride = 4;
  if (acc_in) {
    double *h = (double *)c->h_stage;
    for (size_t i = 0; i < n; ++i) { memcpy(h + 4 * i, (const char *)acc_in + i * acc_in_stride, 24); h[4 * i + 3] = 0.0; }
    HIP_TRY(c, hipMemcpyAsync(ain, h, n * 32, hipMemcpyHostToDevice, c->stream));
  } else {                                                         // the live state's own accelerations, unrounded: the fp64 jerk pass first
    if ((rc = ensure_rows64(c, &c->jerk64, 6))) return rc;
    if ((rc = queue_body_jerk(c, (double *)c->jerk64, nullptr))) return rc;
    ain = (double *)c->jerk64; ain_stride = 6;
  }
  if ((rc = snap_evaluate(c, c->posm, c->vel, ain, ain_stride, ajs))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, ajs, n * rec, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (acc) scatter_records(acc, acc_stride, c->h_stage, 24, n, rec);
  if (jerk) scatter_records(jerk, jerk_stride, (const char *)c->h_stage + 24, 24, n, rec);
  if (snap) scatter_records(snap, snap_stride, (const char *)c->h_stage + 48, 24, n, rec);
  return NBODY_OK;
}

int nbody_jerk_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n, double *acc,
                      size_t acc_stride, double *jerk, size_t jerk_stride) {
  const char *who = "nbody_jerk_at_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (n < 0 || !pos || pos_stride < 24 || (vel && vel_stride < 24) || (!acc && !jerk) || (acc && acc_stride < 24) || (jerk && jerk_stride < 24))
    return fail(c, NBODY_ERR_INVALID, "%s: null points, n < 0, both outputs null, or a stride < 24", who);
  if (n == 0) return NBODY_OK;
  const size_t m = (size_t)n;
  if ((rc = ensure_probe_part(c, n, 3))) return rc;
  Staged64 s;                                                      // the points and their velocities, behind them six doubles per point
  if ((rc = stage_points64(c, pos, pos_stride, vel, vel_stride, true, m, m * 48, &s))) return rc;
  double *d = s.d, *h = s.h + s.skip;
  if ((rc = points64_jerk(c, c->posm, c->vel, d, d + 4 * m, n, d + 8 * m))) return rc;
  if ((rc = stage_to_host(c, s.skip * 8, m * 48))) return rc;
  if (acc) scatter_records(acc, acc_stride, h, 24, m, 48);
  if (jerk) scatter_records(jerk, jerk_stride, h + 3, 24, m, 48);
  return NBODY_OK;
}

int nbody_snap_at_f64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n, double *acc,
                      size_t acc_stride, double *jerk, size_t jerk_stride, double *snap, size_t snap_stride) {
  const char *who = "nbody_snap_at_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (n < 0 || !pos || pos_stride < 24 || (vel && vel_stride < 24) || (!acc && !jerk && !snap) || (acc && acc_stride < 24) ||
      (jerk && jerk_stride < 24) || (snap && snap_stride < 24))
    return fail(c, NBODY_ERR_INVALID, "%s: null points, n < 0, all three outputs null, or a stride < 24", who);
  if (n == 0) return NBODY_OK;
  const size_t m = (size_t)n;
  if ((rc = ensure_probe_part(c, n, 3))) return rc;
  if ((rc = ensure_probe_part(c, n, kSnapRowWidth))) return rc;
  if ((rc = ensure_rows64(c, &c->jerk64, 6))) return rc;
  Staged64 s;                                                      // the points and their velocities, behind them six doubles (a, j), nine (a, j, s)
  if ((rc = stage_points64(c, pos, pos_stride, vel, vel_stride, true, m, m * 120, &s))) return rc;
  double *d = s.d, *h = s.h + 14 * m;
  // the bodies' unrounded accelerations of the live state (as nbody_get_snap_f64 with acc_in == NULL), the points' own, then the snap
  if ((rc = queue_body_jerk(c, (double *)c->jerk64, nullptr))) return rc;
  if ((rc = points64_jerk(c, c->posm, c->vel, d, d + 4 * m, n, d + 8 * m))) return rc;
  if ((rc = points64_snap(c, c->posm, c->vel, (const double *)c->jerk64, 6, d, d + 4 * m, d + 8 * m, 6, n, d + 14 * m))) return rc;
  if ((rc = stage_to_host(c, 14 * m * 8, m * 72))) return rc;
  if (acc) scatter_records(acc, acc_stride, h, 24, m, 72);
  if (jerk) scatter_records(jerk, jerk_stride, h + 3, 24, m, 72);
  if (snap) scatter_records(snap, snap_stride, h + 6, 24, m, 72);
  return NBODY_OK;
}

int nbody_set_tracers_f64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n) {
  const char *who = "nbody_set_tracers_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!pos || pos_stride < 24 || (vel && vel_stride < 24))))
    return fail(c, NBODY_ERR_INVALID, "%s: n < 0, null positions, or a stride < 24", who);
  for (const HermiteBlockSession &s : c->hb)                       // (n == 0 too: the session's lists index the tracers it began with)
    if (s.active && s.carried > 0)
      return fail(c, NBODY_ERR_STATE, "%s: a Hermite block session carries the %d fp64 tracers; nbody_hermite_restart ends the session", who, s.carried);
  if (n > 0 && (c->hb[0].active || c->hb[1].active))
    return fail(c, NBODY_ERR_STATE, "%s: a Hermite block session is active, and it began without tracers (nbody_hermite[6]_block_begin_tracers carries those a context holds at begin); nbody_hermite_restart "
                "ends the session", who);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->tr64) (void)hipFree(c->tr64);
  c->tr64 = nullptr;
  c->tr64_n = 0;
  for (HermiteCache &h : c->trh) {                                 // the tracers' caches, and only those
    if (h.buf) (void)hipFree(h.buf);
    h = HermiteCache{};
  }
  if (n == 0) return NBODY_OK;
  const size_t m = (size_t)n;
  if ((rc = ensure_stage(c, m * 64))) return rc;
  HIP_TRY(c, hipMalloc(&c->tr64, 24 * m * sizeof(double)));
  double *h = (double *)c->h_stage;
  gather4(h, pos, pos_stride, m);
  gather4(h + 4 * m, vel, vel_stride, m);
  HIP_TRY(c, hipMemsetAsync(c->tr64, 0, 24 * m * sizeof(double), c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->tr64, h, m * 64, hipMemcpyHostToDevice, c->stream));   // pos and vel lie side by side
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tr64_n = n;
  return NBODY_OK;
}

int nbody_get_tracers_f64(nbody_ctx *c, double *pos, size_t pos_stride, double *vel, size_t vel_stride) {
  const char *who = "nbody_get_tracers_f64";
  int rc = points64_ready(c, who);
  if (rc) return rc;
  if ((pos && pos_stride < 24) || (vel && vel_stride < 24)) return fail(c, NBODY_ERR_INVALID, "%s: a stride < 24", who);
  const size_t m = (size_t)c->tr64_n;
  if (m == 0 || (!pos && !vel)) return NBODY_OK;
  if ((rc = ensure_stage(c, m * 64))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->tr64, m * 64, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double *h = (const double *)c->h_stage;
  if (pos) scatter_records(pos, pos_stride, h, 24, m, 32);
  if (vel) scatter_records(vel, vel_stride, h + 4 * m, 24, m, 32);
  return NBODY_OK;
}

int nbody_tracer_count_f64(nbody_ctx *c, int32_t *n) {
  int rc = points64_ready(c, "nbody_tracer_count_f64");
  if (rc) return rc;
  if (!n) return fail(c, NBODY_ERR_INVALID, "nbody_tracer_count_f64: null output");
  *n = c->tr64_n;
  return NBODY_OK;
}

}  // extern "C"
