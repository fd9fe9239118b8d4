// The context behind the C-ABI's opaque nbody_ctx and what the host files that work on one (the C-ABI's units capi.hip, capi_state.hip,
// capi_step.hip, capi_query.hip, capi_query64.hip, capi_hermite.hip — capi_common.h says which holds what — and bh_driver.hip) share:
// error texts, the device made current, the kernel timers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nbody.h"
#include "kernels.h"
#include "launch_policy.h"   // (g_create_error lives there: the policy's describe call reports through it too)
#include "multi.h"
#include "sym_plan.h"

namespace nbody {

struct EventPair { hipEvent_t a, b; bool counts = true; };   // counts: the interval is a whole pass (not the first go of two)

struct KernelTimer {
  std::vector<EventPair> pending;   // recorded, not yet read
  std::vector<EventPair> pool;      // free
  double total_ms = 0.0;
  int64_t launches = 0;
};

// One cache of Hermite derivatives — the bodies' or the fp64 tracers', of one order —, allocated at first use.  With `count` the bodies
// (n_total) or the tracers (tr64_n), buf holds, in doubles:
//   the bodies' caches only: the predicted arrays, [count] double4 each
//   the higher derivatives a step leaves, [count] double4 each
//   two rows of the evaluated derivatives, [count][width] each: row `cur` is the stored state's, the other takes the predicted state's
//     (and, at a sixth-order start, the jerk pass's [count][6])
//   the time scale's reduction: its workgroup pairs
//                  predicted    higher derivatives   a row             width
//   fourth order   xp, vp       a2, a3               (a0, j0)          6
//   sixth order    xp, vp, ap   a3, a4, a5           (a0, j0, s0)      9
// (the tracers' predicted arrays lie in tr64)
struct HermiteCache {
  void *buf = nullptr;
  int cur = 0;
  bool valid = false;    // row `cur` is that of the stored (x, v) — the tracers': of the stored tracers in the stored bodies' field
  bool derivs = false;   // the higher derivatives are those a step left at the stored state (sixth order and the tracers: zeros otherwise)
};

// One session of Hermite block time steps on the bodies' cache of its order.  buf, allocated at the first begin: T [n] int64, the
// scheduler's segment minima [slots] int64, the record (T_next, m) and the floor-hit count (int64 each), then level [n], list [n] and the
// segment counts [slots] as int32
struct HermiteBlockSession {
  void *buf = nullptr;
  bool active = false;         // between the order's block_begin and whatever ends the session
  int levels = 0, lanes = 0;   // lanes: bodies per lane of the evaluation forced by NBODY_HERMITE_BLOCK_LANES / NBODY_HERMITE6_BLOCK_LANES (0: by the list's length)
  double dt_max = 0.0, tick = 0.0, eta = 0.0;
  int64_t ticks = 0, block_steps = 0, body_steps = 0, pairs = 0;   // T_sys and the totals since begin
  // A session that carries the fp64 tracers (the order's block_begin_tracers): tbuf, allocated for tbuf_n tracers, holds the joint record
  // — (T_next, m) of the bodies, then of the tracers: the 32 bytes the host reads per block step — and behind it the tracers' T, segment
  // minima, record (unused), floor-hit count, level, list and segment counts in the layout of buf.
  void *tbuf = nullptr;
  int tbuf_n = 0, carried = 0;   // carried: the tracers this session carries (0: none; the plain begins' sessions)
  int64_t tracer_steps = 0, tracer_pairs = 0, tracer_only_steps = 0;
};

}  // namespace nbody

struct nbody_ctx {
  nbody::Multi *multi = nullptr;   // nbody_create_multi: this context is a front for one context per device (multi.h)
  nbody_params p;
  size_t elem;                 // bytes per float4/double4 element
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  void *posm = nullptr, *vel = nullptr, *acc = nullptr, *accp = nullptr;
  void *posm_alt = nullptr;    // small systems: second position buffer of the one-launch step (swapped with posm)
  bool own_posm = false, own_vel = false, own_acc = false;
  // the one staging pair (ensure_stage): the frame's FParticle records, the per-body getters' rows, every point query's points and results —
  // on the device, and its pinned mirror.  Only calls that wait for their own work before they return use it.
  void *d_stage = nullptr, *h_stage = nullptr;
  size_t stage_bytes = 0;
  void *scratch = nullptr;     // 64 B device scratch (bounds bits, energy sums)
  void *h_scratch = nullptr;   // pinned mirror
  void *energy_part = nullptr; // nbody_energy: one pair of doubles per workgroup, folded in a fixed order
  void *moments_part = nullptr, *moments_host = nullptr;   // nbody_get_moments / nbody_mass_within: results + per-workgroup slots (kernels_moments.hip), pinned mirror of the results
  int j_split = 1, j_chunk = 0, ipt = 1, tile = 256;
  int sym_np = 1;                        // register pairs per lane of the symmetric kernel
  std::vector<std::pair<char *, size_t>> pinned;   // caller memory page-locked by nbody_pin_host_buffer
  int wave = 0;                // block kernel: register pairs of bodies per workgroup (0 = tile / symmetric kernels)
  int bh_word = 0;             // larger Barnes-Hut systems: which of the two Size words (scratch + 40, + 44) the next frame uses
  int tick_word = 0;           // nbody_tick on the one-launch step: which of the two Size words (scratch + 32, + 36) is cleared and next
  bool have_state = false;
  double floor_eps2 = -1.0;    // NBODY_ZERO_FLOOR: eps^2 floor for the current masses (< 0 = not yet computed)
  // symmetric algorithm (kernels_sym.hip, kernels_sym64.hip; plan: sym_plan.h)
  bool sym = false;
  int sym_bi = 0, sym_pad = 0, sym_items_n = 0, sym_nsrc = 1, sym_slots = 0, sym_min_sub = 0;
  int sym_n_local = 0;                   // items [0, sym_n_local): strips inside the own slice (sym_plan.h)
  std::vector<int> sym_phase_item0;      // pool phases of the plan: phase p = items [p], [p + 1]) (one phase unless the pool had to be shared)
  int sym_n_gran = 0;
  double sym_k = 0.0;
  bool sym_even = false;                 // the plan is an even-share plan (sym_plan.h)
  size_t sym_pool_elems = 0;
  nbody::SymPlan *plan = nullptr;                  // host copy, dropped once uploaded
  void *sym_pool = nullptr, *sym_items = nullptr, *sym_iptr = nullptr, *sym_ioff = nullptr, *sym_jptr = nullptr,
       *sym_joff = nullptr, *sym_posg = nullptr;
  void *sym_send = nullptr, *sym_recv = nullptr;   // exchange buffers (recv == send when the context owns all bodies)
  void *sym_dup_table = nullptr;                   // coincident-body detector (hash slots + flag)
  int sym_dup_slots = 0;
  // fused single-device fp32 stepping: the update prepares the next pass (posg + the OTHER detector table)
  void *sym_dup_table2 = nullptr;
  int sym_dup_cur = 0;                             // which of the two tables holds the verdict on the current positions
  bool sym_posg_valid = false;                     // posg (and that table) describe the current positions
  bool posm_escaped = false;                       // the caller holds / owns the position buffer: it may change behind our back
  // equal-mass kernels: device word the preparation kernel (fp64: mass_check_kernel) raises when two masses differ (sticky; the host resets it
  // with every state it uploads) and what the host itself saw in that state (1 all equal, 0 not, -1 never saw one)
  void *sym_general = nullptr;
  int masses_equal = -1;
  bool own_send = false, own_recv = false;
  bool step_open = false;      // nbody_step_begin done, nbody_step_end pending
  bool step_local = false;     // nbody_step_begin_local done, nbody_step_begin_remote pending
  int64_t steps_done = 0;      // updates applied since the state was set (saved in checkpoints)
  // Barnes-Hut mode (bh_frame.hip, kernels_bh_*.hip; driven by bh_driver.hip)
  float theta = 0.0f;
  nbody::BhState *bh = nullptr;
  int bh_max_depth = 42;       // the deepest tree a frame may build (nbody_set_bh_max_depth): a setting, not state (checkpoints do not keep it)
  void *bh_acc = nullptr;      // [i_count] float4: the walk's output, summed (j_split = 1) by update_kernel
  struct { int queued = 0; bool whole = false; } bh_batch;   // what bh_queue_frame queued since the last bh_collect_frames (whole: frames, not a force-only pass)
  // massless points in the bodies' field (kernels_probe.hip; theta > 0: bh_probe_walk): the tracers the steps carry along
  // (nbody_set_tracers)
  int tr_n = 0;
  void *tr_pos = nullptr, *tr_vel = nullptr, *tr_acc = nullptr;   // [tr_n] float4 each
  void *probe_part = nullptr;  // the j chunks' partial rows of one slab of points (theta == 0), shared by tracers and queries
  size_t probe_part_elems = 0;
  void *tidal64 = nullptr;     // nbody_tidal_time / nbody_tidal_time_f64: [n_total][6] double, the bodies' unrounded tidal tensors, then the reduction's workgroup pairs
  void *jerk64 = nullptr;      // nbody_get_jerk_f64 / nbody_jerk_time: [n_total][6] double, the bodies' unrounded (a, j), then the reduction's workgroup pairs
  void *pot64 = nullptr;       // nbody_energy_fast: [n_total] double, the bodies' unrounded potentials, then the reduction's workgroup pairs
  int radial_resident = 0;     // nbody_radial_order_f64 / nbody_lagrange_radii_f64: workgroups of the radix pass the device holds at once (0: not asked yet)
  // Hermite stepping of fp64 contexts (capi_hermite.hip), every instance indexed by order: [0] fourth (nbody_hermite_*,
  // kernels_hermite.hip, kernels_hermite_block.hip), [1] sixth (nbody_hermite6_*, kernels_snap.hip, kernels_hermite_block.hip)
  nbody::HermiteCache hm[2];          // the bodies' caches
  bool hm_external = false;           // a buffer was bound or a pointer handed out: somebody else may write the state, every call of either order evaluates anew
  nbody::HermiteBlockSession hb[2];   // the block sessions, each on its order's cache
  void *snap64 = nullptr;             // nbody_get_snap_f64: [n_total][9] double, the bodies' (a, j, s), then [n_total] double4, the input accelerations
  // fp64 tracers (nbody_set_tracers_f64, kernels_points64.hip): massless points the four shared-step Hermite calls carry beside the
  // bodies.  tr64 holds, in doubles, pos, vel, acc, xp, vp, ap ([tr64_n] double4 each); trh are their caches.
  int tr64_n = 0;
  void *tr64 = nullptr;
  nbody::HermiteCache trh[2];
  bool bh_tree_valid = false;  // the tree in the Barnes-Hut state's arrays is that of a frame that was built, with bh_tree_theta
  float bh_tree_theta = 0.0f;
  nbody::KernelTimer timers[2];
  int clk_items = 0;                   // NBODY_SYM_ITEM_CLOCKS: work items with stamps of their own behind the eight clock words
  unsigned long long *clk = nullptr;   // time_kernels: {shader-clock cycles, reference-clock ticks} summed over the force kernels' workgroups (pk_common.h)
  int wall_khz = 0, cus = 0;           // hipDeviceAttributeWallClockRate, compute units
  std::string err;
};

namespace nbody {

inline int fail(nbody_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

#define HIP_TRY(c, expr)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return nbody::fail((c), NBODY_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// One caller thread may hold contexts on several devices (nbody_create_multi does): every entry point that allocates,
// launches, copies or records makes its context's device the current one first.
inline int use_device(nbody_ctx *c) {
  if (c->multi) return NBODY_OK;
  HIP_TRY(c, hipSetDevice(c->p.device));
  return NBODY_OK;
}

// One order's caches are no longer the stored state's: the next call of that order evaluates anew and has no higher derivatives, the
// order's block session ends, and the fp64 tracers' cache of that order — evaluated in the field of a state that is no longer the
// stored one — goes with the bodies'.  capi_hermite.hip alone forgets one order without the other (the table in DESIGN.md).
inline void hermite_invalidate_order(nbody_ctx *c, int order_index) {
  c->hm[order_index].valid = c->hm[order_index].derivs = false;
  c->hb[order_index].active = false;
  c->trh[order_index].valid = c->trh[order_index].derivs = false;
}
// The stored (x, v) are about to change by something other than a Hermite step (an upload, a kick-drift step, a caller's pointer): both
// orders forget.
inline void hermite_invalidate(nbody_ctx *c) {
  hermite_invalidate_order(c, 0);
  hermite_invalidate_order(c, 1);
}

// ---- kernel timers (time_kernels): one event pair around every pass, read when nbody_kernel_time asks or the list grows long
constexpr size_t kTimerPendingCap = 1024;   // live event pairs per timer before a drain

inline int timer_drain(nbody_ctx *c, int which) {
  KernelTimer &t = c->timers[which];
  for (const EventPair &e : t.pending) {
    HIP_TRY(c, hipEventSynchronize(e.b));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e.a, e.b));
    t.total_ms += ms;
    t.launches += e.counts ? 1 : 0;
    t.pool.push_back(e);
  }
  t.pending.clear();
  return NBODY_OK;
}

// bound the number of live events on long runs that never read the timer
inline int timer_drain_at_cap(nbody_ctx *c, int which) {
  return c->timers[which].pending.size() >= kTimerPendingCap ? timer_drain(c, which) : NBODY_OK;
}

// The event pairs of the last `k` passes queued belong to passes that did nothing (a Barnes-Hut frame given up or handed back, and
// the ones queued behind it): they are taken back, so that nbody_kernel_time counts every pass once — with the events around the
// run that did the work.
inline void timer_take_back(nbody_ctx *c, int which, int k) {
  KernelTimer &t = c->timers[which];
  for (; k > 0 && !t.pending.empty(); --k) { t.pool.push_back(t.pending.back()); t.pending.pop_back(); }
}

// launch() — a callable that queues one pass on c->stream and returns an NBODY_ code — inside an event pair of timer `which` when the
// context times its kernels, bare otherwise.  counts: the interval is a whole pass.  may_drain: the pending list may be read once it
// reaches the cap; a caller whose passes may still be taken back (a Barnes-Hut batch in flight) defers that to its collect.
template <typename Launch>
int timed_launch(nbody_ctx *c, int which, Launch &&launch, bool counts = true, bool may_drain = true) {
  if (!c->p.time_kernels) return launch();
  KernelTimer &t = c->timers[which];
  if (t.pool.empty()) {
    EventPair e;
    HIP_TRY(c, hipEventCreate(&e.a));
    HIP_TRY(c, hipEventCreate(&e.b));
    t.pool.push_back(e);
  }
  EventPair ev = t.pool.back();
  t.pool.pop_back();
  // a pass that fails to queue, or whose second stamp does, is not counted: its pair goes back to the pool (which nbody_destroy empties)
  const int rc = [&]() -> int {
    HIP_TRY(c, hipEventRecord(ev.a, c->stream));
    if (int launch_rc = launch()) return launch_rc;
    HIP_TRY(c, hipEventRecord(ev.b, c->stream));
    return NBODY_OK;
  }();
  if (rc) { t.pool.push_back(ev); return rc; }
  ev.counts = counts;
  t.pending.push_back(ev);
  return may_drain ? timer_drain_at_cap(c, which) : NBODY_OK;
}

}  // namespace nbody
