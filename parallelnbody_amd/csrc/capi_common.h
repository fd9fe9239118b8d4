// What the C-ABI's host units call of each other, each helper under the unit that defines it: capi.hip (the context's life, stream and
// buffers, Barnes-Hut settings, info getters, timers, debug calls), capi_state.hip (state in and out), capi_step.hip (the passes and what
// drives them), capi_query.hip (the fp32 queries, the jerk, the fp32 tracers), capi_query64.hip (the fp64 queries), capi_hermite.hip.
#pragma once
#include <cstring>

#include "ctx.h"

namespace nbody {
// every point query's staging: n records of three T (float, double), `stride` bytes apart (NULL: zeros), as rows of four with a fourth of 0
template <typename T>
void gather4(T *dst, const T *src, size_t stride, size_t n) {
  for (size_t k = 0; k < n; ++k) {
    if (src) memcpy(dst + 4 * k, (const char *)src + k * stride, 3 * sizeof(T));
    else     dst[4 * k] = dst[4 * k + 1] = dst[4 * k + 2] = T(0);
    dst[4 * k + 3] = T(0);
  }
}

// `count` staged records of record_bytes each (src_stride apart: packed unless given) -> the caller's array, records `stride` bytes apart
// (inline: where a call's record size is a constant, a million records are moves, not calls of memcpy: 0.35 ms of nbody_field_at's 2.8)
inline void scatter_records(void *dst, size_t stride, const void *src, size_t record_bytes, size_t count, size_t src_stride = 0) {
  if (src_stride == 0) src_stride = record_bytes;
  if (stride == record_bytes && src_stride == record_bytes) {
    memcpy(dst, src, count * record_bytes);
    return;
  }
  for (size_t i = 0; i < count; ++i) memcpy((char *)dst + i * stride, (const char *)src + i * src_stride, record_bytes);
}

// ---- capi.hip ----
int multi_unsupported(nbody_ctx *c, const char *who);   // the refusal of a call a multi-device context does not answer
int multi_rc(nbody_ctx *c, int rc);                      // a call a multi-device context's Multi answered: its message becomes the context's
int check_ready(nbody_ctx *c);                           // a context, a state set; makes the context's device the current one
int read_energy(nbody_ctx *c, double *ke, double *pe);   // the two doubles a reduction left in the scratch, waited for
int ensure_stage(nbody_ctx *c, size_t bytes);            // the staging pair (d_stage, h_stage), grown on demand
int ensure_probe_part(nbody_ctx *c, int m, int width = 1);   // the partial rows of a slab of m points, grown on demand

// ---- capi_state.hip ----
int queue_particle_mirror(nbody_ctx *c, void *aos, size_t stride, bool *direct);   // the owned bodies' FParticle records, packed and queued to the caller's pinned mirror or the staging pair
int mirror_device_ptr(nbody_ctx *c, void *aos, size_t stride, bool align16, bool *direct, void **dev);   // ... the device pointer of whichever of the two a launch writes them into itself

// ---- capi_step.hip ----
ForceLaunch make_launch(const nbody_ctx *c);             // the one-sided passes' launch struct of the context as it stands
int ensure_floor(nbody_ctx *c);                          // NBODY_ZERO_FLOOR: the eps^2 floor of the current masses, computed once per state
int queue_probe(nbody_ctx *c, void *pts, void *vel, void *acc, int m, float dt);   // theta == 0: the bodies' field at m points, queued
int run_forces(nbody_ctx *c, bool diagnostic = false, int phase = 0, float tracer_dt = -1.0f);   // one force pass of either theta
int run_update(nbody_ctx *c, float dt);                  // the update behind it
int posm_escapes(nbody_ctx *c);                          // the caller gets hold of the position buffer: fused and one-launch stepping end

// ---- capi_query.hip ----
int queue_body_jerk(nbody_ctx *c, double *aj64, float *ajf);   // the bodies' own (a, j): one pass under NBODY_KERNEL_FORCES
int ensure_rows64(nbody_ctx *c, void **buf, int width);   // *buf (pot64, tidal64, jerk64), at first use: the bodies' unrounded rows, [n_total][width] double, then the workgroup pairs of the reduction over them
int tidal_time_out(nbody_ctx *c, double *t_min, int32_t *body);   // the tail of nbody_tidal_time[_f64]: the tensors in tidal64 reduced, t = n2^(-1/4), its body

// ---- capi_query64.hip ----
// where the fp64 points exist — the contexts that answer nbody_hermite_step: fp64 state, one device, all bodies — and when: a state set,
// no step half done
int points64_ready(nbody_ctx *c, const char *who);
// a point pass is never queued into a staging area that does not hold a slab's partial rows
int points64_part_holds(nbody_ctx *c, int m, int width, const char *what);

// m points (with_vel: and behind them their velocities, NULL = at rest) as double4 at the head of the staging pair, the results behind
// them: h and d are the pair's two sides, the results start `skip` doubles in (4 m, with_vel: 8 m)
struct Staged64 {
  double *h = nullptr, *d = nullptr;
  size_t m = 0, skip = 0;
};
// the pair grown to hold the points and result_bytes of results, the points gathered and queued to the device in ONE copy
int stage_points64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, bool with_vel, size_t m,
                   size_t result_bytes, Staged64 *s);
// `bytes` of the staging pair from byte `first` on, device to host, waited for
int stage_to_host(nbody_ctx *c, size_t first, size_t bytes);

}  // namespace nbody
