// What the C-ABI's host units share: capi.hip's helpers that capi_hermite.hip and capi_query64.hip call (defined there, beside the calls
// that first needed them), and what those two share with each other.
#pragma once
#include "ctx.h"

namespace nbody {

int multi_unsupported(nbody_ctx *c, const char *who);   // the refusal of a call a multi-device context does not answer
int check_ready(nbody_ctx *c);                           // a context, a state set; makes the context's device the current one
int read_energy(nbody_ctx *c, double *ke, double *pe);   // the two doubles a reduction left in the scratch, waited for
int ensure_stage(nbody_ctx *c, size_t bytes);            // the staging pair (d_stage, h_stage), grown on demand
int ensure_probe_part(nbody_ctx *c, int m, int width = 1);   // the partial rows of a slab of m points, grown on demand
void scatter_records(void *dst, size_t stride, const void *src, size_t record_bytes, size_t count, size_t src_stride = 0);
int queue_body_jerk(nbody_ctx *c, double *aj64, float *ajf);   // the bodies' own (a, j): one pass under NBODY_KERNEL_FORCES
int ensure_jerk64(nbody_ctx *c);                         // c->jerk64, at first use

// capi_query64.hip: where the fp64 points exist — the contexts that answer nbody_hermite_step: fp64 state, one device, all bodies — and
// when: a state set, no step half done
int points64_ready(nbody_ctx *c, const char *who);
// n records of three doubles, `stride` bytes apart (NULL: zeros), as double4 rows with a fourth component of 0
void gather_double4(double *dst, const double *src, size_t stride, size_t n);
// a point pass is never queued into a staging area that does not hold a slab's partial rows
int points64_part_holds(nbody_ctx *c, int m, int width, const char *what);

// capi_query64.hip: m points (with_vel: and behind them their velocities, NULL = at rest) as double4 at the head of the staging pair, the
// results behind them: h and d are the pair's two sides, the results start `skip` doubles in (4 m, with_vel: 8 m)
struct Staged64 {
  double *h = nullptr, *d = nullptr;
  size_t m = 0, skip = 0;
};
// the pair grown to hold the points and result_bytes of results, the points gathered and queued to the device in ONE copy
int stage_points64(nbody_ctx *c, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, bool with_vel, size_t m,
                   size_t result_bytes, Staged64 *s);
// `bytes` of the staging pair from double `first` on, device to host, waited for
int stage_to_host(nbody_ctx *c, size_t first, size_t bytes);

}  // namespace nbody
