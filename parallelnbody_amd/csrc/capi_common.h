// What capi_hermite.hip calls of capi.hip's helpers (defined there, beside the calls that first needed them).
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

}  // namespace nbody
