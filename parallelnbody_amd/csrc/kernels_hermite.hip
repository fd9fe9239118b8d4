// Fourth-order Hermite stepping of fp64 contexts (nbody_hermite_step, nbody_hermite_timescale, nbody_hermite_advance; build-defined: the
// reference has one integrator, its kick-drift) — Makino & Aarseth's shared-step P(EC) around the fp64 jerk pass of kernels_jerk.hip,
// which this file neither holds nor changes.  One lane per body, no LDS tiles, no atomics:
//   hermite_predict_kernel     <- (xp, vp) from (x, v, a0, j0): the Taylor series to third / second order
//   hermite_correct_kernel     <- (x, v) from (a0, j0) and the (a1, j1) of the predicted state; the stored acceleration; a2, a3 at the new time
//   hermite_time_parts_kernel  <- Aarseth's k = (|j| |a3| + |a2|^2) / (|a| |a2| + |j|^2) per body, its maximum and that body
//   launch_max_fold            <- the workgroups' pairs folded in a fixed order (kernels_probe.hip)
// The arithmetic of all three is hermite_step64.h's, which the block kernels (kernels_hermite_block.hip) call too.  EVERY operation is
// one correctly rounded fp64 operation, in the order that header writes it: contraction is off for the whole file (the Makefile sets no
// contraction flag), so that plain C or numpy reproduces a step in every bit from the (a, j) of nbody_get_jerk_f64 (tests/hermite_ref.py).
#include "kernels.h"

#include "hermite_step64.h"
#include "point_tile.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// (xp, vp) := hermite4_predict of every body with the call's constants
__global__ __launch_bounds__(kBlock) void hermite_predict_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                 const double *__restrict__ aj0, double4 *__restrict__ xp,
                                                                 double4 *__restrict__ vp, int n, Hermite4Predict k) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  hermite4_predict(k, posm, vel, aj0, xp, vp, i);
}

// hermite4_correct per component with (a1, j1) the row of aj1:  x := x1 (the mass stays), v := v1 (its fourth component stays), acc := (a1, 0),
// a2 := (a2, 0), a3 := (a3, 0)
__global__ __launch_bounds__(kBlock) void hermite_correct_kernel(double4 *__restrict__ posm, double4 *__restrict__ vel,
                                                                 double4 *__restrict__ acc, const double *__restrict__ aj0,
                                                                 const double *__restrict__ aj1, double4 *__restrict__ a2,
                                                                 double4 *__restrict__ a3, int n, Hermite4Correct k) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double4 x = posm[i], v = vel[i];
  const Aj s0 = load_aj(aj0, i), s1 = load_aj(aj1, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  Hermite4Comp r[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) r[q] = hermite4_correct(k, xc[q], vc[q], s0.a[q], s0.j[q], s1.a[q], s1.j[q]);
  posm[i] = make_double4(r[0].x, r[1].x, r[2].x, x.w);
  vel[i] = make_double4(r[0].v, r[1].v, r[2].v, v.w);
  acc[i] = make_double4(s1.a[0], s1.a[1], s1.a[2], 0.0);
  a2[i] = make_double4(r[0].a2, r[1].a2, r[2].a2, 0.0);
  a3[i] = make_double4(r[0].a3, r[1].a3, r[2].a3, 0.0);
}

// nbody_hermite_timescale with derivatives: the ratio hermite4_ratio of A = |a0|, J = |j0|, S = |a2|, C = |a3|, a value that is not finite counting as
// +inf; the candidates (k, body) reduced as jerk_time_parts_kernel reduces its own.
__global__ __launch_bounds__(kBlock) void hermite_time_parts_kernel(const double *__restrict__ aj0, const double4 *__restrict__ a2,
                                                                    const double4 *__restrict__ a3, int n, double *__restrict__ part) {
  __shared__ ValueAt red[kBlock / 64];
  ValueAt m{-1.0, 0x7fffffff};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const Aj s = load_aj(aj0, i);
    const double4 d2 = a2[i], d3 = a3[i];
    value_at_take<true>(m, ratio_k<true>(hermite4_ratio(norm3(s.a[0], s.a[1], s.a[2]), norm3(s.j[0], s.j[1], s.j[2]), norm3(d2), norm3(d3))), i);
  }
  const ValueAt r = value_at_workgroup<true>(m, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = r.v; part[2 * blockIdx.x + 1] = (double)r.i; }
}

inline bool bad(const HermiteLaunch &L) {
  return L.n <= 0 || !L.posm || !L.vel || !L.aj0;
}

}  // namespace

// the constants are the host's own doubles — products and one quotient each, in the order written (nothing a host compiler could fuse)
hipError_t launch_hermite_predict(const HermiteLaunch &L, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite_predict_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double4 *)L.posm,
                     (const double4 *)L.vel, L.aj0, (double4 *)L.xp, (double4 *)L.vp, L.n, hermite4_predict_consts(L.dt));
  return hipGetLastError();
}

hipError_t launch_hermite_correct(const HermiteLaunch &L, hipStream_t s) {
  if (bad(L) || !L.acc || !L.aj1 || !L.a2 || !L.a3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite_correct_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (double4 *)L.posm, (double4 *)L.vel,
                     (double4 *)L.acc, L.aj0, L.aj1, (double4 *)L.a2, (double4 *)L.a3, L.n, hermite4_correct_consts(L.dt));
  return hipGetLastError();
}

hipError_t launch_hermite_time(const double *aj0, const void *a2, const void *a3, int n, double *partials, double *out, hipStream_t s) {
  if (n <= 0 || !aj0 || !a2 || !a3 || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(hermite_time_parts_kernel, dim3(slots), dim3(kBlock), 0, s, aj0, (const double4 *)a2, (const double4 *)a3, n, partials);
  return launch_max_fold(partials, slots, out, s);
}

}  // namespace nbody
