// Fourth-order Hermite stepping of fp64 contexts (nbody_hermite_step, nbody_hermite_timescale, nbody_hermite_advance; build-defined: the
// reference has one integrator, its kick-drift) — Makino & Aarseth's shared-step P(EC) around the fp64 jerk pass of kernels_jerk.hip,
// which this file neither holds nor changes.  One lane per body, no LDS tiles, no atomics:
//   hermite_predict_kernel     <- (xp, vp) from (x, v, a0, j0): the Taylor series to third / second order
//   hermite_correct_kernel     <- (x, v) from (a0, j0) and the (a1, j1) of the predicted state; the stored acceleration; a2, a3 at the new time
//   hermite_time_parts_kernel  <- Aarseth's k = (|j| |a3| + |a2|^2) / (|a| |a2| + |j|^2) per body, its maximum and that body
//   hermite_time_fold_kernel   <- the workgroups' pairs folded in a fixed order (point_tile.h: tidal_max_*)
// EVERY operation of these kernels is one correctly rounded fp64 operation, in the order the comments write it: contraction is off for
// the whole file (the Makefile sets no contraction flag), so that plain C or numpy reproduces a step in every bit from the (a, j) of
// nbody_get_jerk_f64 (tests/hermite_ref.py).
#include "kernels.h"

#include "point_tile.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// a body's (ax, ay, az, jx, jy, jz) in the jerk fold's rows: six doubles, 48 bytes apart — three 16-byte loads
struct Aj { double a[3], j[3]; };
__device__ __forceinline__ Aj load_aj(const double *__restrict__ aj, int i) {
  const double2 *r = (const double2 *)(aj + 6 * (size_t)i);
  const double2 r0 = r[0], r1 = r[1], r2 = r[2];
  return Aj{{r0.x, r0.y, r1.x}, {r1.y, r2.x, r2.y}};
}

// per component  xp = ((x + c1 v) + c2 a0) + c3 j0;  vp = (v + c1 a0) + c2 j0;  xp.w = m, vp.w = 0
__global__ __launch_bounds__(kBlock) void hermite_predict_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                 const double *__restrict__ aj0, double4 *__restrict__ xp,
                                                                 double4 *__restrict__ vp, int n, double c1, double c2, double c3) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double4 x = posm[i], v = vel[i];
  const Aj s = load_aj(aj0, i);
  auto px = [&](double xc, double vc, double a, double j) { return ((xc + c1 * vc) + c2 * a) + c3 * j; };
  auto pv = [&](double vc, double a, double j) { return (vc + c1 * a) + c2 * j; };
  xp[i] = make_double4(px(x.x, v.x, s.a[0], s.j[0]), px(x.y, v.y, s.a[1], s.j[1]), px(x.z, v.z, s.a[2], s.j[2]), x.w);
  vp[i] = make_double4(pv(v.x, s.a[0], s.j[0]), pv(v.y, s.a[1], s.j[1]), pv(v.z, s.a[2], s.j[2]), 0.0);
}

// per component, with (a1, j1) the jerk pass's answer at (xp, vp):
//   v1 = v + (ch (a0 + a1) + c12 (j0 - j1));   x1 = x + (ch (v + v1) + c12 (a0 - a1));   da = a0 - a1
//   a2_0 = ((-6 da) - dt ((4 j0) + (2 j1))) / d2;   a3 = ((12 da) + (6 dt) (j0 + j1)) / d3;   a2_1 = a2_0 + dt a3
// x := x1 (the mass stays), v := v1 (its fourth component stays), acc := (a1, 0), a2 := (a2_1, 0), a3 := (a3, 0)
struct HermiteConsts { double dt, ch, c12, d2, d3; };
__global__ __launch_bounds__(kBlock) void hermite_correct_kernel(double4 *__restrict__ posm, double4 *__restrict__ vel,
                                                                 double4 *__restrict__ acc, const double *__restrict__ aj0,
                                                                 const double *__restrict__ aj1, double4 *__restrict__ a2,
                                                                 double4 *__restrict__ a3, int n, HermiteConsts k) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double4 x = posm[i], v = vel[i];
  const Aj s0 = load_aj(aj0, i), s1 = load_aj(aj1, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  double x1[3], v1[3], q2[3], q3[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    v1[q] = vc[q] + (k.ch * (s0.a[q] + s1.a[q]) + k.c12 * (s0.j[q] - s1.j[q]));
    x1[q] = xc[q] + (k.ch * (vc[q] + v1[q]) + k.c12 * (s0.a[q] - s1.a[q]));
    const double da = s0.a[q] - s1.a[q];
    const double a20 = ((-6.0 * da) - k.dt * ((4.0 * s0.j[q]) + (2.0 * s1.j[q]))) / k.d2;
    q3[q] = ((12.0 * da) + (6.0 * k.dt) * (s0.j[q] + s1.j[q])) / k.d3;
    q2[q] = a20 + k.dt * q3[q];
  }
  posm[i] = make_double4(x1[0], x1[1], x1[2], x.w);
  vel[i] = make_double4(v1[0], v1[1], v1[2], v.w);
  acc[i] = make_double4(s1.a[0], s1.a[1], s1.a[2], 0.0);
  a2[i] = make_double4(q2[0], q2[1], q2[2], 0.0);
  a3[i] = make_double4(q3[0], q3[1], q3[2], 0.0);
}

// nbody_hermite_timescale with derivatives: norms sqrt((x x + y y) + z z) — A = |a0|, J = |j0|, S = |a2|, C = |a3| —, k = (J C + S S) /
// (A S + J J) with 0 / 0 = 0, x / 0 = +inf, and a value that is not finite counting as +inf; the candidates (k, body) reduced as
// jerk_time_parts_kernel reduces its own.
__global__ __launch_bounds__(kBlock) void hermite_time_parts_kernel(const double *__restrict__ aj0, const double4 *__restrict__ a2,
                                                                    const double4 *__restrict__ a3, int n, double *__restrict__ part) {
  __shared__ TidalMax red[kBlock / 64];
  TidalMax m{-1.0, 0x7fffffff};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const Aj s = load_aj(aj0, i);
    const double4 d2 = a2[i], d3 = a3[i];
    const double A = sqrt((s.a[0] * s.a[0] + s.a[1] * s.a[1]) + s.a[2] * s.a[2]);
    const double J = sqrt((s.j[0] * s.j[0] + s.j[1] * s.j[1]) + s.j[2] * s.j[2]);
    const double S = sqrt((d2.x * d2.x + d2.y * d2.y) + d2.z * d2.z);
    const double C = sqrt((d3.x * d3.x + d3.y * d3.y) + d3.z * d3.z);
    const double num = J * C + S * S, den = A * S + J * J;
    double k = (num == 0.0 && den == 0.0) ? 0.0 : num / den;
    if (!(k <= 0x1.fffffffffffffp1023)) k = __builtin_inf();
    tidal_max_take(m, k, i);
  }
  const TidalMax r = tidal_max_workgroup(m, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = r.v; part[2 * blockIdx.x + 1] = (double)r.i; }
}
__global__ __launch_bounds__(kBlock) void hermite_time_fold_kernel(const double *__restrict__ part, int slots, double *__restrict__ out) {
  __shared__ TidalMax red[kBlock / 64];
  TidalMax m{-1.0, 0x7fffffff};
  for (int q = threadIdx.x; q < slots; q += kBlock) tidal_max_take(m, part[2 * q], (int)part[2 * q + 1]);
  const TidalMax r = tidal_max_workgroup(m, red);
  if (threadIdx.x == 0) { out[0] = r.v; out[1] = (double)r.i; }
}

inline bool bad(const HermiteLaunch &L) {
  return L.n <= 0 || !L.posm || !L.vel || !L.aj0;
}

}  // namespace

// the constants are the host's own doubles — products and one quotient each, in the order written (nothing a host compiler could fuse)
hipError_t launch_hermite_predict(const HermiteLaunch &L, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp) return hipErrorInvalidValue;
  const double dt = L.dt;
  const double c2 = (dt * dt) * 0.5, c3 = ((dt * dt) * dt) / 6.0;
  hipLaunchKernelGGL(hermite_predict_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double4 *)L.posm,
                     (const double4 *)L.vel, L.aj0, (double4 *)L.xp, (double4 *)L.vp, L.n, dt, c2, c3);
  return hipGetLastError();
}

hipError_t launch_hermite_correct(const HermiteLaunch &L, hipStream_t s) {
  if (bad(L) || !L.acc || !L.aj1 || !L.a2 || !L.a3) return hipErrorInvalidValue;
  const double dt = L.dt;
  const HermiteConsts k{dt, dt * 0.5, (dt * dt) / 12.0, dt * dt, (dt * dt) * dt};
  hipLaunchKernelGGL(hermite_correct_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (double4 *)L.posm, (double4 *)L.vel,
                     (double4 *)L.acc, L.aj0, L.aj1, (double4 *)L.a2, (double4 *)L.a3, L.n, k);
  return hipGetLastError();
}

hipError_t launch_hermite_time(const double *aj0, const void *a2, const void *a3, int n, double *partials, double *out, hipStream_t s) {
  if (n <= 0 || !aj0 || !a2 || !a3 || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(hermite_time_parts_kernel, dim3(slots), dim3(kBlock), 0, s, aj0, (const double4 *)a2, (const double4 *)a3, n, partials);
  hipLaunchKernelGGL(hermite_time_fold_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)partials, slots, out);
  return hipGetLastError();
}

}  // namespace nbody
