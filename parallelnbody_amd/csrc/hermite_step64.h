// The arithmetic of one Hermite step of one body, written ONCE per order: the shared-step kernels (kernels_hermite.hip, kernels_snap.hip)
// call it with the host's constants of the call's dt, the block kernels (kernels_hermite_block.hip) with the constants of the body's own
// dt.  The constants come from one maker per struct — the same products and one quotient in the same order on the host and on the device,
// no sum in any of them, so nothing a compiler could fuse — and a predictor's and a corrector's constants stay two structs: they are the
// shared-step kernels' arguments as they were.  EVERY operation here is one correctly rounded fp64 operation in the order written:
// contraction is off for this header and for every file that includes it, so that numpy (tests/hermite*_ref.py) reproduces a step in
// every bit.  The helpers take scalars and small structs BY VALUE and return values: one that reads a struct or an array through a
// reference gave the same instructions in another order, which the kernels' comparison with their written-out forms
// does not allow.
#pragma once
#include "kernels.h"

#pragma clang fp contract(off)

namespace nbody {
namespace {

// a body's (ax, ay, az, jx, jy, jz) in the jerk fold's rows: six doubles, 48 bytes apart — three 16-byte accesses
struct Aj { double a[3], j[3]; };
__device__ __forceinline__ Aj load_aj(const double *__restrict__ aj, int i) {
  const double2 *r = (const double2 *)(aj + 6 * (size_t)i);
  const double2 r0 = r[0], r1 = r[1], r2 = r[2];
  return Aj{{r0.x, r0.y, r1.x}, {r1.y, r2.x, r2.y}};
}
// a body's (a, j, s) in the snap fold's rows: nine doubles, 72 bytes apart
struct Ajs { double a[3], j[3], s[3]; };
__device__ __forceinline__ Ajs load_ajs(const double *__restrict__ ajs, int i) {
  const double *r = ajs + 9 * (size_t)i;
  return Ajs{{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}};
}
// a cached row by its width: Aj for six doubles, Ajs for nine
template <int ROW>
__device__ __forceinline__ auto load_row(const double *__restrict__ rows, int i) {
  static_assert(ROW == 6 || ROW == 9, "a jerk row or a snap row");
  if constexpr (ROW == 6) return load_aj(rows, i);
  else return load_ajs(rows, i);
}

// ---- the time scales ----
// |x| = sqrt((x x + y y) + z z) and its square; a criterion's two sums, and k = num / den with 0 / 0 = 0 and x / 0 = +inf — CLAMP: a
// value that is not finite (a NaN too) counts as +inf —; the step 1 / sqrt(k) a k stands for: +inf for k == 0, 0 for a k that is not finite
__device__ __forceinline__ double sqnorm3(double x, double y, double z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(sqnorm3(x, y, z)); }
__device__ __forceinline__ double norm3(double4 c) { return norm3(c.x, c.y, c.z); }
struct Ratio { double num, den; };
template <bool CLAMP>
__device__ __forceinline__ double ratio_k(Ratio r) {
  double k = (r.num == 0.0 && r.den == 0.0) ? 0.0 : r.num / r.den;
  if (CLAMP && !(k <= 0x1.fffffffffffffp1023)) k = __builtin_inf();
  return k;
}
__device__ __forceinline__ double time_of_k(double k) {
  if (k == 0.0) return __builtin_inf();
  if (!(k <= 0x1.fffffffffffffp1023)) return 0.0;
  return 1.0 / sqrt(k);
}

// ---- fourth order (Makino & Aarseth) ----
// per component  xp = ((x + dt v) + c2 a0) + c3 j0;  vp = (v + dt a0) + c2 j0;  xp.w = m, vp.w = 0
struct Hermite4Predict { double dt, c2, c3; };
__host__ __device__ __forceinline__ Hermite4Predict hermite4_predict_consts(double dt) {
  return Hermite4Predict{dt, (dt * dt) * 0.5, ((dt * dt) * dt) / 6.0};
}
__device__ __forceinline__ void hermite4_predict(const Hermite4Predict &k, const double4 *posm, const double4 *vel, const double *aj0,
                                                 double4 *xp, double4 *vp, int i) {
  const double4 x = posm[i], v = vel[i];
  const Aj s = load_aj(aj0, i);
  auto px = [&](double xc, double vc, double a, double j) { return ((xc + k.dt * vc) + k.c2 * a) + k.c3 * j; };
  auto pv = [&](double vc, double a, double j) { return (vc + k.dt * a) + k.c2 * j; };
  xp[i] = make_double4(px(x.x, v.x, s.a[0], s.j[0]), px(x.y, v.y, s.a[1], s.j[1]), px(x.z, v.z, s.a[2], s.j[2]), x.w);
  vp[i] = make_double4(pv(v.x, s.a[0], s.j[0]), pv(v.y, s.a[1], s.j[1]), pv(v.z, s.a[2], s.j[2]), 0.0);
}

// one component, with (a1, j1) the jerk pass's answer at (xp, vp) — a second row's, or a block corrector's folded sums —:
//   v1 = v + (ch (a0 + a1) + c12 (j0 - j1));   x1 = x + (ch (v + v1) + c12 (a0 - a1));   da = a0 - a1
//   a2_0 = ((-6 da) - dt ((4 j0) + (2 j1))) / d2;   a3 = ((12 da) + (6 dt) (j0 + j1)) / d3;   a2 = a2_0 + dt a3 (a2, a3 at the new time)
struct Hermite4Correct { double dt, ch, c12, d2, d3; };
__host__ __device__ __forceinline__ Hermite4Correct hermite4_correct_consts(double dt) {
  return Hermite4Correct{dt, dt * 0.5, (dt * dt) / 12.0, dt * dt, (dt * dt) * dt};
}
struct Hermite4Comp { double x, v, a2, a3; };
__device__ __forceinline__ Hermite4Comp hermite4_correct(const Hermite4Correct &k, double x, double v, double a0, double j0, double a1,
                                                         double j1) {
  Hermite4Comp r;
  r.v = v + (k.ch * (a0 + a1) + k.c12 * (j0 - j1));
  r.x = x + (k.ch * (v + r.v) + k.c12 * (a0 - a1));
  const double da = a0 - a1;
  const double a20 = ((-6.0 * da) - k.dt * ((4.0 * j0) + (2.0 * j1))) / k.d2;
  r.a3 = ((12.0 * da) + (6.0 * k.dt) * (j0 + j1)) / k.d3;
  r.a2 = a20 + k.dt * r.a3;
  return r;
}
// Aarseth's k = (|j| |a3| + |a2|^2) / (|a| |a2| + |j|^2) from the four norms
__device__ __forceinline__ Ratio hermite4_ratio(double A, double J, double S, double C) {
  return Ratio{J * C + S * S, A * S + J * J};
}

// ---- sixth order (Nitadori & Makino) ----
// per component  xp = ((((x + dt v) + c2 a0) + c3 j0) + c4 s0) + c5 a3;  vp = (((v + dt a0) + c2 j0) + c3 s0) + c4 a3;
// ap = ((a0 + dt j0) + c2 s0) + c3 a3;  xp.w = m, vp.w = 0, ap.w = 0
struct Hermite6Predict { double dt, c2, c3, c4, c5; };
__host__ __device__ __forceinline__ Hermite6Predict hermite6_predict_consts(double dt) {
  const double d2 = dt * dt;
  return Hermite6Predict{dt, d2 * 0.5, (d2 * dt) / 6.0, (d2 * d2) / 24.0, ((d2 * d2) * dt) / 120.0};
}
__device__ __forceinline__ void hermite6_predict(const Hermite6Predict &k, const double4 *posm, const double4 *vel, const double *ajs0,
                                                 const double4 *a3, double4 *xp, double4 *vp, double4 *ap, int i) {
  const double4 x = posm[i], v = vel[i], d3 = a3[i];
  const Ajs s = load_ajs(ajs0, i);
  auto px = [&](double xc, double vc, double a, double j, double sn, double c) {
    return ((((xc + k.dt * vc) + k.c2 * a) + k.c3 * j) + k.c4 * sn) + k.c5 * c;
  };
  auto pv = [&](double vc, double a, double j, double sn, double c) { return (((vc + k.dt * a) + k.c2 * j) + k.c3 * sn) + k.c4 * c; };
  auto pa = [&](double a, double j, double sn, double c) { return ((a + k.dt * j) + k.c2 * sn) + k.c3 * c; };
  xp[i] = make_double4(px(x.x, v.x, s.a[0], s.j[0], s.s[0], d3.x), px(x.y, v.y, s.a[1], s.j[1], s.s[1], d3.y),
                       px(x.z, v.z, s.a[2], s.j[2], s.s[2], d3.z), x.w);
  vp[i] = make_double4(pv(v.x, s.a[0], s.j[0], s.s[0], d3.x), pv(v.y, s.a[1], s.j[1], s.s[1], d3.y), pv(v.z, s.a[2], s.j[2], s.s[2], d3.z), 0.0);
  ap[i] = make_double4(pa(s.a[0], s.j[0], s.s[0], d3.x), pa(s.a[1], s.j[1], s.s[1], d3.y), pa(s.a[2], s.j[2], s.s[2], d3.z), 0.0);
}

// one component, with (a1, j1, s1) the snap pass's answer at (xp, vp) given ap — a second row's, or a block corrector's folded sums —:
//   v1 = v + ((ch (a0 + a1) + c10 (j0 - j1)) + c120 (s0 + s1));   x1 = x + ((ch (v + v1) + c10 (a0 - a1)) + c120 (j0 + j1))
//   R1 = ((a1 - a0) - dt j0) - c2 s0;   R2 = dt ((j1 - j0) - dt s0);   R3 = d2 (s1 - s0)
//   X = ((60 R1) - (24 R2)) + (3 R3);   Y = ((168 R2) - (360 R1)) - (24 R3);   Z = ((720 R1) - (360 R2)) + (60 R3)
//   a3 = ((X + Y) + 0.5 Z) / d3;   a4 = (Y + Z) / d4;   a5 = Z / d5   (at the new time, from the quintic through both ends)
struct Hermite6Correct { double dt, ch, c2, c10, c120, d2, d3, d4, d5; };
__host__ __device__ __forceinline__ Hermite6Correct hermite6_correct_consts(double dt) {
  const double d2 = dt * dt, d4 = d2 * d2;
  return Hermite6Correct{dt, dt * 0.5, d2 * 0.5, d2 / 10.0, (d2 * dt) / 120.0, d2, d2 * dt, d4, d4 * dt};
}
struct Hermite6Comp { double x, v, a3, a4, a5; };
__device__ __forceinline__ Hermite6Comp hermite6_correct(const Hermite6Correct &k, double x, double v, double a0, double j0, double s0,
                                                         double a1, double j1, double s1) {
  Hermite6Comp r;
  r.v = v + ((k.ch * (a0 + a1) + k.c10 * (j0 - j1)) + k.c120 * (s0 + s1));
  r.x = x + ((k.ch * (v + r.v) + k.c10 * (a0 - a1)) + k.c120 * (j0 + j1));
  const double R1 = ((a1 - a0) - k.dt * j0) - k.c2 * s0;
  const double R2 = k.dt * ((j1 - j0) - k.dt * s0);
  const double R3 = k.d2 * (s1 - s0);
  const double X = ((60.0 * R1) - (24.0 * R2)) + (3.0 * R3);
  const double Y = ((168.0 * R2) - (360.0 * R1)) - (24.0 * R3);
  const double Z = ((720.0 * R1) - (360.0 * R2)) + (60.0 * R3);
  r.a3 = ((X + Y) + 0.5 * Z) / k.d3;
  r.a4 = (Y + Z) / k.d4;
  r.a5 = Z / k.d5;
  return r;
}
// k = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2) from the six norms
__device__ __forceinline__ Ratio hermite6_ratio(double A0, double J0, double S0, double A3, double A4, double A5) {
  return Ratio{A3 * A5 + A4 * A4, A0 * S0 + J0 * J0};
}

}  // namespace
}  // namespace nbody
