// The snap s = d^2 a / dt^2 of the pair law beside the acceleration and the jerk, and sixth-order Hermite stepping on it (nbody_get_snap_f64,
// nbody_hermite6_step, nbody_hermite6_timescale, nbody_hermite6_advance, nbody_hermite6_get; build-defined: the reference computes none).
// fp64 state, the bodies only.  With d = x_j - x_i, w = v_j - v_i, b = acc_j - acc_i (acc: a per-body INPUT array), s^2 = |d|^2 + eps^2,
// t = 1 / s, al = (d . w) t^2, be = (w . w + d . b) t^2 + al^2:
//     A_ij = G m_j d t^3      J_ij = G m_j w t^3 - 3 al A_ij      S_ij = G m_j b t^3 - 6 al J_ij - 3 be A_ij
//   deriv_tile_f64_kernel   <- (deriv_tile64.h) the <SOFT, kSnapIpt, false, false, true> form of the jerk pass's own kernel template: the g and S
//                              chains beside its A and J chains — so the A and J of a snap pass are nbody_get_jerk_f64's in every bit —; a
//                              third pair of LDS tiles holds the input accelerations
//   snap_fold_f64_kernel    <- the chunks' rows, nine doubles per body, added in chunk order
//   hermite6_predict_kernel <- (xp, vp, ap) from (x, v, a0, j0, s0, a3): the Taylor series to fifth / fourth / third order
//   hermite6_correct_kernel <- (x, v) from (a0, j0, s0) and the (a1, j1, s1) of the predicted state; the stored acceleration; a3, a4, a5
//                              at the new time, from the quintic through both ends
//   hermite6_time_parts_kernel <- k = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2) per body — without derivatives |j0|^2 / |a0|^2 —, its
//                              maximum and that body, folded in a fixed order by launch_max_fold (kernels_probe.hip)
// The arithmetic of the stepping kernels is hermite_step64.h's, which the block kernels (kernels_hermite_block.hip) call too.
// Contraction is off for the whole file: every fused multiply-add of the tile loop is written out as fma(), and EVERY operation of the
// stepping kernels is one correctly rounded fp64 operation in the order that header writes it, so that numpy reproduces a step in
// every bit from the (a, j, s) of nbody_get_snap_f64 (tests/hermite6_ref.py).  No scratch, no atomics, no grid-wide waits.
#include "kernels.h"

#include <algorithm>

#include "deriv_tile64.h"
#include "hermite_step64.h"
#include "point_tile.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

#ifndef NBODY_SNAP_IPT
#define NBODY_SNAP_IPT 2        // (an A/B build may say 1: make variant NAME=ipt1 EXTRA=-DNBODY_SNAP_IPT=1)
#endif
constexpr int kSnapIpt = NBODY_SNAP_IPT;   // bodies per lane (profiles/hermite6_kernel_resources.txt)
static_assert(kSnapIpt == 1 || kSnapIpt == 2, "one or two bodies per lane");

// (a, j, s)[k] from the chunks' rows: the nine sums added from 0.0 in chunk order (no atomics: the same bits every time)
__global__ __launch_bounds__(kBlock) void snap_fold_f64_kernel(const double *__restrict__ part, int m, int j_split, double *__restrict__ ajs64) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) s[q] = s[q] + row[q];
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) ajs64[(size_t)k * 9 + q] = s[q];
}

// ---- sixth-order Hermite stepping: one lane per body ----

// (xp, vp, ap) := hermite6_predict of every body with the call's constants
__global__ __launch_bounds__(kBlock) void hermite6_predict_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                  const double *__restrict__ ajs0, const double4 *__restrict__ a3,
                                                                  double4 *__restrict__ xp, double4 *__restrict__ vp,
                                                                  double4 *__restrict__ ap, int n, Hermite6Predict k) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  hermite6_predict(k, posm, vel, ajs0, a3, xp, vp, ap, i);
}

// hermite6_correct per component with (a1, j1, s1) the row of ajs1:  x := x1 (the mass stays), v := v1 (its fourth component stays), acc := (a1, 0),
// a3, a4, a5 := (those, 0)
__global__ __launch_bounds__(kBlock) void hermite6_correct_kernel(double4 *__restrict__ posm, double4 *__restrict__ vel,
                                                                  double4 *__restrict__ acc, const double *__restrict__ ajs0,
                                                                  const double *__restrict__ ajs1, double4 *__restrict__ a3,
                                                                  double4 *__restrict__ a4, double4 *__restrict__ a5, int n,
                                                                  Hermite6Correct k) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double4 x = posm[i], v = vel[i];
  const Ajs s0 = load_ajs(ajs0, i), s1 = load_ajs(ajs1, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  Hermite6Comp r[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) r[q] = hermite6_correct(k, xc[q], vc[q], s0.a[q], s0.j[q], s0.s[q], s1.a[q], s1.j[q], s1.s[q]);
  posm[i] = make_double4(r[0].x, r[1].x, r[2].x, x.w);
  vel[i] = make_double4(r[0].v, r[1].v, r[2].v, v.w);
  acc[i] = make_double4(s1.a[0], s1.a[1], s1.a[2], 0.0);
  a3[i] = make_double4(r[0].a3, r[1].a3, r[2].a3, 0.0);
  a4[i] = make_double4(r[0].a4, r[1].a4, r[2].a4, 0.0);
  a5[i] = make_double4(r[0].a5, r[1].a5, r[2].a5, 0.0);
}

// nbody_hermite6_timescale's candidates (k, body), reduced as jerk_time_parts_kernel reduces its own.  derivs: hermite6_ratio of the six
// norms; else nbody_jerk_time's k = |j0|^2 / |a0|^2 of the squared norms.  0 / 0 = 0, x / 0 = +inf, and a value that is not finite
// counts as +inf.
__global__ __launch_bounds__(kBlock) void hermite6_time_parts_kernel(const double *__restrict__ ajs0, const double4 *__restrict__ a3,
                                                                     const double4 *__restrict__ a4, const double4 *__restrict__ a5,
                                                                     int n, int derivs, double *__restrict__ part) {
  __shared__ ValueAt red[kBlock / 64];
  ValueAt m{-1.0, 0x7fffffff};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const Ajs s = load_ajs(ajs0, i);
    Ratio r;
    if (derivs) {
      const double4 d3 = a3[i], d4 = a4[i], d5 = a5[i];
      r = hermite6_ratio(norm3(s.a[0], s.a[1], s.a[2]), norm3(s.j[0], s.j[1], s.j[2]), norm3(s.s[0], s.s[1], s.s[2]), norm3(d3), norm3(d4), norm3(d5));
    } else {
      r = Ratio{sqnorm3(s.j[0], s.j[1], s.j[2]), sqnorm3(s.a[0], s.a[1], s.a[2])};
    }
    value_at_take<true>(m, ratio_k<true>(r), i);
  }
  const ValueAt r = value_at_workgroup<true>(m, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = r.v; part[2 * blockIdx.x + 1] = (double)r.i; }
}

inline bool bad(const Hermite6Launch &L) {
  return L.n <= 0 || !L.posm || !L.vel || !L.ajs0 || !L.a3;
}

}  // namespace

hipError_t launch_snap(const SnapLaunch &L, hipStream_t s) {
  if (L.n_total <= 0 || !L.posm || !L.vel || !L.ain || L.ain_stride < 3 || !L.part || !L.ajs64) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;                              // eps == 0: the exact d == 0 rule, as the jerk
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total, kSnapRowWidth);
  for (size_t first = 0; first < (size_t)L.n_total; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.n_total - first);
    const dim3 grid((m + kBlock * kSnapIpt - 1) / (kBlock * kSnapIpt), j_split);
    hipLaunchKernelGGL((soft ? deriv_tile_f64_kernel<true, kSnapIpt, false, false, true> : deriv_tile_f64_kernel<false, kSnapIpt, false, false, true>),
                       grid, dim3(kBlock), 0, s,
                       DerivArgs<false, true>{(const double4 *)L.posm, (const double4 *)L.vel, L.ain, L.ain_stride, L.n_total, m, (int)first, j_chunk, L.G,
                                              L.eps2, nullptr},
                       (double *)L.part);
    hipLaunchKernelGGL(snap_fold_f64_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)L.part, m, j_split,
                       L.ajs64 + 9 * first);
  }
  return hipGetLastError();
}

// snap_fold_f64_kernel on its own, for the rows another file's kernel wrote in this layout (kernels_points64.hip: the point form)
hipError_t launch_snap_fold_f64(const void *part, int m, int j_split, double *ajs64, hipStream_t s) {
  if (m <= 0 || j_split <= 0 || !part || !ajs64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(snap_fold_f64_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)part, m, j_split, ajs64);
  return hipGetLastError();
}

// the constants are the host's own doubles — products and one quotient each, in the order written (nothing a host compiler could fuse)
hipError_t launch_hermite6_predict(const Hermite6Launch &L, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp || !L.ap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite6_predict_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double4 *)L.posm,
                     (const double4 *)L.vel, L.ajs0, (const double4 *)L.a3, (double4 *)L.xp, (double4 *)L.vp, (double4 *)L.ap, L.n,
                     hermite6_predict_consts(L.dt));
  return hipGetLastError();
}

hipError_t launch_hermite6_correct(const Hermite6Launch &L, hipStream_t s) {
  if (bad(L) || !L.acc || !L.ajs1 || !L.a4 || !L.a5) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite6_correct_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (double4 *)L.posm, (double4 *)L.vel,
                     (double4 *)L.acc, L.ajs0, L.ajs1, (double4 *)L.a3, (double4 *)L.a4, (double4 *)L.a5, L.n,
                     hermite6_correct_consts(L.dt));
  return hipGetLastError();
}

hipError_t launch_hermite6_time(const double *ajs0, const void *a3, const void *a4, const void *a5, int n, bool derivs, double *partials,
                                double *out, hipStream_t s) {
  if (n <= 0 || !ajs0 || !a3 || !a4 || !a5 || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(hermite6_time_parts_kernel, dim3(slots), dim3(kBlock), 0, s, ajs0, (const double4 *)a3, (const double4 *)a4,
                     (const double4 *)a5, n, derivs ? 1 : 0, partials);
  return launch_max_fold(partials, slots, out, s);
}

}  // namespace nbody
