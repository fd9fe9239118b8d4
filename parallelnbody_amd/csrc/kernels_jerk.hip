// The jerk j = da/dt of the pair law at theta = 0 — and, as the tree holds no node velocities, at every other theta too
// (nbody_jerk_at, nbody_get_jerk, nbody_get_jerk_f64, nbody_jerk_time; build-defined: the reference computes none).  With d = x_j - x,
// w = v_j - v, s^2 = |d|^2 + eps^2:
//     a(x) = sum_j G m_j d / s^3        j(x, v) = sum_j G m_j [ w / s^3 - 3 (d . w) d / s^5 ]
//   probe_jerk_pk_kernel   <- fp32 state: the tile loop of point_tile.h with the bodies' velocities in a second pair of LDS tiles, the
//                             potential's distance term, six accumulators, no s^-5; SELF: the points are the bodies, j == i dropped by index
//   jerk_fold_kernel       <- the chunks' rows added in chunk order in fp64, rounded once
//   deriv_tile_f64_kernel  <- fp64 state, the bodies only: scalar, shaped like forces_tile_kernel<double> (kernels.hip): the <SOFT, 2, false, false, false> form of deriv_tile64.h's template
//   jerk_fold_f64_kernel   <- its chunks' rows added in chunk order
//   jerk_time_*_kernel     <- the largest |j_i|^2 / |a_i|^2 of the unrounded vectors and its body, reduced in a fixed order
#include "kernels.h"

#include <algorithm>

#include "../../include/nbody.h"
#include "deriv_tile64.h"
#include "point_tile.h"

namespace nbody {

namespace {

// The jerk's pair term for JB j-bodies against NP register pairs of points, stage by stage like tidal_group_pk (kernels_probe.hip), whose
// distance term it takes as it is (Z_SOFT / Z_CLAMP, the same rsq, GUARD by index): t = 1 / s, or 0 for a pair that adds nothing.
// Then, all of them the compiler's own operations on the rsq result,
//   g = G m_j * t;  g2 = g * t;  q = g2 * t = G m / s^3;  n_a = d_a * t (the unit vector: |n_a| <= 1)
//   k = n . w: nz * wz, then fused in y, then in x;  u_a = fma(-3 k, n_a, w_a) = w_a - 3 (d . w) d_a / s^2
//   A_a = fma(q, d_a, A_a);  J_a = fma(q, u_a, J_a)
// — one chain of fused multiply-adds per sum, in body order.  No s^-5 is formed: |u| <= 4 |w|, so a pair is finite wherever
// 4 G m |w| / s^3 is.  A pair with t == 0 adds q = 0 times finite values: nothing; so does the zero-mass padding (at rest on the origin).
struct Acc6pk {
  f2 ax = splat2(0.f), ay = splat2(0.f), az = splat2(0.f), jx = splat2(0.f), jy = splat2(0.f), jz = splat2(0.f);
};
template <int NP, int JB, int ZMODE, bool GUARD>
__device__ __forceinline__ void jerk_group_pk(const f2 (&xi)[NP], const f2 (&yi)[NP], const f2 (&zi)[NP], const f2 (&vxi)[NP],
                                              const f2 (&vyi)[NP], const f2 (&vzi)[NP], const float4 (&pj)[JB], const float4 (&vj)[JB],
                                              f2 zp2, f2 one2, f2 mthree2, Acc6pk (&a)[NP], int rel) {
  f2 dx[JB][NP], dy[JB][NP], dz[JB][NP], wx[JB][NP], wy[JB][NP], wz[JB][NP], w[JB][NP], nf[JB][NP], u[JB][NP];
#pragma unroll
  for (int b = 0; b < JB; ++b)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      dx[b][p] = splat2(pj[b].x) - xi[p]; dy[b][p] = splat2(pj[b].y) - yi[p]; dz[b][p] = splat2(pj[b].z) - zi[p];
      if (ZMODE == Z_SOFT) w[b][p] = fma2(dz[b][p], dz[b][p], zp2);
      else                 w[b][p] = dz[b][p] * dz[b][p];
      w[b][p] = fma2(dy[b][p], dy[b][p], w[b][p]);
      w[b][p] = fma2(dx[b][p], dx[b][p], w[b][p]);
    }
  if (ZMODE == Z_CLAMP) {
#pragma unroll
    for (int b = 0; b < JB; ++b)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(nf[b][p]) : "v"(w[b][p]), "v"(zp2), "v"(one2));
        w[b][p] = w[b][p] + nf[b][p];
      }
  }
#pragma unroll
  for (int b = 0; b < JB; ++b)
#pragma unroll
    for (int p = 0; p < NP; ++p) u[b][p] = f2{rsq_dev(w[b][p].x), rsq_dev(w[b][p].y)};
  // the velocity differences behind the roots: independent work in the slots after them
#pragma unroll
  for (int b = 0; b < JB; ++b)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      wx[b][p] = splat2(vj[b].x) - vxi[p]; wy[b][p] = splat2(vj[b].y) - vyi[p]; wz[b][p] = splat2(vj[b].z) - vzi[p];
    }
#pragma unroll
  for (int b = 0; b < JB; ++b)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      f2 t = u[b][p];
      if (ZMODE == Z_CLAMP) t = t - nf[b][p];
      if (GUARD) {
        t.x = (rel + b == (2 * p) * kBlock) ? 0.0f : t.x;
        t.y = (rel + b == (2 * p + 1) * kBlock) ? 0.0f : t.y;
      }
      const f2 g = splat2(pj[b].w) * t;
      const f2 g2 = g * t;
      const f2 q = g2 * t;
      const f2 nx = dx[b][p] * t, ny = dy[b][p] * t, nz = dz[b][p] * t;
      f2 k = nz * wz[b][p];
      k = fma2(ny, wy[b][p], k);
      k = fma2(nx, wx[b][p], k);
      const f2 k3 = k * mthree2;
      const f2 ux = fma2(k3, nx, wx[b][p]), uy = fma2(k3, ny, wy[b][p]), uz = fma2(k3, nz, wz[b][p]);
      a[p].ax = fma2(q, dx[b][p], a[p].ax); a[p].ay = fma2(q, dy[b][p], a[p].ay); a[p].az = fma2(q, dz[b][p], a[p].az);
      a[p].jx = fma2(q, ux, a[p].jx); a[p].jy = fma2(q, uy, a[p].jy); a[p].jz = fma2(q, uz, a[p].jz);
    }
}

// Two float4 per point in a chunk's row — (Ax, Ay, Az, 0), (Jx, Jy, Jz, 0).  SELF as in probe_pot_pk_kernel: `probe` is posm + i_first,
// `pvel` is vel + i_first, and the tiles that overlap the workgroup's own bodies run the guarded group; all others the plain one.
template <int NP, int TILE, int ZMODE, bool SELF>
__global__ __launch_bounds__(kBlock) void probe_jerk_pk_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ velj,
                                                               const float4 *__restrict__ probe, const float4 *__restrict__ pvel,
                                                               float4 *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                               float gscale, float zp) {
  constexpr int JB = point_group(NP);
  Acc6pk a[NP];
  f2 mthree2 = splat2(-3.0f);
  asm volatile("" : "+v"(mthree2));
  const int own0 = i_first + blockIdx.x * (kBlock * 2 * NP), own1 = own0 + kBlock * 2 * NP;
  point_tile_loop<NP, TILE, true>(posm, probe, n_total, m, j_chunk, gscale, zp,
                                  [&](int jt, const float4 *tile, const float4 *vtile, const f2 (&xi)[NP], const f2 (&yi)[NP],
                                      const f2 (&zi)[NP], const f2 (&vxi)[NP], const f2 (&vyi)[NP], const f2 (&vzi)[NP], f2 zp2, f2 one2) {
    if (SELF && jt < own1 && jt + TILE > own0) {               // (uniform over the workgroup)
      const int rel0 = jt - (own0 + (int)threadIdx.x);
      tile_groups_v<NP, TILE>(tile, vtile, [&](int jj, const float4 (&pj)[JB], const float4 (&vj)[JB]) {
        jerk_group_pk<NP, JB, ZMODE, true>(xi, yi, zi, vxi, vyi, vzi, pj, vj, zp2, one2, mthree2, a, rel0 + jj);
      });
    } else {
      tile_groups_v<NP, TILE>(tile, vtile, [&](int, const float4 (&pj)[JB], const float4 (&vj)[JB]) {
        jerk_group_pk<NP, JB, ZMODE, false>(xi, yi, zi, vxi, vyi, vzi, pj, vj, zp2, one2, mthree2, a, 0);
      });
    }
  }, velj, pvel);
  point_write_out<NP>(m, [&, part](int p, int h, size_t at) {
    part[2 * at] = make_float4(a[p].ax[h], a[p].ay[h], a[p].az[h], 0.f);
    part[2 * at + 1] = make_float4(a[p].jx[h], a[p].jy[h], a[p].jz[h], 0.f);
  });
}

// (a, j)[k] from the chunks' rows: the six sums added in chunk order in fp64 (no atomics: the same bits every time); aj64 gets the six
// doubles (ax, ay, az, jx, jy, jz) as they are, ajf the same rounded once.  Either may be null.
__global__ __launch_bounds__(kBlock) void jerk_fold_kernel(const float4 *__restrict__ part, int m, int j_split, double *__restrict__ aj64,
                                                           float *__restrict__ ajf) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const float4 r0 = part[2 * ((size_t)c * m + k)], r1 = part[2 * ((size_t)c * m + k) + 1];
    s[0] = s[0] + (double)r0.x; s[1] = s[1] + (double)r0.y; s[2] = s[2] + (double)r0.z;
    s[3] = s[3] + (double)r1.x; s[4] = s[4] + (double)r1.y; s[5] = s[5] + (double)r1.z;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if (aj64 != nullptr) aj64[(size_t)k * 6 + c] = s[c];
    if (ajf != nullptr) ajf[(size_t)k * 6 + c] = (float)s[c];
  }
}

// ---- fp64 state ----

constexpr int kJerk64Ipt = 2;   // bodies per lane

// (the pair kernel: deriv_tile64.h, shared with the snap, the active-set evaluations of kernels_hermite_block.hip and the points of kernels_points64.hip)

__global__ __launch_bounds__(kBlock) void jerk_fold_f64_kernel(const double *__restrict__ part, int m, int j_split, double *__restrict__ aj64,
                                                               float *__restrict__ ajf) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] = s[q] + row[q];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if (aj64 != nullptr) aj64[(size_t)k * 6 + c] = s[c];
    if (ajf != nullptr) ajf[(size_t)k * 6 + c] = (float)s[c];
  }
}

// nbody_jerk_time's reduction, shaped like tidal_time_*_kernel (kernels_probe.hip): a candidate is (k, body), k = |j|^2 / |a|^2 with
// 0 / 0 = 0, x / 0 = +inf for x > 0, and a value that is not finite counting as +inf.
__global__ __launch_bounds__(kBlock) void jerk_time_parts_kernel(const double *__restrict__ aj64, int n, double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ ValueAt red[kBlock / 64];
  ValueAt a{-1.0, 0x7fffffff};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const double *v = aj64 + (size_t)i * 6;
    const double ax = v[0], ay = v[1], az = v[2], jx = v[3], jy = v[4], jz = v[5];
    const double a2 = (ax * ax + ay * ay) + az * az, j2 = (jx * jx + jy * jy) + jz * jz;
    double k = (j2 == 0.0 && a2 == 0.0) ? 0.0 : j2 / a2;
    if (!(k <= 0x1.fffffffffffffp1023)) k = __builtin_inf();
    value_at_take<true>(a, k, i);
  }
  const ValueAt r = value_at_workgroup<true>(a, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = r.v; part[2 * blockIdx.x + 1] = (double)r.i; }
}

}  // namespace

hipError_t launch_jerk(const JerkLaunch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.vel || !L.part || (!L.aj64 && !L.ajf)) return hipErrorInvalidValue;
  const bool self = L.probe == nullptr;
  if (self ? L.m != L.n_total : !L.pvel) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;                              // eps == 0: the exact d == 0 rule, as the potential
  if (L.precision == NBODY_PREC_F64) {
    if (!self) return hipErrorInvalidValue;
    int j_split, j_chunk;
    probe_geometry(L.n_total, &j_split, &j_chunk);
    const size_t slab = probe_slab_points(L.n_total, 3);       // a row of six doubles: three float4
    for (size_t first = 0; first < (size_t)L.m; first += slab) {
      const int m = (int)std::min(slab, (size_t)L.m - first);
      const dim3 grid((m + kBlock * kJerk64Ipt - 1) / (kBlock * kJerk64Ipt), j_split);
      hipLaunchKernelGGL((soft ? deriv_tile_f64_kernel<true, kJerk64Ipt, false, false, false> : deriv_tile_f64_kernel<false, kJerk64Ipt, false, false, false>),
                         grid, dim3(kBlock), 0, s,
                         DerivArgs<false, false>{(const double4 *)L.posm, (const double4 *)L.vel, L.n_total, m, (int)first, j_chunk, L.G, L.eps2, nullptr},
                         (double *)L.part);
      hipLaunchKernelGGL(jerk_fold_f64_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)L.part, m, j_split,
                         L.aj64 ? L.aj64 + 6 * first : nullptr, L.ajf ? L.ajf + 6 * first : nullptr);
    }
    return hipGetLastError();
  }
  for_point_slabs(L.n_total, L.m, 2, [&](auto np, size_t first, int m, dim3 grid, int j_split, int j_chunk) {
    constexpr int NP = decltype(np)::value;
    const auto kernel = self ? (soft ? probe_jerk_pk_kernel<NP, kJerkTile, Z_SOFT, true> : probe_jerk_pk_kernel<NP, kJerkTile, Z_CLAMP, true>)
                             : (soft ? probe_jerk_pk_kernel<NP, kJerkTile, Z_SOFT, false> : probe_jerk_pk_kernel<NP, kJerkTile, Z_CLAMP, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const float4 *)L.posm, (const float4 *)L.vel,
                       (const float4 *)(self ? L.posm : L.probe) + first, (const float4 *)(self ? L.vel : L.pvel) + first, (float4 *)L.part,
                       L.n_total, m, self ? (int)first : 0, j_chunk, (float)L.G, soft ? (float)L.eps2 : -0x1p126f);
    hipLaunchKernelGGL(jerk_fold_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const float4 *)L.part, m, j_split,
                       L.aj64 ? L.aj64 + 6 * first : nullptr, L.ajf ? L.ajf + 6 * first : nullptr);
  });
  return hipGetLastError();
}

// jerk_fold_f64_kernel on its own, for the rows another file's kernel wrote in this layout (kernels_points64.hip: the point form)
hipError_t launch_jerk_fold_f64(const void *part, int m, int j_split, double *aj64, hipStream_t s) {
  if (m <= 0 || j_split <= 0 || !part || !aj64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jerk_fold_f64_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)part, m, j_split, aj64,
                     (float *)nullptr);
  return hipGetLastError();
}

hipError_t launch_jerk_time(const double *aj64, int n, double *partials, double *out, hipStream_t s) {
  if (n <= 0 || !aj64 || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(jerk_time_parts_kernel, dim3(slots), dim3(kBlock), 0, s, aj64, n, partials);
  return launch_max_fold(partials, slots, out, s);
}

}  // namespace nbody
