// The theta = 0 point queries: the bodies' field and potential at points (nbody_field_at and the tracers of nbody_set_tracers;
// nbody_potential_at, nbody_get_potentials, nbody_energy_fast — the potential is build-defined: the reference computes none — and the
// tidal tensor, build-defined as well).  One tile loop (point_tile.h), three pair terms:
//   probe_tile_pk_kernel   <- the pair law OctreeSearch.h:101-104 of a massless point against every body, i.e. the loop
//                             OctreeSearch.cpp:83-86 with the i side taken from another array
//   probe_fold_kernel      <- the chunks' partial rows added in chunk order and, for tracers, OctreeSearch.cpp:29-30 (v += dt*a; x += dt*v)
//   probe_pot_pk_kernel    <- phi(x) = -sum_j G m_j / sqrt(|x - x_j|^2 + eps^2): one accumulator instead of three and no cube; SELF: the
//                             points are the bodies themselves, j == i dropped by index
//   pot_fold_kernel        <- the chunks' partial rows added in chunk order in fp64, negated, rounded once
//   energy_fast_*_kernel   <- 1/2 m v^2 and 1/2 m phi from the unrounded potentials, reduced in a fixed order
//   probe_tidal_pk_kernel  <- T_ab(x) = sum_j G m_j [3 d_a d_b / s^5 - delta_ab / s^3] (nbody_tidal_at, nbody_get_tidal, nbody_tidal_time):
//                             seven accumulators, the potential's distance term, no s^-5; SELF as the potential's
//   tidal_fold_kernel      <- the chunks' rows added in chunk order in fp64, T_aa = S_aa - Q there, rounded once
//   tidal_time_*_kernel    <- the largest squared Frobenius norm of the unrounded tensors and its body, reduced in a fixed order
// The theta > 0 counterparts — the walk of the last tree from a point — are bh_probe_walk_kernel, bh_pot_walk_kernel and
// bh_tidal_walk_kernel (kernels_bh_pot.hip).
#include "kernels.h"

#include <algorithm>

#include "../../include/nbody.h"
#include "point_tile.h"
#include "tracer_update.h"

namespace nbody {

namespace {

constexpr int kProbeTile = 256;

// The field: a point may sit on a body anywhere, so every tile runs the guarded law (there is no "own range" and no bare pass); the
// zero-mass padding of ragged tiles is kept out of the sum by every ZMODE here.  A point's sum over a chunk is one chain of fused
// multiply-adds in body order whatever NP is and wherever the point stands in the array.
template <int NP, int TILE, int ZMODE>
__global__ __launch_bounds__(kBlock) void probe_tile_pk_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ probe,
                                                               float4 *__restrict__ part, int n_total, int m, int j_chunk,
                                                               float gscale, float zp, unsigned long long *__restrict__ clk) {
  constexpr int JB = point_group(NP);
  const ClockStamp stamp = clock_begin(clk);
  Acc3pk<false> a[NP];
  point_tile_loop<NP, TILE>(posm, probe, n_total, m, j_chunk, gscale, zp,
                            [&](int, const float4 *tile, const f2 (&xi)[NP], const f2 (&yi)[NP], const f2 (&zi)[NP], f2 zp2, f2 one2) {
    tile_groups<NP, TILE>(tile, [&](int, const float4 (&pj)[JB]) {
      pair_group_pk<NP, JB, ZMODE, false, false>(xi, yi, zi, pj, zp2, one2, a);
    });
  });
  point_write_out<NP>(m, [&, part](int p, int h, size_t at) { part[at] = make_float4(a[p].x[h], a[p].y[h], a[p].z[h], 0.f); });
  clock_end(clk, stamp);
}

// acc[k] = sum_c part[c][k] in chunk order (no atomics: the same bits every time).  integrate != 0: the point is a tracer and
// gets the bodies' own kick-drift, multiply and add kept apart (OctreeSearch.cpp:29-30).
__global__ __launch_bounds__(kBlock) void probe_fold_kernel(const float4 *__restrict__ part, int m, int j_split,
                                                            float4 *__restrict__ acc, float4 *__restrict__ pos,
                                                            float4 *__restrict__ vel, float dt, int integrate) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll 8
  for (int c = 0; c < j_split; ++c) {
    const float4 p = part[(size_t)c * m + k];
    ax = ax + p.x; ay = ay + p.y; az = az + p.z;
  }
  acc[k] = make_float4(ax, ay, az, 0.f);
  if (integrate) {
    float4 v = vel[k], x = pos[k];
    tracer_kick_drift(dt, ax, ay, az, v, x);
    vel[k] = v;
    pos[k] = x;
  }
}

// The potential's pair term for JB j-bodies against NP register pairs of points, stage by stage like pair_group_pk (pk_common.h):
//   r2 as there (dz^2 [+ eps^2], dy, dx fused in that order), then
//   Z_SOFT  : t = rsq(r2 + eps^2)                      — a point on a body feels that body's G m / eps
//   Z_CLAMP : t = rsq(r2 + nf) - nf, nf = clamp01(1 - r2 * 2^126): exactly rsq(r2) for every normal r2 > 0, exactly 1 - 1 = 0 for
//             r2 == 0 — a pair at distance 0 adds nothing (a potential has no zero difference vector to do that for it)
//   a[p] = fma(G m_j, t, a[p])                         — one chain of fused multiply-adds per point, in body order.
// GUARD (the tiles of a SELF launch that hold the workgroup's own bodies): the pair j == i adds nothing whatever its distance term is —
// by index: `rel` = (the index of pj[0]) - (the index of the lane's first point); the lane's points stand (2 p + h) * kBlock further on.
// Every operation on a v_rsq_f32 result is the compiler's own (it pads the transcendental hazard for its own instructions only).
template <int NP, int JB, int ZMODE, bool GUARD>
__device__ __forceinline__ void pot_group_pk(const f2 (&xi)[NP], const f2 (&yi)[NP], const f2 (&zi)[NP], const float4 (&pj)[JB], f2 zp2,
                                             f2 one2, f2 (&a)[NP], int rel) {
  f2 w[JB][NP], nf[JB][NP], u[JB][NP];
#pragma unroll
  for (int b = 0; b < JB; ++b)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const f2 dx = splat2(pj[b].x) - xi[p], dy = splat2(pj[b].y) - yi[p], dz = splat2(pj[b].z) - zi[p];
      if (ZMODE == Z_SOFT) w[b][p] = fma2(dz, dz, zp2);
      else                 w[b][p] = dz * dz;
      w[b][p] = fma2(dy, dy, w[b][p]);
      w[b][p] = fma2(dx, dx, w[b][p]);
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
      a[p] = fma2(splat2(pj[b].w), t, a[p]);
    }
}

// The potential: one float per point in a chunk's row; the padding adds 0 * a finite term: nothing.  SELF: `probe` is posm + i_first, the
// points are bodies i_first .. i_first + m, and the tiles that overlap the workgroup's own bodies run the guarded group; all others the
// plain one.
template <int NP, int TILE, int ZMODE, bool SELF>
__global__ __launch_bounds__(kBlock) void probe_pot_pk_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ probe,
                                                              float *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                              float gscale, float zp, unsigned long long *__restrict__ clk) {
  constexpr int JB = point_group(NP);
  const ClockStamp stamp = clock_begin(clk);
  f2 a[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) a[p] = splat2(0.f);
  // the workgroup's own bodies, as indices of posm (SELF)
  const int own0 = i_first + blockIdx.x * (kBlock * 2 * NP), own1 = own0 + kBlock * 2 * NP;
  point_tile_loop<NP, TILE>(posm, probe, n_total, m, j_chunk, gscale, zp,
                            [&](int jt, const float4 *tile, const f2 (&xi)[NP], const f2 (&yi)[NP], const f2 (&zi)[NP], f2 zp2, f2 one2) {
    if (SELF && jt < own1 && jt + TILE > own0) {               // (uniform over the workgroup)
      const int rel0 = jt - (own0 + (int)threadIdx.x);
      tile_groups<NP, TILE>(tile, [&](int jj, const float4 (&pj)[JB]) {
        pot_group_pk<NP, JB, ZMODE, true>(xi, yi, zi, pj, zp2, one2, a, rel0 + jj);
      });
    } else {
      tile_groups<NP, TILE>(tile, [&](int, const float4 (&pj)[JB]) {
        pot_group_pk<NP, JB, ZMODE, false>(xi, yi, zi, pj, zp2, one2, a, 0);
      });
    }
  });
  point_write_out<NP>(m, [&, part](int p, int h, size_t at) { part[at] = a[p][h]; });
  clock_end(clk, stamp);
}

// phi[k] = -(sum_c part[c][k]): the rows added in chunk order in fp64 (no atomics: the same bits every time; a same-sign sum whose
// error stays that of one chunk), negated; phi64 gets it as it is (nbody_energy_fast), phif rounded once (the getters).  Either may be null.
__global__ __launch_bounds__(kBlock) void pot_fold_kernel(const float *__restrict__ part, int m, int j_split, double *__restrict__ phi64,
                                                          float *__restrict__ phif) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < j_split; ++c) s = s + (double)part[(size_t)c * m + k];
  const double phi = -s;
  if (phi64 != nullptr) phi64[k] = phi;
  if (phif != nullptr) phif[k] = (float)phi;
}

// nbody_energy_fast's reduction, two launches, no atomics, the same bits every run.  First: workgroup g adds 1/2 m_i v_i^2 and
// 1/2 m_i phi_i of bodies g * kBlock + t + q * (gridDim.x * kBlock), q = 0, 1, ... in that order per lane, then the fixed shuffle tree
// and the four waves in order, into part[2 g], part[2 g + 1].  Second (energy_fast_fold_kernel): the workgroups' pairs the same way.
__global__ __launch_bounds__(kBlock) void energy_fast_parts_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ vel,
                                                                   const double *__restrict__ phi64, int n, double *__restrict__ part) {
  __shared__ double red[2][kBlock / 64];
  const int t = threadIdx.x;
  double k = 0.0, p = 0.0;
  for (int i = blockIdx.x * kBlock + t; i < n; i += gridDim.x * kBlock) {
    const double mi = (double)posm[i].w;
    const float4 v = vel[i];
    const double vx = v.x, vy = v.y, vz = v.z;
    k += 0.5 * mi * (vx * vx + vy * vy + vz * vz);
    p += 0.5 * mi * phi64[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { k += __shfl_xor(k, off, 64); p += __shfl_xor(p, off, 64); }
  if ((t & 63) == 0) { red[0][t >> 6] = k; red[1][t >> 6] = p; }
  __syncthreads();
  if (t == 0) {
    double ks = 0, ps = 0;
    for (int w = 0; w < kBlock / 64; ++w) { ks += red[0][w]; ps += red[1][w]; }
    part[2 * blockIdx.x] = ks;
    part[2 * blockIdx.x + 1] = ps;
  }
}
__global__ __launch_bounds__(kBlock) void energy_fast_fold_kernel(const double *__restrict__ part, int slots, double *__restrict__ out) {
  __shared__ double red[2][kBlock / 64];
  const int t = threadIdx.x;
  double k = 0.0, p = 0.0;
  for (int q = t; q < slots; q += kBlock) { k += part[2 * q]; p += part[2 * q + 1]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { k += __shfl_xor(k, off, 64); p += __shfl_xor(p, off, 64); }
  if ((t & 63) == 0) { red[0][t >> 6] = k; red[1][t >> 6] = p; }
  __syncthreads();
  if (t == 0) {
    double ks = 0, ps = 0;
    for (int w = 0; w < kBlock / 64; ++w) { ks += red[0][w]; ps += red[1][w]; }
    out[0] = ks;
    out[1] = ps;
  }
}

// The tidal tensor's pair term, stage by stage like pot_group_pk, whose distance term it takes as it is (Z_SOFT / Z_CLAMP, the same rsq,
// GUARD by index): t = 1 / s, or 0 for a pair that adds nothing.  Then, all of them the compiler's own operations,
//   g = G m_j * t;  g2 = g * t;  n_a = d_a * t (the unit vector: |n_a| <= 1);  h = (3 g2) * t = 3 G m / s^3;  h_a = h * n_a
//   S_ab = fma(h_a, n_b, S_ab) for the six pairs a <= b;  Q = fma(g2, t, Q)
// — one chain of fused multiply-adds per sum, in body order.  No s^-5 is formed: every value on the way is at most 3 G m / s^3 in
// magnitude, so a pair is finite wherever that is.  T_aa = S_aa - Q is the fold's.
struct Acc7pk {
  f2 xx = splat2(0.f), yy = splat2(0.f), zz = splat2(0.f), xy = splat2(0.f), xz = splat2(0.f), yz = splat2(0.f), q = splat2(0.f);
};
template <int NP, int JB, int ZMODE, bool GUARD>
__device__ __forceinline__ void tidal_group_pk(const f2 (&xi)[NP], const f2 (&yi)[NP], const f2 (&zi)[NP], const float4 (&pj)[JB], f2 zp2,
                                               f2 one2, f2 three2, Acc7pk (&a)[NP], int rel) {
  f2 dx[JB][NP], dy[JB][NP], dz[JB][NP], w[JB][NP], nf[JB][NP], u[JB][NP];
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
      const f2 nx = dx[b][p] * t, ny = dy[b][p] * t, nz = dz[b][p] * t;
      const f2 h = (g2 * three2) * t;
      const f2 hx = h * nx, hy = h * ny, hz = h * nz;
      a[p].xx = fma2(hx, nx, a[p].xx); a[p].xy = fma2(hx, ny, a[p].xy); a[p].xz = fma2(hx, nz, a[p].xz);
      a[p].yy = fma2(hy, ny, a[p].yy); a[p].yz = fma2(hy, nz, a[p].yz);
      a[p].zz = fma2(hz, nz, a[p].zz);
      a[p].q = fma2(g2, t, a[p].q);
    }
}

// The tidal tensor: two float4 per point in a chunk's row — (Sxx, Syy, Szz, Sxy), (Sxz, Syz, Q, 0); the padding adds 0 * finite terms.
// SELF as in probe_pot_pk_kernel.
template <int NP, int TILE, int ZMODE, bool SELF>
__global__ __launch_bounds__(kBlock) void probe_tidal_pk_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ probe,
                                                                float4 *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                                float gscale, float zp, unsigned long long *__restrict__ clk) {
  constexpr int JB = point_group(NP);
  const ClockStamp stamp = clock_begin(clk);
  Acc7pk a[NP];
  f2 three2 = splat2(3.0f);
  asm volatile("" : "+v"(three2));
  const int own0 = i_first + blockIdx.x * (kBlock * 2 * NP), own1 = own0 + kBlock * 2 * NP;
  point_tile_loop<NP, TILE>(posm, probe, n_total, m, j_chunk, gscale, zp,
                            [&](int jt, const float4 *tile, const f2 (&xi)[NP], const f2 (&yi)[NP], const f2 (&zi)[NP], f2 zp2, f2 one2) {
    if (SELF && jt < own1 && jt + TILE > own0) {               // (uniform over the workgroup)
      const int rel0 = jt - (own0 + (int)threadIdx.x);
      tile_groups<NP, TILE>(tile, [&](int jj, const float4 (&pj)[JB]) {
        tidal_group_pk<NP, JB, ZMODE, true>(xi, yi, zi, pj, zp2, one2, three2, a, rel0 + jj);
      });
    } else {
      tile_groups<NP, TILE>(tile, [&](int, const float4 (&pj)[JB]) {
        tidal_group_pk<NP, JB, ZMODE, false>(xi, yi, zi, pj, zp2, one2, three2, a, 0);
      });
    }
  });
  point_write_out<NP>(m, [&, part](int p, int h, size_t at) {
    part[2 * at] = make_float4(a[p].xx[h], a[p].yy[h], a[p].zz[h], a[p].xy[h]);
    part[2 * at + 1] = make_float4(a[p].xz[h], a[p].yz[h], a[p].q[h], 0.f);
  });
  clock_end(clk, stamp);
}

// T[k] from the chunks' rows: the seven sums added in chunk order in fp64 (no atomics: the same bits every time), T_aa = S_aa - Q in fp64;
// t64 gets the six doubles as they are (nbody_tidal_time), tf rounded once (the getters).  Either may be null.
__global__ __launch_bounds__(kBlock) void tidal_fold_kernel(const float4 *__restrict__ part, int m, int j_split, double *__restrict__ t64,
                                                            float *__restrict__ tf) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double xx = 0.0, yy = 0.0, zz = 0.0, xy = 0.0, xz = 0.0, yz = 0.0, q = 0.0;
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const float4 r0 = part[2 * ((size_t)c * m + k)], r1 = part[2 * ((size_t)c * m + k) + 1];
    xx = xx + (double)r0.x; yy = yy + (double)r0.y; zz = zz + (double)r0.z; xy = xy + (double)r0.w;
    xz = xz + (double)r1.x; yz = yz + (double)r1.y; q = q + (double)r1.z;
  }
  const double t[6] = {xx - q, yy - q, zz - q, xy, xz, yz};
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if (t64 != nullptr) t64[(size_t)k * 6 + c] = t[c];
    if (tf != nullptr) tf[(size_t)k * 6 + c] = (float)t[c];
  }
}

// nbody_tidal_time's reduction, shaped like energy_fast_*_kernel: two launches, no atomics, the same bits and the same body every run.
// A candidate is (n2, body) (pk_common.h: value_at_*); a value that is not finite counts as +inf.
__global__ __launch_bounds__(kBlock) void tidal_time_parts_kernel(const double *__restrict__ t64, int n, double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ ValueAt red[kBlock / 64];
  ValueAt a{-1.0, 0x7fffffff};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const double *t = t64 + (size_t)i * 6;
    const double xx = t[0], yy = t[1], zz = t[2], xy = t[3], xz = t[4], yz = t[5];
    double n2 = (xx * xx + yy * yy) + zz * zz + 2.0 * ((xy * xy + xz * xz) + yz * yz);
    if (!(n2 <= 0x1.fffffffffffffp1023)) n2 = __builtin_inf();
    value_at_take<true>(a, n2, i);
  }
  const ValueAt r = value_at_workgroup<true>(a, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = r.v; part[2 * blockIdx.x + 1] = (double)r.i; }
}
// the one fold of every (value, body) maximum: the workgroups' pairs in a fixed order (launch_max_fold)
__global__ __launch_bounds__(kBlock) void max_fold_kernel(const double *__restrict__ part, int slots, double *__restrict__ out) {
  __shared__ ValueAt red[kBlock / 64];
  ValueAt a{-1.0, 0x7fffffff};
  for (int q = threadIdx.x; q < slots; q += kBlock) value_at_take<true>(a, part[2 * q], (int)part[2 * q + 1]);
  const ValueAt r = value_at_workgroup<true>(a, red);
  if (threadIdx.x == 0) { out[0] = r.v; out[1] = (double)r.i; }
}

}  // namespace

// The j range is cut by the number of bodies ALONE — chunks of whole tiles, at most 128 of them — so that a point's bits depend
// neither on the other points of the call nor on their number, nor on the part the library runs on.  (128 chunks: a query of a
// hundred points against 2^20 bodies is 128 workgroups, and a partial row costs 2 KB per point.)
void probe_geometry(int n_total, int *j_split, int *j_chunk) {
  int chunk = (n_total + 127) / 128;
  chunk = std::max(1, (chunk + kProbeTile - 1) / kProbeTile) * kProbeTile;
  *j_chunk = chunk;
  *j_split = (n_total + chunk - 1) / chunk;
}

size_t probe_slab_points(int n_total, int width) {
  int js, jc;
  probe_geometry(n_total, &js, &jc);
  const size_t pts = kProbePartBytes / ((size_t)js * sizeof(float4) * (size_t)width);
  return std::max<size_t>(1024, pts / 1024 * 1024);
}

hipError_t launch_probe(const ProbeLaunch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.probe || !L.part || !L.acc) return hipErrorInvalidValue;
  const int integrate = L.dt > 0.0f ? 1 : 0;
  if (integrate && (!L.vel || !L.pos_out)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  for_point_slabs(L.n_total, L.m, 1, [&](auto np, size_t first, int m, dim3 grid, int j_split, int j_chunk) {
    constexpr int NP = decltype(np)::value;
    hipLaunchKernelGGL((soft ? probe_tile_pk_kernel<NP, kProbeTile, Z_SOFT> : probe_tile_pk_kernel<NP, kProbeTile, Z_CLAMP>), grid,
                       dim3(kBlock), 0, s, (const float4 *)L.posm, (const float4 *)L.probe + first, (float4 *)L.part, L.n_total, m, j_chunk,
                       (float)L.G, soft ? (float)L.eps2 : -0x1p126f, (unsigned long long *)L.clk);
    hipLaunchKernelGGL(probe_fold_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const float4 *)L.part, m, j_split,
                       (float4 *)L.acc + first, integrate ? (float4 *)L.pos_out + first : nullptr,
                       integrate ? (float4 *)L.vel + first : nullptr, L.dt, integrate);
  });
  return hipGetLastError();
}

hipError_t launch_pot(const PotLaunch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.part || (!L.phi64 && !L.phif)) return hipErrorInvalidValue;
  const bool self = L.probe == nullptr;
  if (self && L.m != L.n_total) return hipErrorInvalidValue;
  // eps == 0: the exact d == 0 rule whatever the context's zero_mode is (an eps floor would add G m / 1e-10 for a point on a body)
  const bool soft = L.eps2 > 0.0;
  for_point_slabs(L.n_total, L.m, 1, [&](auto np, size_t first, int m, dim3 grid, int j_split, int j_chunk) {
    constexpr int NP = decltype(np)::value;
    const auto kernel = self ? (soft ? probe_pot_pk_kernel<NP, kProbeTile, Z_SOFT, true> : probe_pot_pk_kernel<NP, kProbeTile, Z_CLAMP, true>)
                             : (soft ? probe_pot_pk_kernel<NP, kProbeTile, Z_SOFT, false> : probe_pot_pk_kernel<NP, kProbeTile, Z_CLAMP, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const float4 *)L.posm, (const float4 *)(self ? L.posm : L.probe) + first,
                       (float *)L.part, L.n_total, m, self ? (int)first : 0, j_chunk, (float)L.G, soft ? (float)L.eps2 : -0x1p126f,
                       (unsigned long long *)L.clk);
    hipLaunchKernelGGL(pot_fold_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const float *)L.part, m, j_split,
                       L.phi64 ? (double *)L.phi64 + first : nullptr, L.phif ? (float *)L.phif + first : nullptr);
  });
  return hipGetLastError();
}

hipError_t launch_tidal(const TidalLaunch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.part || (!L.t64 && !L.tf)) return hipErrorInvalidValue;
  const bool self = L.probe == nullptr;
  if (self && L.m != L.n_total) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;                              // eps == 0: the exact d == 0 rule, as the potential
  for_point_slabs(L.n_total, L.m, 2, [&](auto np, size_t first, int m, dim3 grid, int j_split, int j_chunk) {
    constexpr int NP = decltype(np)::value;
    const auto kernel = self ? (soft ? probe_tidal_pk_kernel<NP, kProbeTile, Z_SOFT, true> : probe_tidal_pk_kernel<NP, kProbeTile, Z_CLAMP, true>)
                             : (soft ? probe_tidal_pk_kernel<NP, kProbeTile, Z_SOFT, false> : probe_tidal_pk_kernel<NP, kProbeTile, Z_CLAMP, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const float4 *)L.posm, (const float4 *)(self ? L.posm : L.probe) + first,
                       (float4 *)L.part, L.n_total, m, self ? (int)first : 0, j_chunk, (float)L.G, soft ? (float)L.eps2 : -0x1p126f,
                       (unsigned long long *)L.clk);
    hipLaunchKernelGGL(tidal_fold_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const float4 *)L.part, m, j_split,
                       L.t64 ? L.t64 + 6 * first : nullptr, L.tf ? L.tf + 6 * first : nullptr);
  });
  return hipGetLastError();
}

hipError_t launch_tidal_time(const double *t64, int n, double *partials, double *out, hipStream_t s) {
  if (n <= 0 || !t64 || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(tidal_time_parts_kernel, dim3(slots), dim3(kBlock), 0, s, t64, n, partials);
  return launch_max_fold(partials, slots, out, s);
}

hipError_t launch_max_fold(const double *partials, int slots, double *out, hipStream_t s) {
  if (slots <= 0 || !partials || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(max_fold_kernel, dim3(1), dim3(kBlock), 0, s, partials, slots, out);
  return hipGetLastError();
}

int energy_fast_slots(int n) { return std::max(1, std::min(kEnergyFastSlots, (n + kBlock - 1) / kBlock)); }

hipError_t launch_energy_fast(const void *posm, const void *vel, const double *phi64, int n, double *partials, double *out, hipStream_t s) {
  if (n <= 0 || !posm || !vel || !phi64 || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(energy_fast_parts_kernel, dim3(slots), dim3(kBlock), 0, s, (const float4 *)posm, (const float4 *)vel, phi64, n, partials);
  hipLaunchKernelGGL(energy_fast_fold_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)partials, slots, out);
  return hipGetLastError();
}

}  // namespace nbody
