// The fp64 snap pass's tile loop, ONE kernel template for snap_tile_f64_kernel<SOFT, kSnapIpt, false> (kernels_snap.hip: every body, lane by
// lane) and its list forms (kernels_hermite6_block.hip: the bodies an index list names, one or two per lane).  Both run the SAME per-pair
// operations in the same order over the same chunks, so a body's nine sums of a chunk are the same bits whichever kernel formed them,
// whatever the other bodies of the launch, its place among them or the bodies per lane.
#pragma once
#include "kernels.h"
#include "pk_common.h"

#pragma clang fp contract(off)

namespace nbody {
namespace {

constexpr int kSnapTile = 256;
constexpr int kSnapJb = 2;      // j-bodies per staged group

// 1 / sqrt(x) as every fp64 pair kernel here forms it: the v_rsq_f64 seed and one third-order step
__device__ __forceinline__ double snap_rsq_dev(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = fma(-(x * y), y, 1.0);
  const double q = e * fma(e, 0.375, 0.5);
  return fma(y, q, y);
}

__device__ __forceinline__ double4 load_ain(const double *__restrict__ ain, int stride, int i) {
  const double *r = ain + (size_t)i * stride;
  return make_double4(r[0], r[1], r[2], 0.0);
}

// A, J and S of IPT bodies per lane from all bodies of chunk blockIdx.y: local body il = blockIdx.x * (kBlock * IPT) + t + k * kBlock
// (the lanes past m repeat body m - 1 and write nothing) is body i_first + il — LIST: body list[il], the list ascending or not.  The
// bodies go through double-buffered LDS tiles as (x, y, z, G m), (vx, vy, vz, -) and (ax, ay, az, -): 48 KB.  ain holds body i's input
// acceleration at ain[i * ain_stride + 0 .. 2].
// Per pair, s2 = fma(dx, dx, fma(dy, dy, dz * dz [+ eps^2])), t = rsq(s2) — 0 where s2 == 0 and for j == the body itself by index —, then
//   t2 = t * t;  q = (G m * t) * t2;  dw = fma(dx, wx, fma(dy, wy, dz * wz));  k3 = -3 * (dw * t2);  u_a = fma(k3, d_a, w_a)
//   A_a = fma(q, d_a, A_a);  J_a = fma(q, u_a, J_a)                                        (the jerk kernel's, in its order)
//   ww = fma(wx, wx, fma(wy, wy, wz * wz));  db = fma(dx, bx, fma(dy, by, dz * bz));  al = dw * t2;  be = fma(al, al, (ww + db) * t2)
//   k6 = 2 * k3;  m3 = -3 * be;  g_a = fma(m3, d_a, fma(k6, u_a, b_a));  S_a = fma(q, g_a, S_a)
// — one chain per sum and chunk of probe_geometry, in body order.  A dropped pair has q = 0 and finite factors: it adds exactly 0 to
// all nine sums; so does the zero-mass padding (at rest on the origin, unaccelerated).  A chunk's row is nine doubles per local body:
// part[(c * m + il) * 9].
// <SOFT, kSnapIpt, false> is nbody_get_snap_f64's kernel, instruction for instruction what it was before the list forms existed
// (profiles/hermite6_block_isa_compare.txt).
template <bool SOFT, int IPT, bool LIST>
__global__ __launch_bounds__(kBlock) void snap_tile_f64_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                               const double *__restrict__ ain, int ain_stride,
                                                               double *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                               double gscale, double eps2, const int *__restrict__ list) {
  constexpr int JB = kSnapJb, TILE = kSnapTile;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  __shared__ double4 shp[2][TILE], shv[2][TILE], sha[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT], vxi[IPT], vyi[IPT], vzi[IPT], axi[IPT], ayi[IPT], azi[IPT];
  int self[IPT];
  double A[IPT][3], J[IPT][3], S[IPT][3];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    if (LIST) self[k] = list[min(ibase + t + k * kBlock, m - 1)];
    else      self[k] = i_first + min(ibase + t + k * kBlock, m - 1);
    const double4 p = posm[self[k]], v = vel[self[k]], a = load_ain(ain, ain_stride, self[k]);
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z; vxi[k] = v.x; vyi[k] = v.y; vzi[k] = v.z; axi[k] = a.x; ayi[k] = a.y; azi[k] = a.z;
#pragma unroll
    for (int q = 0; q < 3; ++q) { A[k][q] = 0.0; J[k][q] = 0.0; S[k][q] = 0.0; }
  }

  double4 rp, rv, ra;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) { rp = posm[j]; rv = vel[j]; ra = load_ain(ain, ain_stride, j); }
    else        { rp = make_double4(0.0, 0.0, 0.0, 0.0); rv = rp; ra = rp; }   // zero-mass padding, at rest, unaccelerated
  };
  auto store_tile = [&](int buf) {
    double4 q = rp; q.w *= gscale; shp[buf][t] = q; shv[buf][t] = rv; sha[buf][t] = ra;
  };

  if (ntiles > 0) { load_tile(0); store_tile(0); }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
    const int jt = j0 + tile * TILE;
#pragma unroll 2
    for (int jj = 0; jj < TILE; jj += JB) {
      double4 pj[JB], vj[JB], aj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) { pj[b] = shp[buf][jj + b]; vj[b] = shv[buf][jj + b]; aj[b] = sha[buf][jj + b]; }
      double dx[JB][IPT], dy[JB][IPT], dz[JB][IPT], s2[JB][IPT], ti[JB][IPT];
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          dx[b][k] = pj[b].x - xi[k]; dy[b][k] = pj[b].y - yi[k]; dz[b][k] = pj[b].z - zi[k];
          if (SOFT) s2[b][k] = fma(dz[b][k], dz[b][k], eps2);
          else      s2[b][k] = dz[b][k] * dz[b][k];
          s2[b][k] = fma(dy[b][k], dy[b][k], s2[b][k]);
          s2[b][k] = fma(dx[b][k], dx[b][k], s2[b][k]);
        }
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double r = snap_rsq_dev(s2[b][k]);
          ti[b][k] = (s2[b][k] > 0.0 && jt + jj + b != self[k]) ? r : 0.0;
        }
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double wx = vj[b].x - vxi[k], wy = vj[b].y - vyi[k], wz = vj[b].z - vzi[k];
          const double t2 = ti[b][k] * ti[b][k];
          const double q = (pj[b].w * ti[b][k]) * t2;
          double dw = dz[b][k] * wz;
          dw = fma(dy[b][k], wy, dw);
          dw = fma(dx[b][k], wx, dw);
          const double k3 = -3.0 * (dw * t2);
          const double ux = fma(k3, dx[b][k], wx), uy = fma(k3, dy[b][k], wy), uz = fma(k3, dz[b][k], wz);
          A[k][0] = fma(q, dx[b][k], A[k][0]); A[k][1] = fma(q, dy[b][k], A[k][1]); A[k][2] = fma(q, dz[b][k], A[k][2]);
          J[k][0] = fma(q, ux, J[k][0]); J[k][1] = fma(q, uy, J[k][1]); J[k][2] = fma(q, uz, J[k][2]);
          const double bx = aj[b].x - axi[k], by = aj[b].y - ayi[k], bz = aj[b].z - azi[k];
          const double ww = fma(wx, wx, fma(wy, wy, wz * wz));
          const double db = fma(dx[b][k], bx, fma(dy[b][k], by, dz[b][k] * bz));
          const double al = dw * t2;
          const double be = fma(al, al, (ww + db) * t2);
          const double k6 = 2.0 * k3;
          const double m3 = -3.0 * be;
          const double gx = fma(m3, dx[b][k], fma(k6, ux, bx)), gy = fma(m3, dy[b][k], fma(k6, uy, by)),
                       gz = fma(m3, dz[b][k], fma(k6, uz, bz));
          S[k][0] = fma(q, gx, S[k][0]); S[k][1] = fma(q, gy, S[k][1]); S[k][2] = fma(q, gz, S[k][2]);
        }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    if (il < m) {
      double *row = part + ((size_t)c * m + il) * 9;
#pragma unroll
      for (int q = 0; q < 3; ++q) { row[q] = A[k][q]; row[3 + q] = J[k][q]; row[6 + q] = S[k][q]; }
    }
  }
}

}  // namespace
}  // namespace nbody
