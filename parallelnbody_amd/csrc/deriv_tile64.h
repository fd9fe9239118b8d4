// The fp64 jerk and snap passes' tile loop: ONE kernel template, deriv_tile_f64_kernel<SOFT, IPT, LIST, POINTS, SNAP>, for a, j (and the
// snap s) of rows held in registers against all bodies of one chunk.  Every form runs the SAME per-pair operations in the same order
// over the same chunks, so a row's sums of a chunk are the same bits whichever form made them, whatever the other rows of the launch,
// its place among them or the rows per lane: a body asked about as a point gets nbody_get_jerk_f64's bits, an active body of a block
// step the full pass's, and the a and j of a snap pass are the jerk pass's.
//   <SOFT, 2, false, false, false>         nbody_get_jerk_f64 (kernels_jerk.hip): lane t of workgroup g holds bodies i_first + g * 512 + t (+ 256)
//   <SOFT, kSnapIpt, false, false, true>   nbody_get_snap_f64 (kernels_snap.hip)
//   <., ., true, false, .>                 the active bodies of a Hermite block step (kernels_hermite_block.hip), one or two per lane
//   <., ., false, true, .>                 caller points and shared-step tracers (kernels_points64.hip)
//   <., ., true, true, .>                  the active tracers of a block step (kernels_points64.hip)
// Rows.  Local row il = blockIdx.x * (kBlock * IPT) + t + k * kBlock; the lanes past m repeat row m - 1 and write nothing.  Bodies: row il
// is body i_first + il of (posm, vel, ain) — LIST: body list[il], the list ascending or not.  POINTS: row il is row il of the caller's
// (ppos, pvel, pain) — LIST: row list[il].  ain holds body j's input acceleration at ain[j * ain_stride + 0 .. 2], pain a point's the same way.
// Bodies go through double-buffered LDS tiles of kJerkTile as (x, y, z, G m), (vx, vy, vz, -) and, SNAP, (ax, ay, az, -): 32 / 48 KB; the
// last tile is padded with bodies of zero mass, at rest on the origin, unaccelerated.
// Per pair, with d = x_j - x_i, w = v_j - v_i, b = acc_j - acc_i:  s2 = fma(dx, dx, fma(dy, dy, dz * dz [+ eps^2])), t = rsq_dev(s2) — 0
// where s2 == 0 and, bodies, for j == the body itself BY INDEX; no pair of a point is dropped by index —, then
//   t2 = t * t;  q = (G m * t) * t2;  dw = fma(dx, wx, fma(dy, wy, dz * wz));  k3 = -3 * (dw * t2);  u_a = fma(k3, d_a, w_a)
//   A_a = fma(q, d_a, A_a);  J_a = fma(q, u_a, J_a)
//   SNAP:  ww = fma(wx, wx, fma(wy, wy, wz * wz));  db = fma(dx, bx, fma(dy, by, dz * bz));  al = dw * t2;  be = fma(al, al, (ww + db) * t2)
//          k6 = 2 * k3;  m3 = -3 * be;  g_a = fma(m3, d_a, fma(k6, u_a, b_a));  S_a = fma(q, g_a, S_a)
// — one chain per sum and chunk of probe_geometry, in body order.  A dropped pair has q = 0 and finite factors: it adds exactly 0 to every
// sum; so does the padding.  d == 0: with eps == 0 a point exactly on a body (or two coincident bodies) drops that pair from every sum;
// with eps > 0 that pair adds G m w / eps^3 to the jerk, G m b / eps^3 to the snap and nothing to a (a body's own pair has w = b = 0).
// A chunk's row is W = 6 (A, J) or 9 (A, J, S) doubles per local row: part[(c * m + il) * W], folded from 0.0 in chunk order by the fold
// kernels of kernels_jerk.hip and kernels_snap.hip or by the block correctors.  No scratch, no atomics.
// It is one __global__ template, not four kernels around a shared __device__ body: inlined into <., 2, ., false, true> such a body cost
// 58 VGPRs.  What a form reads is its DerivArgs<POINTS, SNAP>; the rows it writes are an argument of their own (as a member
// of the struct the row address of the one-row jerk forms took two more moves).
#pragma once
#include "kernels.h"
#include "pk_common.h"

namespace nbody {
namespace {

constexpr int kJerkTile = 256;
constexpr int kJerk64Jb = 2;    // j-bodies per staged group

__device__ __forceinline__ double4 load_ain(const double *__restrict__ ain, int stride, int i) {
  const double *r = ain + (size_t)i * stride;
  return make_double4(r[0], r[1], r[2], 0.0);
}

// What each (POINTS, SNAP) form reads.
template <bool POINTS, bool SNAP> struct DerivArgs;
template <> struct DerivArgs<false, false> {
  const double4 *posm, *vel;
  int n_total, m, i_first, j_chunk;
  double gscale, eps2;
  const int *list;
};
template <> struct DerivArgs<false, true> {
  const double4 *posm, *vel;
  const double *ain;
  int ain_stride;
  int n_total, m, i_first, j_chunk;
  double gscale, eps2;
  const int *list;
};
template <> struct DerivArgs<true, false> {
  const double4 *posm, *vel, *ppos, *pvel;
  int n_total, m, j_chunk;
  double gscale, eps2;
  const int *list;
};
template <> struct DerivArgs<true, true> {
  const double4 *posm, *vel;
  const double *ain;
  int ain_stride;
  const double4 *ppos, *pvel;
  const double *pain;
  int pain_stride;
  int n_total, m, j_chunk;
  double gscale, eps2;
  const int *list;
};

template <bool SOFT, int IPT, bool LIST, bool POINTS, bool SNAP>
__global__ __launch_bounds__(kBlock) void deriv_tile_f64_kernel(const DerivArgs<POINTS, SNAP> a, double *__restrict__ part) {
#pragma clang fp contract(off)
  constexpr int JB = kJerk64Jb, TILE = kJerkTile, W = SNAP ? 9 : 6;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  __shared__ double4 shp[2][TILE], shv[2][TILE];
  __shared__ double4 sha[SNAP ? 2 : 1][SNAP ? TILE : 1];   // (never referenced without SNAP: no LDS then)

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * a.j_chunk;
  const int j1 = min(j0 + a.j_chunk, a.n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT], vxi[IPT], vyi[IPT], vzi[IPT], axi[IPT], ayi[IPT], azi[IPT];
  int self[IPT];                                   // the row's index in the i-side arrays; bodies: the j it is
  double A[IPT][3], J[IPT][3], S[IPT][3];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = min(ibase + t + k * kBlock, a.m - 1);
    double4 p, v;
    if constexpr (POINTS) {
      self[k] = LIST ? a.list[il] : il;
      p = a.ppos[self[k]]; v = a.pvel[self[k]];
    } else {
      self[k] = LIST ? a.list[il] : a.i_first + il;
      p = a.posm[self[k]]; v = a.vel[self[k]];
    }
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z; vxi[k] = v.x; vyi[k] = v.y; vzi[k] = v.z;
    if constexpr (SNAP) {
      double4 b;
      if constexpr (POINTS) b = load_ain(a.pain, a.pain_stride, self[k]);
      else                  b = load_ain(a.ain, a.ain_stride, self[k]);
      axi[k] = b.x; ayi[k] = b.y; azi[k] = b.z;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      A[k][q] = 0.0; J[k][q] = 0.0;
      if constexpr (SNAP) S[k][q] = 0.0;
    }
  }

  double4 rp, rv, ra;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) {
      rp = a.posm[j]; rv = a.vel[j];
      if constexpr (SNAP) ra = load_ain(a.ain, a.ain_stride, j);
    } else {
      rp = make_double4(0.0, 0.0, 0.0, 0.0);                     // zero-mass padding, at rest, unaccelerated
      // (the same zeros either way; written as each law's kernel had them: the copy alone sends rp, rv of the jerk forms to scratch)
      if constexpr (SNAP) { rv = rp; ra = rp; }
      else                rv = make_double4(0.0, 0.0, 0.0, 0.0);
    }
  };
  auto store_tile = [&](int buf) {
    double4 q = rp; q.w *= a.gscale; shp[buf][t] = q; shv[buf][t] = rv;
    if constexpr (SNAP) sha[buf][t] = ra;
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
      for (int b = 0; b < JB; ++b) {
        pj[b] = shp[buf][jj + b]; vj[b] = shv[buf][jj + b];
        if constexpr (SNAP) aj[b] = sha[buf][jj + b];
      }
      double dx[JB][IPT], dy[JB][IPT], dz[JB][IPT], s2[JB][IPT], ti[JB][IPT];
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          dx[b][k] = pj[b].x - xi[k]; dy[b][k] = pj[b].y - yi[k]; dz[b][k] = pj[b].z - zi[k];
          if (SOFT) s2[b][k] = fma(dz[b][k], dz[b][k], a.eps2);
          else      s2[b][k] = dz[b][k] * dz[b][k];
          s2[b][k] = fma(dy[b][k], dy[b][k], s2[b][k]);
          s2[b][k] = fma(dx[b][k], dx[b][k], s2[b][k]);
        }
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double r = rsq_dev(s2[b][k]);
          ti[b][k] = (s2[b][k] > 0.0 && (POINTS || jt + jj + b != self[k])) ? r : 0.0;
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
          if constexpr (SNAP) {
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
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    if (il < a.m) {
      double *row = part + ((size_t)c * a.m + il) * W;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        row[q] = A[k][q]; row[3 + q] = J[k][q];
        if constexpr (SNAP) row[6 + q] = S[k][q];
      }
    }
  }
}

// the kernel for one or two rows per lane
template <bool LIST, bool POINTS, bool SNAP>
auto deriv_tile_f64_form(int lanes, bool soft) {
  return lanes == 2 ? (soft ? deriv_tile_f64_kernel<true, 2, LIST, POINTS, SNAP> : deriv_tile_f64_kernel<false, 2, LIST, POINTS, SNAP>)
                    : (soft ? deriv_tile_f64_kernel<true, 1, LIST, POINTS, SNAP> : deriv_tile_f64_kernel<false, 1, LIST, POINTS, SNAP>);
}

}  // namespace
}  // namespace nbody
