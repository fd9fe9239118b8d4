// The fp64 jerk and snap passes at points that are not bodies (nbody_jerk_at_f64 and the fp64 tracers of the shared-step Hermite calls:
// nbody_set_tracers_f64, nbody_hermite_step, nbody_hermite6_step and their advances; build-defined: the reference computes none).
//   jerk_points_f64_kernel <- the tile loop of jerk_tile64.h with the i side taken from caller arrays: m points as double4 positions and
//                             double4 velocities against all n_total bodies
//   snap_points_f64_kernel <- the tile loop of snap_tile64.h the same way; a point's input acceleration (the acc_i of b = acc_j - acc_i)
//                             is three doubles at pain[k * pain_stride]
//   <., ., true> of both   <- the LIST forms: the i side taken through an index list — the ACTIVE tracers of a block step
//                             (nbody_hermite[6]_block_begin_tracers), rows of the tracers' predicted arrays —, the partial rows left
//                             unfolded for the block corrector.  The <., ., false> forms are instruction for instruction the kernels
//                             they were (profiles/block_tracers_isa_compare.txt)
// Both are SIBLINGS of the body templates, not further forms of them: the two headers stay as they are, and so does every kernel built
// from them (profiles/tracers_f64_isa_compare.txt).  What they share is written out again here, operation for operation in the same
// order: the chunks of probe_geometry(n_total), the double-buffered 256-body LDS tiles, two j-bodies per staged group,
// s2 = fma(dx, dx, fma(dy, dy, dz * dz [+ eps^2])), rsq_dev, t2, q, dw, k3, u, the A and J chains and the snap's g and S chains.  The ONE
// difference: no pair is dropped by index — t = (s2 > 0) ? rsq_dev(s2) : 0.  With eps == 0 a point exactly on a body drops that pair
// from every sum; with eps > 0 that pair has d = 0 and adds G m w / eps^3 to the jerk, G m b / eps^3 to the snap and nothing to a (the
// rule nbody_get_snap_f64 documents for coincident bodies).  A zero-mass body adds fma(0, finite, A) = A: exactly nothing.
// A point's sums depend on the point and the bodies alone — not on m, the other points, the slab, the points per lane or the device:
// a body asked about as a point at its own (x, v) gets nbody_get_jerk_f64's bits (its own pair has s2 == 0, or q d = 0 and w = 0).
// The chunks' rows — part[(c * m + il) * W], W = 6 / 9 doubles — are folded from 0.0 in chunk order by the fold kernels of
// kernels_jerk.hip and kernels_snap.hip.  No scratch, no atomics.
#include "kernels.h"

#include <algorithm>

#include "jerk_tile64.h"
#include "snap_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// local point il = blockIdx.x * (kBlock * IPT) + t + k * kBlock of the slab (ppos, pvel) — the lanes past m repeat point m - 1 and
// write nothing — against the bodies of chunk blockIdx.y
// LIST: local point il is row list[il] of (ppos, pvel) — the active tracers of a block step in the tracers' predicted arrays —, its
// partial row still part[(c * m + il) * 6]
template <bool SOFT, int IPT, bool LIST>
__global__ __launch_bounds__(kBlock) void jerk_points_f64_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                 const double4 *__restrict__ ppos, const double4 *__restrict__ pvel,
                                                                 double *__restrict__ part, int n_total, int m, int j_chunk,
                                                                 double gscale, double eps2, const int *__restrict__ list) {
  constexpr int JB = kJerk64Jb, TILE = kJerkTile;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  __shared__ double4 shp[2][TILE], shv[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT], vxi[IPT], vyi[IPT], vzi[IPT];
  double A[IPT][3], J[IPT][3];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = min(ibase + t + k * kBlock, m - 1);
    const int ip = LIST ? list[il] : il;
    const double4 p = ppos[ip], v = pvel[ip];
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z; vxi[k] = v.x; vyi[k] = v.y; vzi[k] = v.z;
#pragma unroll
    for (int q = 0; q < 3; ++q) { A[k][q] = 0.0; J[k][q] = 0.0; }
  }

  double4 rp, rv;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) { rp = posm[j]; rv = vel[j]; }
    else        { rp = make_double4(0.0, 0.0, 0.0, 0.0); rv = make_double4(0.0, 0.0, 0.0, 0.0); }   // zero-mass padding, at rest
  };
  auto store_tile = [&](int buf) {
    double4 q = rp; q.w *= gscale; shp[buf][t] = q; shv[buf][t] = rv;
  };

  if (ntiles > 0) { load_tile(0); store_tile(0); }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
#pragma unroll 2
    for (int jj = 0; jj < TILE; jj += JB) {
      double4 pj[JB], vj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) { pj[b] = shp[buf][jj + b]; vj[b] = shv[buf][jj + b]; }
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
          const double r = rsq_dev(s2[b][k]);
          ti[b][k] = (s2[b][k] > 0.0) ? r : 0.0;
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
        }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    if (il < m) {
      double *row = part + ((size_t)c * m + il) * 6;
      row[0] = A[k][0]; row[1] = A[k][1]; row[2] = A[k][2]; row[3] = J[k][0]; row[4] = J[k][1]; row[5] = J[k][2];
    }
  }
}

// the same for the snap: ain holds body j's input acceleration at ain[j * ain_stride + 0 .. 2], pain point il's at pain[il * pain_stride + 0 .. 2]
// (LIST: pain is read at row list[il] too)
template <bool SOFT, int IPT, bool LIST>
__global__ __launch_bounds__(kBlock) void snap_points_f64_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                 const double *__restrict__ ain, int ain_stride,
                                                                 const double4 *__restrict__ ppos, const double4 *__restrict__ pvel,
                                                                 const double *__restrict__ pain, int pain_stride,
                                                                 double *__restrict__ part, int n_total, int m, int j_chunk,
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
  double A[IPT][3], J[IPT][3], S[IPT][3];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = min(ibase + t + k * kBlock, m - 1);
    const int ip = LIST ? list[il] : il;
    const double4 p = ppos[ip], v = pvel[ip], a = load_ain(pain, pain_stride, ip);
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
          ti[b][k] = (s2[b][k] > 0.0) ? r : 0.0;
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

// what both launchers refuse: nothing to do, a missing array, or a staging area that does not hold a slab's rows
bool bad(const Points64Launch &L, int width, bool folds = true) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.vel || !L.ppos || !L.pvel || !L.part || (folds && !L.out)) return true;
  return L.part_elems < probe_part_elems(L.n_total, L.m, width);
}

}  // namespace

hipError_t launch_jerk_points_f64(const Points64Launch &L, hipStream_t s) {
  if (bad(L, 3)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;                              // eps == 0: the exact d == 0 rule, as the bodies' pass
  const int ipt = hermite_block_lanes(L.m, L.lanes);           // one or two points per lane, as the block evaluation picks them
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total, 3);         // a row of six doubles: three float4
  for (size_t first = 0; first < (size_t)L.m; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.m - first);
    const dim3 grid((m + kBlock * ipt - 1) / (kBlock * ipt), j_split);
    const auto kernel = ipt == 2 ? (soft ? jerk_points_f64_kernel<true, 2, false> : jerk_points_f64_kernel<false, 2, false>)
                                 : (soft ? jerk_points_f64_kernel<true, 1, false> : jerk_points_f64_kernel<false, 1, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const double4 *)L.posm, (const double4 *)L.vel, (const double4 *)L.ppos + first,
                       (const double4 *)L.pvel + first, (double *)L.part, L.n_total, m, j_chunk, L.G, L.eps2, (const int *)nullptr);
    if (hipError_t e = launch_jerk_fold_f64(L.part, m, j_split, L.out + 6 * first, s)) return e;
  }
  return hipGetLastError();
}

hipError_t launch_snap_points_f64(const Points64Launch &L, hipStream_t s) {
  if (bad(L, kSnapRowWidth) || !L.ain || L.ain_stride < 3 || !L.pain || L.pain_stride < 3) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  const int ipt = hermite_block_lanes(L.m, L.lanes);
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total, kSnapRowWidth);
  for (size_t first = 0; first < (size_t)L.m; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.m - first);
    const dim3 grid((m + kBlock * ipt - 1) / (kBlock * ipt), j_split);
    const auto kernel = ipt == 2 ? (soft ? snap_points_f64_kernel<true, 2, false> : snap_points_f64_kernel<false, 2, false>)
                                 : (soft ? snap_points_f64_kernel<true, 1, false> : snap_points_f64_kernel<false, 1, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const double4 *)L.posm, (const double4 *)L.vel, L.ain, L.ain_stride,
                       (const double4 *)L.ppos + first, (const double4 *)L.pvel + first, L.pain + first * (size_t)L.pain_stride, L.pain_stride,
                       (double *)L.part, L.n_total, m, j_chunk, L.G, L.eps2, (const int *)nullptr);
    if (hipError_t e = launch_snap_fold_f64(L.part, m, j_split, L.out + 9 * first, s)) return e;
  }
  return hipGetLastError();
}

// The list forms: ONE slab — list[0 .. m), m <= the slab — into part, unfolded: the block corrector adds the chunks' rows itself.
hipError_t launch_jerk_points_list_f64(const Points64Launch &L, const int *list, hipStream_t s) {
  if (bad(L, 3, false) || !list || (size_t)L.m > probe_slab_points(L.n_total, 3) || (L.lanes != 1 && L.lanes != 2)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const dim3 grid((L.m + kBlock * L.lanes - 1) / (kBlock * L.lanes), j_split);
  const auto kernel = L.lanes == 2 ? (soft ? jerk_points_f64_kernel<true, 2, true> : jerk_points_f64_kernel<false, 2, true>)
                                   : (soft ? jerk_points_f64_kernel<true, 1, true> : jerk_points_f64_kernel<false, 1, true>);
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const double4 *)L.posm, (const double4 *)L.vel, (const double4 *)L.ppos,
                     (const double4 *)L.pvel, (double *)L.part, L.n_total, L.m, j_chunk, L.G, L.eps2, list);
  return hipGetLastError();
}

hipError_t launch_snap_points_list_f64(const Points64Launch &L, const int *list, hipStream_t s) {
  if (bad(L, kSnapRowWidth, false) || !list || !L.ain || L.ain_stride < 3 || !L.pain || L.pain_stride < 3 ||
      (size_t)L.m > probe_slab_points(L.n_total, kSnapRowWidth) || (L.lanes != 1 && L.lanes != 2))
    return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const dim3 grid((L.m + kBlock * L.lanes - 1) / (kBlock * L.lanes), j_split);
  const auto kernel = L.lanes == 2 ? (soft ? snap_points_f64_kernel<true, 2, true> : snap_points_f64_kernel<false, 2, true>)
                                   : (soft ? snap_points_f64_kernel<true, 1, true> : snap_points_f64_kernel<false, 1, true>);
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const double4 *)L.posm, (const double4 *)L.vel, L.ain, L.ain_stride,
                     (const double4 *)L.ppos, (const double4 *)L.pvel, L.pain, L.pain_stride, (double *)L.part, L.n_total, L.m, j_chunk,
                     L.G, L.eps2, list);
  return hipGetLastError();
}

}  // namespace nbody
