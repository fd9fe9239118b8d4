// The fp64 potential and tidal tensor of an fp64 state (nbody_potential_at_f64, nbody_get_potentials_f64, nbody_tidal_at_f64,
// nbody_get_tidal_f64, nbody_tidal_time_f64; build-defined: the reference computes neither).  With d = x_j - x, s^2 = |d|^2 + eps^2:
//     phi(x) = -sum_j G m_j / s        T_ab(x) = sum_j G m_j [3 d_a d_b / s^5 - delta_ab / s^3]
//   pot_tile_f64_kernel<., ., false, .>  <- one sum per row: P = sum G m_j t
//   pot_tile_f64_kernel<., ., true, .>   <- seven sums per row: S_ab = sum (3 G m_j t^5) d_a d_b (six of them), Q = sum G m_j t^3
//   <., ., ., SELF = true>               <- the rows are the bodies (i_first + il of posm), each leaves itself out BY INDEX
//   <., ., ., SELF = false>              <- the rows are caller points (ipos[il]); NO pair is dropped by index
//   pot_fold_f64_kernel                  <- the chunks' rows added from 0.0 in chunk order, phi = -P
//   tidal_fold_f64_kernel                <- the same for the seven sums, then T_aa = S_aa - Q: xx, yy, zz, xy, xz, yz
// A row scan (scan_tile64.h) over tiles of (x, y, z, G m) — no velocity tile: 16 KiB of LDS a workgroup —, with the jerk's
// s2 = fma(dx, dx, fma(dy, dy, dz * dz [+ eps^2])) and rsq_dev.  Per pair, contraction off and every bracket one fp64 operation:
//     t = (s2 > 0 [&& j != self]) ? rsq_dev(s2) : 0;  t2 = t * t;  q = (gm * t) * t2           (the jerk's q)
//     potential:  P = fma(gm, t, P)
//     tidal:      h = (3.0 * q) * t2;  hx = h * dx;  hy = h * dy;  hz = h * dz
//                 Sxx = fma(hx, dx, Sxx);  Sxy = fma(hx, dy, Sxy);  Sxz = fma(hx, dz, Sxz)
//                 Syy = fma(hy, dy, Syy);  Syz = fma(hy, dz, Syz);  Szz = fma(hz, dz, Szz);  Q = Q + q
// h IS G m / s^5 times three: the fp32 kernel (kernels_probe.hip) avoids s^-5 because t^5 leaves the fp32 range long before the
// tensor does; fp64 has the range (t^5 overflows only below s = 1e-61), so forming it costs nothing here.
// One chain per sum and chunk, in body order.  A dropped pair has t = 0: gm * 0 = 0, q = 0, h = 0 — it adds fma(0, ., S) = S and
// Q + 0 = Q, exactly nothing; so does a body of mass 0 (gm = 0) and the zero-mass padding of a chunk's last tile.  With eps > 0 a point
// exactly on body i has d = 0 and t = 1 / eps: hx = hy = hz = 0, so S gets exactly 0, Q gets q = G m_i / eps^3 and P gets G m_i / eps.
// A row's sums depend on the row's point and the bodies alone — not on m, the other rows, the slab, the rows per lane or the device.
// A chunk's partial row is ONE double per row (potential: part[c * m + il]) or EIGHT (tidal: part[(c * m + il) * 8], Sxx, Syy, Szz,
// Sxy, Sxz, Syz, Q and a pad nobody reads: four float4, probe_slab_points(n_total, 4)).  No scratch, no atomics.
#include "kernels.h"

#include "scan_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// local row il = blockIdx.x * (kBlock * IPT) + t + k * kBlock — the lanes past m repeat row m - 1 and write nothing — is
// SELF: body i_first + il of ipos (== posm);  else: point il of ipos — against the bodies of chunk blockIdx.y
template <bool SOFT, int IPT, bool TIDAL, bool SELF>
__global__ __launch_bounds__(kBlock) void pot_tile_f64_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ ipos,
                                                              double *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                              double gscale, double eps2) {
  constexpr int JB = kJerk64Jb, TILE = kJerkTile;
  constexpr int NS = TIDAL ? 7 : 1;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  __shared__ double4 shp[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT];
  int self[IPT];
  double S[IPT][NS];            // potential: P;  tidal: Sxx, Syy, Szz, Sxy, Sxz, Syz, Q
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    self[k] = i_first + min(ibase + t + k * kBlock, m - 1);        // (the points' i_first is 0: the index into ipos)
    const double4 p = ipos[self[k]];
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z;
#pragma unroll
    for (int q = 0; q < NS; ++q) S[k][q] = 0.0;
  }

  double4 rp;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) rp = posm[j];
    else        rp = make_double4(0.0, 0.0, 0.0, 0.0);             // zero-mass padding
  };
  auto store_tile = [&](int buf) {
    double4 q = rp; q.w *= gscale; shp[buf][t] = q;
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
      double4 pj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) pj[b] = shp[buf][jj + b];
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
          if (SELF) ti[b][k] = (s2[b][k] > 0.0 && jt + jj + b != self[k]) ? r : 0.0;
          else      ti[b][k] = (s2[b][k] > 0.0) ? r : 0.0;
        }
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          if constexpr (!TIDAL) {
            S[k][0] = fma(pj[b].w, ti[b][k], S[k][0]);
          } else {
            const double t2 = ti[b][k] * ti[b][k];
            const double q = (pj[b].w * ti[b][k]) * t2;
            const double h = (3.0 * q) * t2;
            const double hx = h * dx[b][k], hy = h * dy[b][k], hz = h * dz[b][k];
            S[k][0] = fma(hx, dx[b][k], S[k][0]); S[k][3] = fma(hx, dy[b][k], S[k][3]); S[k][4] = fma(hx, dz[b][k], S[k][4]);
            S[k][1] = fma(hy, dy[b][k], S[k][1]); S[k][5] = fma(hy, dz[b][k], S[k][5]); S[k][2] = fma(hz, dz[b][k], S[k][2]);
            S[k][NS - 1] = S[k][NS - 1] + q;
          }
        }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    if (il < m) {
      if constexpr (!TIDAL) {
        part[(size_t)c * m + il] = S[k][0];
      } else {
        double *row = part + ((size_t)c * m + il) * 8;
#pragma unroll
        for (int q = 0; q < NS; ++q) row[q] = S[k][q];
      }
    }
  }
}

// phi[k] = -(the chunks' P added from 0.0 in chunk order): no atomics, the same bits every time
__global__ __launch_bounds__(kBlock) void pot_fold_f64_kernel(const double *__restrict__ part, int m, int j_split, double *__restrict__ phi) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double p = 0.0;
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) p = p + part[(size_t)c * m + k];
  phi[k] = -p;
}

// t6[k] = (Sxx - Q, Syy - Q, Szz - Q, Sxy, Sxz, Syz) of the seven sums added from 0.0 in chunk order
__global__ __launch_bounds__(kBlock) void tidal_fold_f64_kernel(const double *__restrict__ part, int m, int j_split, double *__restrict__ t6) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * 8;
#pragma unroll
    for (int q = 0; q < 7; ++q) s[q] = s[q] + row[q];
  }
  double *out = t6 + (size_t)k * 6;
  out[0] = s[0] - s[6]; out[1] = s[1] - s[6]; out[2] = s[2] - s[6];
  out[3] = s[3]; out[4] = s[4]; out[5] = s[5];
}

// both passes: nothing is launched where there is nothing to do, an array is missing, the bodies' form is asked for other than all
// bodies, or the staging area does not hold a slab's partial rows
template <bool TIDAL>
hipError_t launch(const Pot64Launch &L, hipStream_t s) {
  constexpr int W = TIDAL ? kTidal64Width : kPot64Width;
  const bool self = L.ppos == nullptr;
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.part || !L.out || (self && L.m != L.n_total)) return hipErrorInvalidValue;
  if (L.part_elems < probe_part_elems(L.n_total, L.m, W)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;                              // eps == 0: the exact d == 0 rule, as the jerk pass
  for_row_slabs64(L.n_total, L.m, W, self, L.lanes, [&](const RowSlab64 &b) {
    if (self) {
      const auto kernel = soft ? pot_tile_f64_kernel<true, kScan64Ipt, TIDAL, true> : pot_tile_f64_kernel<false, kScan64Ipt, TIDAL, true>;
      hipLaunchKernelGGL(kernel, b.grid, dim3(kBlock), 0, s, (const double4 *)L.posm, (const double4 *)L.posm, (double *)L.part, L.n_total,
                         b.m, (int)b.first, b.j_chunk, L.G, L.eps2);
    } else {
      const auto kernel = b.ipt == 2 ? (soft ? pot_tile_f64_kernel<true, 2, TIDAL, false> : pot_tile_f64_kernel<false, 2, TIDAL, false>)
                                     : (soft ? pot_tile_f64_kernel<true, 1, TIDAL, false> : pot_tile_f64_kernel<false, 1, TIDAL, false>);
      hipLaunchKernelGGL(kernel, b.grid, dim3(kBlock), 0, s, (const double4 *)L.posm, (const double4 *)L.ppos + b.first, (double *)L.part,
                         L.n_total, b.m, 0, b.j_chunk, L.G, L.eps2);
    }
    if (TIDAL)
      hipLaunchKernelGGL(tidal_fold_f64_kernel, b.fold, dim3(kBlock), 0, s, (const double *)L.part, b.m, b.j_split, L.out + 6 * b.first);
    else
      hipLaunchKernelGGL(pot_fold_f64_kernel, b.fold, dim3(kBlock), 0, s, (const double *)L.part, b.m, b.j_split, L.out + b.first);
  });
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pot_f64(const Pot64Launch &L, hipStream_t s) { return launch<false>(L, s); }
hipError_t launch_tidal_f64(const Pot64Launch &L, hipStream_t s) { return launch<true>(L, s); }

}  // namespace nbody
