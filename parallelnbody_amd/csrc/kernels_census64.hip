// The fp64 pair census of an fp64 state (nbody_get_nearest_f64, nbody_nearest_at_f64, nbody_closest_pair_f64, nbody_get_partners_f64,
// nbody_partner_at_f64, nbody_hardest_pair_f64, nbody_pair_time_f64; build-defined: the reference computes none of it).  For a row at
// (x, v) with mass term g (a body: g = G m_i; a point: g = 0) and body j, with d = x_j - x and w = v_j - v:
//     d2 = fma(dx, dx, fma(dy, dy, dz * dz))                      never softened
//     s2 = d2 + eps^2 (d2 itself when eps == 0);  t = (s2 > 0 [&& j != self]) ? rsq_dev(s2) : 0
//     w2 = fma(wx, wx, fma(wy, wy, wz * wz));  e = fma(-(G m_j + g), t, 0.5 * w2)      the pair's specific orbital energy
//   census_tile_f64_kernel<., ., false, .>  <- NEAREST: the body with the smallest d2 per row — no root at all
//   census_tile_f64_kernel<., ., true, .>   <- PARTNER: the body with the smallest e per row, its d2 beside it
//   <., ., ., SELF = true>                  <- the rows are the bodies (i_first + il of posm, vel), each leaves itself out BY INDEX
//   <., ., ., SELF = false>                 <- the rows are caller points (ipos[il], ivel[il]); NO body is dropped by index
//   census_fold_f64_kernel<BOUND>           <- the chunks' rows taken in chunk order with strict <, from (+inf, -1)
//   census_pair_parts / _fold_kernel        <- the smallest value over the rows and the lowest row that attains it, in a fixed order
// A row scan (scan_tile64.h) over tiles of (x, y, z, G m) — PARTNER: the velocity tile beside it, 32 KiB of LDS a workgroup as the jerk.
// Each lane keeps (best, index) — PARTNER: and d2 — per row and updates them with compare and select in ASCENDING j, under strict <:
// the lowest index wins a tie, a NaN is never chosen (< is false), nor is a d2 that is not finite (NEAREST: +inf < +inf is false;
// PARTNER: the candidate must have d2 < +inf, which also keeps out the body whose position is NaN — its s2 > 0 is false, so its t
// would be 0 and its e the finite 0.5 w2).  The candidates are the bodies j0 <= j < j1 of the chunk: the zero padding of a chunk's last
// tile is NOT a body and is kept out BY INDEX (j < j1), not by mass — it sits at the origin.  A zero-mass body is a candidate; a
// coincident body (d2 == 0) is one too, at every eps, and is the nearest.
// e_ij and e_ji come from the same operations on negated operands (G m_j + g commutes), d2_ij and d2_ji likewise: both are symmetric
// in every bit.  A row's result depends on the row and the bodies alone — not on m, the other rows, the slab, the rows per lane or
// the device.  A chunk's partial row is (d2, index) — 16 B, one float4 — or (e, d2, index, pad) — 32 B, two float4 —, the index as a
// double (exact).  No scratch, no atomics.
#include "kernels.h"

#include "scan_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// local row il = blockIdx.x * (kBlock * IPT) + t + k * kBlock — the lanes past m repeat row m - 1 and write nothing — is
// SELF: body i_first + il of (ipos, ivel) (== posm, vel);  else: point il of (ipos, ivel) — against the bodies of chunk blockIdx.y
template <bool SOFT, int IPT, bool BOUND, bool SELF>
__global__ __launch_bounds__(kBlock) void census_tile_f64_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                 const double4 *__restrict__ ipos, const double4 *__restrict__ ivel,
                                                                 double *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                                 double gscale, double eps2) {
  constexpr int JB = kJerk64Jb, TILE = kJerkTile;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  static_assert(BOUND || !SOFT, "the nearest form has no softening to apply");
  __shared__ double4 shp[2][TILE];
  __shared__ double4 shv[BOUND ? 2 : 1][BOUND ? TILE : 1];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT], vxi[IPT], vyi[IPT], vzi[IPT], gi[IPT];
  int self[IPT];
  double best[IPT], bd2[IPT];   // NEAREST: the smallest d2;  PARTNER: the smallest e and that body's d2
  int at[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    self[k] = i_first + min(ibase + t + k * kBlock, m - 1);        // (the points' i_first is 0: the index into ipos)
    const double4 p = ipos[self[k]];
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z;
    gi[k] = SELF ? p.w * gscale : 0.0;
    if (BOUND) { const double4 v = ivel[self[k]]; vxi[k] = v.x; vyi[k] = v.y; vzi[k] = v.z; }
    else       { vxi[k] = vyi[k] = vzi[k] = 0.0; }
    best[k] = __builtin_inf(); bd2[k] = __builtin_inf(); at[k] = -1;
  }

  double4 rp, rv;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) { rp = posm[j]; if (BOUND) rv = vel[j]; }
    else        { rp = make_double4(0.0, 0.0, 0.0, 0.0); if (BOUND) rv = make_double4(0.0, 0.0, 0.0, 0.0); }   // padding: never a candidate
  };
  auto store_tile = [&](int buf) {
    double4 q = rp; q.w *= gscale; shp[buf][t] = q;
    if (BOUND) shv[buf][t] = rv;
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
      double4 pj[JB], vj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) { pj[b] = shp[buf][jj + b]; if (BOUND) vj[b] = shv[buf][jj + b]; }
      double d2[JB][IPT], ti[JB][IPT];
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double dx = pj[b].x - xi[k], dy = pj[b].y - yi[k], dz = pj[b].z - zi[k];
          d2[b][k] = dz * dz;
          d2[b][k] = fma(dy, dy, d2[b][k]);
          d2[b][k] = fma(dx, dx, d2[b][k]);
        }
      if constexpr (BOUND) {
#pragma unroll
        for (int b = 0; b < JB; ++b)
#pragma unroll
          for (int k = 0; k < IPT; ++k) {
            const double s2 = SOFT ? d2[b][k] + eps2 : d2[b][k];
            const double r = rsq_dev(s2);
            if (SELF) ti[b][k] = (s2 > 0.0 && jt + jj + b != self[k]) ? r : 0.0;
            else      ti[b][k] = (s2 > 0.0) ? r : 0.0;
          }
      }
#pragma unroll
      for (int b = 0; b < JB; ++b)                                 // ascending j: b, then the next group
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const int j = jt + jj + b;
          bool cand = j < j1;
          if (SELF) cand = cand && j != self[k];
          if constexpr (!BOUND) {
            const bool take = cand && d2[b][k] < best[k];
            best[k] = take ? d2[b][k] : best[k];
            at[k] = take ? j : at[k];
          } else {
            const double wx = vj[b].x - vxi[k], wy = vj[b].y - vyi[k], wz = vj[b].z - vzi[k];
            double w2 = wz * wz;
            w2 = fma(wy, wy, w2);
            w2 = fma(wx, wx, w2);
            const double e = fma(-(pj[b].w + gi[k]), ti[b][k], 0.5 * w2);
            const bool take = cand && e < best[k] && d2[b][k] < __builtin_inf();
            best[k] = take ? e : best[k];
            bd2[k] = take ? d2[b][k] : bd2[k];
            at[k] = take ? j : at[k];
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
      if constexpr (!BOUND) {
        double *row = part + ((size_t)c * m + il) * 2;
        row[0] = best[k]; row[1] = (double)at[k];
      } else {
        double *row = part + ((size_t)c * m + il) * 4;
        row[0] = best[k]; row[1] = bd2[k]; row[2] = (double)at[k];
      }
    }
  }
}

// row k's answer: the chunks' rows in chunk order under strict <, from (+inf, -1) — the chunks ascend in j, so the lowest index wins
// NEAREST: index[k], a[k] = d2;  PARTNER: index[k], a[k] = e, b[k] = d2
template <bool BOUND>
__global__ __launch_bounds__(kBlock) void census_fold_f64_kernel(const double *__restrict__ part, int m, int j_split, int *__restrict__ index,
                                                                 double *__restrict__ a, double *__restrict__ b) {
  constexpr int W = BOUND ? 4 : 2;
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double best = __builtin_inf(), d2 = __builtin_inf(), at = -1.0;
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * W;
    const bool take = row[0] < best;
    best = take ? row[0] : best;
    at = take ? row[BOUND ? 2 : 1] : at;
    if (BOUND) d2 = take ? row[1] : d2;
  }
  index[k] = (int)at;
  a[k] = best;
  if (BOUND) b[k] = d2;
}

// The pair reductions, shaped like launch_tidal_time's (kernels_probe.hip): two launches, no atomics, the same bits and the same row every
// run.  A candidate is (value, row); the smallest value wins, the lowest row among equals: value_at_workgroup<false> (pk_common.h).
__global__ __launch_bounds__(kBlock) void census_pair_parts_kernel(const double *__restrict__ value, int n, double *__restrict__ part) {
  __shared__ ValueAt red[kBlock / 64];
  ValueAt a{__builtin_inf(), 0x7fffffff};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) value_at_take<false>(a, value[i], i);
  const ValueAt r = value_at_workgroup<false>(a, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = r.v; part[2 * blockIdx.x + 1] = (double)r.i; }
}
// out[0] = the smallest value, out[1] = its row i, out[2] = index[i], out[3] = aux[i] (aux == nullptr: the value again);
// no row below +inf: (+inf, -1, -1, +inf)
__global__ __launch_bounds__(kBlock) void census_pair_fold_kernel(const double *__restrict__ part, int slots, const int *__restrict__ index,
                                                                  const double *__restrict__ aux, double *__restrict__ out) {
  __shared__ ValueAt red[kBlock / 64];
  ValueAt a{__builtin_inf(), 0x7fffffff};
  for (int q = threadIdx.x; q < slots; q += kBlock) value_at_take<false>(a, part[2 * q], (int)part[2 * q + 1]);
  const ValueAt r = value_at_workgroup<false>(a, red);
  if (threadIdx.x == 0) {
    const bool some = r.v < __builtin_inf();
    out[0] = some ? r.v : __builtin_inf();
    out[1] = some ? (double)r.i : -1.0;
    out[2] = some ? (double)index[r.i] : -1.0;
    out[3] = some ? (aux ? aux[r.i] : r.v) : __builtin_inf();
  }
}

// both passes: nothing is launched where there is nothing to do, an array is missing, the bodies' form is asked for other than all
// bodies, or the staging area does not hold a slab's partial rows
template <bool BOUND>
hipError_t launch(const Census64Launch &L, hipStream_t s) {
  constexpr int W = BOUND ? kPartner64Width : kNearest64Width;
  const bool self = L.ppos == nullptr;
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.part || !L.index || !L.value || (self && L.m != L.n_total)) return hipErrorInvalidValue;
  if (BOUND && (!L.vel || !L.d2 || (!self && !L.pvel))) return hipErrorInvalidValue;
  if (L.part_elems < probe_part_elems(L.n_total, L.m, W)) return hipErrorInvalidValue;
  const bool soft = BOUND && L.eps2 > 0.0;                     // eps == 0: s2 is d2 itself
  const double4 *posm = (const double4 *)L.posm, *vel = (const double4 *)L.vel;
  for_row_slabs64(L.n_total, L.m, W, self, L.lanes, [&](const RowSlab64 &b) {
    if (self) {
      auto kernel = census_tile_f64_kernel<false, kScan64Ipt, BOUND, true>;
      if constexpr (BOUND) { if (soft) kernel = census_tile_f64_kernel<true, kScan64Ipt, true, true>; }
      hipLaunchKernelGGL(kernel, b.grid, dim3(kBlock), 0, s, posm, vel, posm, vel, (double *)L.part, L.n_total, b.m, (int)b.first, b.j_chunk,
                         L.G, L.eps2);
    } else {
      auto kernel = b.ipt == 2 ? census_tile_f64_kernel<false, 2, BOUND, false> : census_tile_f64_kernel<false, 1, BOUND, false>;
      if constexpr (BOUND) { if (soft) kernel = b.ipt == 2 ? census_tile_f64_kernel<true, 2, true, false> : census_tile_f64_kernel<true, 1, true, false>; }
      hipLaunchKernelGGL(kernel, b.grid, dim3(kBlock), 0, s, posm, vel, (const double4 *)L.ppos + b.first,
                         BOUND ? (const double4 *)L.pvel + b.first : nullptr, (double *)L.part, L.n_total, b.m, 0, b.j_chunk, L.G, L.eps2);
    }
    hipLaunchKernelGGL(census_fold_f64_kernel<BOUND>, b.fold, dim3(kBlock), 0, s, (const double *)L.part, b.m, b.j_split, L.index + b.first,
                       L.value + b.first, BOUND ? L.d2 + b.first : nullptr);
  });
  return hipGetLastError();
}

}  // namespace

hipError_t launch_nearest_f64(const Census64Launch &L, hipStream_t s) { return launch<false>(L, s); }
hipError_t launch_partner_f64(const Census64Launch &L, hipStream_t s) { return launch<true>(L, s); }

hipError_t launch_census_pair(const double *value, const int *index, const double *aux, int n, double *partials, double *out, hipStream_t s) {
  if (n <= 0 || !value || !index || !partials || !out) return hipErrorInvalidValue;
  const int slots = energy_fast_slots(n);
  hipLaunchKernelGGL(census_pair_parts_kernel, dim3(slots), dim3(kBlock), 0, s, value, n, partials);
  hipLaunchKernelGGL(census_pair_fold_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)partials, slots, index, aux, out);
  return hipGetLastError();
}

}  // namespace nbody
