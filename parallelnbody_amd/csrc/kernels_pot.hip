// The bodies' gravitational potential at theta = 0 (nbody_potential_at, nbody_get_potentials, nbody_energy_fast; build-defined: the
// reference computes no potential):
//   probe_pot_pk_kernel    <- phi(x) = -sum_j G m_j / sqrt(|x - x_j|^2 + eps^2): probe_tile_pk_kernel's shape (kernels_probe.hip) with one
//                             accumulator instead of three and no cube; SELF: the points are the bodies themselves, j == i dropped by index
//   pot_fold_kernel        <- the chunks' partial rows added in chunk order in fp64, negated, rounded once
//   energy_fast_*_kernel   <- 1/2 m v^2 and 1/2 m phi from the unrounded potentials, reduced in a fixed order
// The theta > 0 counterpart — the walk of the last tree — is bh_pot_walk_kernel (kernels_bh_pot.hip).
#include "kernels.h"

#include <algorithm>

#include "../../include/nbody.h"
#include "pk_common.h"

namespace nbody {

namespace {

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

// probe_tile_pk_kernel (kernels_probe.hip) for the potential: lanes hold their points two by two in register pairs, the bodies go
// through double-buffered LDS tiles as (x, y, z, G m), every constant in a VGPR.
//   grid.x : blocks of kBlock * 2 NP points (lane t holds points base + t + k * kBlock: coalesced)
//   grid.y : j chunks [c * j_chunk, min((c + 1) * j_chunk, n_total)); each writes its own partial row part[c][m], one float per point
// Ragged tiles are padded with zero-mass bodies on the origin (0 * a finite term: nothing).  SELF: `probe` is posm + i_first, the points
// are bodies i_first .. i_first + m, and the tiles that overlap the workgroup's own bodies run the guarded group; all others the plain one.
template <int NP, int TILE, int ZMODE, bool SELF>
__global__ __launch_bounds__(kBlock) void probe_pot_pk_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ probe,
                                                              float *__restrict__ part, int n_total, int m, int i_first, int j_chunk,
                                                              float gscale, float zp, unsigned long long *__restrict__ clk) {
  constexpr int IPT = 2 * NP;
  constexpr int LPT = (TILE + kBlock - 1) / kBlock;
  constexpr int JB = (NP == 1) ? 4 : 2;
  const ClockStamp stamp = clock_begin(clk);
  __shared__ float4 sh[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  f2 xi[NP], yi[NP], zi[NP], a[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float4 p0 = probe[min(ibase + t + (2 * p) * kBlock, m - 1)];
    const float4 p1 = probe[min(ibase + t + (2 * p + 1) * kBlock, m - 1)];
    xi[p] = f2{p0.x, p1.x}; yi[p] = f2{p0.y, p1.y}; zi[p] = f2{p0.z, p1.z};
    a[p] = splat2(0.f);
  }
  // every loop-invariant operand in VGPRs (an SGPR operand halves the issue rate), loads consumed before the loops
  f2 zp2 = splat2(zp), one2 = splat2(1.0f);
  asm volatile("" : "+v"(zp2), "+v"(one2));
#pragma unroll
  for (int p = 0; p < NP; ++p) asm volatile("" ::"v"(xi[p]), "v"(yi[p]), "v"(zi[p]));

  float4 r[LPT];
  auto load_tile = [&](int tile) {
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
      const int e = t + l * kBlock;
      if (e < TILE) {
        const int j = j0 + tile * TILE + e;
        if (j < j1) r[l] = posm[j];
        else        r[l] = make_float4(0.f, 0.f, 0.f, 0.f);   // zero-mass padding
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
      const int e = t + l * kBlock;
      if (e < TILE) { float4 q = r[l]; q.w *= gscale; sh[buf][e] = q; }
    }
  };

  // the workgroup's own bodies, as indices of posm (SELF)
  const int own0 = i_first + ibase, own1 = own0 + kBlock * IPT;

  if (ntiles > 0) { load_tile(0); store_tile(0); }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
    const int jt = j0 + tile * TILE;
    if (SELF && jt < own1 && jt + TILE > own0) {               // (uniform over the workgroup)
      const int rel0 = jt - (own0 + t);
#pragma unroll 2
      for (int jj = 0; jj < TILE; jj += JB) {
        float4 pj[JB];
#pragma unroll
        for (int b = 0; b < JB; ++b) pj[b] = sh[buf][jj + b];
        pot_group_pk<NP, JB, ZMODE, true>(xi, yi, zi, pj, zp2, one2, a, rel0 + jj);
      }
    } else {
#pragma unroll 2
      for (int jj = 0; jj < TILE; jj += JB) {
        float4 pj[JB];
#pragma unroll
        for (int b = 0; b < JB; ++b) pj[b] = sh[buf][jj + b];
        pot_group_pk<NP, JB, ZMODE, false>(xi, yi, zi, pj, zp2, one2, a, 0);
      }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int il0 = ibase + t + (2 * p) * kBlock, il1 = il0 + kBlock;
    if (il0 < m) part[(size_t)c * m + il0] = a[p].x;
    if (il1 < m) part[(size_t)c * m + il1] = a[p].y;
  }
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

constexpr int kPotTile = 256;   // = kernels_probe.hip's tile: probe_geometry's chunks are whole tiles of it

template <int NP, bool SELF>
void launch_pot_np(const PotLaunch &L, int m, int i_first, const float4 *probe, int j_split, int j_chunk, hipStream_t s) {
  const dim3 grid((m + kBlock * 2 * NP - 1) / (kBlock * 2 * NP), j_split), block(kBlock);
  // eps == 0: the exact d == 0 rule whatever the context's zero_mode is (an eps floor would add G m / 1e-10 for a point on a body)
  if (L.eps2 > 0.0)
    hipLaunchKernelGGL((probe_pot_pk_kernel<NP, kPotTile, Z_SOFT, SELF>), grid, block, 0, s, (const float4 *)L.posm, probe, (float *)L.part,
                       L.n_total, m, i_first, j_chunk, (float)L.G, (float)L.eps2, (unsigned long long *)L.clk);
  else
    hipLaunchKernelGGL((probe_pot_pk_kernel<NP, kPotTile, Z_CLAMP, SELF>), grid, block, 0, s, (const float4 *)L.posm, probe, (float *)L.part,
                       L.n_total, m, i_first, j_chunk, (float)L.G, -0x1p126f, (unsigned long long *)L.clk);
}

}  // namespace

// Points in the slabs of launch_probe (probe_slab_points: the rows are a quarter of the field's, so they fit its staging area); which
// slab a point falls into, and which workgroup shape its slab gets, changes nothing it is summed from.
hipError_t launch_pot(const PotLaunch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.part || (!L.phi64 && !L.phif)) return hipErrorInvalidValue;
  const bool self = L.probe == nullptr;
  if (self && L.m != L.n_total) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total);
  for (size_t first = 0; first < (size_t)L.m; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.m - first);
    const float4 *probe = (self ? (const float4 *)L.posm : (const float4 *)L.probe) + first;
    const long long wgs2 = (long long)((m + 4 * kBlock - 1) / (4 * kBlock)) * j_split;
    if (self) {
      if (wgs2 < 1024) launch_pot_np<1, true>(L, m, (int)first, probe, j_split, j_chunk, s);
      else             launch_pot_np<2, true>(L, m, (int)first, probe, j_split, j_chunk, s);
    } else {
      if (wgs2 < 1024) launch_pot_np<1, false>(L, m, 0, probe, j_split, j_chunk, s);
      else             launch_pot_np<2, false>(L, m, 0, probe, j_split, j_chunk, s);
    }
    hipLaunchKernelGGL(pot_fold_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const float *)L.part, m, j_split,
                       L.phi64 ? (double *)L.phi64 + first : nullptr, L.phif ? (float *)L.phif + first : nullptr);
  }
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
