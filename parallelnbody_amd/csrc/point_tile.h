// The tile loop of the theta = 0 point queries (kernels_probe.hip, kernels_jerk.hip): points held in registers against every body, the
// bodies going through LDS.  forces_tile_pk_kernel (kernels.hip) with the i-bodies from `probe` [m] instead of posm: lanes hold their
// points two by two in register pairs, the bodies go through double-buffered LDS tiles as (x, y, z, G m), every constant in a VGPR.
//   grid.x : blocks of kBlock * 2 NP points (lane t holds points base + t + k * kBlock: coalesced)
//   grid.y : j chunks [c * j_chunk, min((c + 1) * j_chunk, n_total)); each writes its own partial row part[c][m]
// What a pair adds and what a chunk's row holds is the kernel's: a per-tile functor and a write-out.  VEL (the jerk): the bodies'
// velocities go through a second pair of LDS tiles beside their positions, and the points carry theirs in register pairs.
// Also here, shared by the two files: the points' slabs (for_point_slabs).
#pragma once
#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "pk_common.h"

namespace nbody {
namespace {

constexpr int point_group(int NP) { return NP == 1 ? 4 : 2; }   // JB: the bodies of one pair group

// The chunk's tiles in body order: on_tile(jt, tile, xi, yi, zi, zp2, one2) once per tile — jt the index of the tile's first body,
// tile its TILE bodies in LDS.  Ragged tiles are padded with zero-mass bodies on the origin.  Points past m repeat point m - 1.
// VEL: on_tile(jt, tile, vtile, xi, yi, zi, vxi, vyi, vzi, zp2, one2) — vtile the same bodies' velocities (velj, float4 each, the 4th
// unused; the padding is at rest), vxi ... the points' (pvel [m], float4 each).  What VEL adds sits in `if constexpr` and in structs
// that are empty without it, and its two arrays come last: the kernels without velocities keep their code instruction for instruction.
template <bool VEL, int N> struct VelPairs { f2 x[N], y[N], z[N]; };
template <int N> struct VelPairs<false, N> {};
template <bool VEL, int N> struct VelQuads { float4 q[N]; };
template <int N> struct VelQuads<false, N> {};

template <int NP, int TILE, bool VEL = false, class OnTile>
__device__ __forceinline__ void point_tile_loop(const float4 *__restrict__ posm, const float4 *__restrict__ probe, int n_total, int m,
                                                int j_chunk, float gscale, float zp, OnTile on_tile, const float4 *__restrict__ velj = nullptr,
                                                const float4 *__restrict__ pvel = nullptr) {
  constexpr int IPT = 2 * NP;
  constexpr int LPT = (TILE + kBlock - 1) / kBlock;
  __shared__ float4 sh[2][TILE];
  float4 (*shv)[TILE] = nullptr;
  if constexpr (VEL) {
    __shared__ float4 shv_[2][TILE];
    shv = shv_;
  }

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  f2 xi[NP], yi[NP], zi[NP];
  VelPairs<VEL, NP> vi;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float4 p0 = probe[min(ibase + t + (2 * p) * kBlock, m - 1)];
    const float4 p1 = probe[min(ibase + t + (2 * p + 1) * kBlock, m - 1)];
    xi[p] = f2{p0.x, p1.x}; yi[p] = f2{p0.y, p1.y}; zi[p] = f2{p0.z, p1.z};
    if constexpr (VEL) {
      const float4 v0 = pvel[min(ibase + t + (2 * p) * kBlock, m - 1)];
      const float4 v1 = pvel[min(ibase + t + (2 * p + 1) * kBlock, m - 1)];
      vi.x[p] = f2{v0.x, v1.x}; vi.y[p] = f2{v0.y, v1.y}; vi.z[p] = f2{v0.z, v1.z};
    }
  }
  // every loop-invariant operand in VGPRs (an SGPR operand halves the issue rate), loads consumed before the loops
  f2 zp2 = splat2(zp), one2 = splat2(1.0f);
  asm volatile("" : "+v"(zp2), "+v"(one2));
#pragma unroll
  for (int p = 0; p < NP; ++p) asm volatile("" ::"v"(xi[p]), "v"(yi[p]), "v"(zi[p]));
  if constexpr (VEL) {
#pragma unroll
    for (int p = 0; p < NP; ++p) asm volatile("" ::"v"(vi.x[p]), "v"(vi.y[p]), "v"(vi.z[p]));
  }

  float4 r[LPT];
  VelQuads<VEL, LPT> rv;
  auto load_tile = [&](int tile) {
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
      const int e = t + l * kBlock;
      if (e < TILE) {
        const int j = j0 + tile * TILE + e;
        if (j < j1) r[l] = posm[j];
        else        r[l] = make_float4(0.f, 0.f, 0.f, 0.f);   // zero-mass padding
        if constexpr (VEL) {
          if (j < j1) rv.q[l] = velj[j];
          else        rv.q[l] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
      const int e = t + l * kBlock;
      if (e < TILE) { float4 q = r[l]; q.w *= gscale; sh[buf][e] = q; }
    }
    if constexpr (VEL) {
#pragma unroll
      for (int l = 0; l < LPT; ++l) {
        const int e = t + l * kBlock;
        if (e < TILE) shv[buf][e] = rv.q[l];
      }
    }
  };

  if (ntiles > 0) { load_tile(0); store_tile(0); }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
    if constexpr (VEL) on_tile(j0 + tile * TILE, sh[buf], shv[buf], xi, yi, zi, vi.x, vi.y, vi.z, zp2, one2);
    else               on_tile(j0 + tile * TILE, sh[buf], xi, yi, zi, zp2, one2);
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }
}

// A tile's bodies a pair group at a time: group(jj, pj) — pj the bodies tile[jj .. jj + JB).
template <int NP, int TILE, class Group>
__device__ __forceinline__ void tile_groups(const float4 *tile, Group group) {
  constexpr int JB = point_group(NP);
#pragma unroll 2
  for (int jj = 0; jj < TILE; jj += JB) {
    float4 pj[JB];
#pragma unroll
    for (int b = 0; b < JB; ++b) pj[b] = tile[jj + b];
    group(jj, pj);
  }
}

// VEL: group(jj, pj, vj) — vj the same bodies' velocities.
template <int NP, int TILE, class Group>
__device__ __forceinline__ void tile_groups_v(const float4 *tile, const float4 *vtile, Group group) {
  constexpr int JB = point_group(NP);
#pragma unroll 2
  for (int jj = 0; jj < TILE; jj += JB) {
    float4 pj[JB], vj[JB];
#pragma unroll
    for (int b = 0; b < JB; ++b) { pj[b] = tile[jj + b]; vj[b] = vtile[jj + b]; }
    group(jj, pj, vj);
  }
}

// The lane's points that exist: put(p, h, at) — half h of register pair p, `at` its place in the chunk's partial row.
// (Let put capture the row's pointer by value: through a reference the compiler works its base address out again in front of every store.)
template <int NP, class Put>
__device__ __forceinline__ void point_write_out(int m, Put put) {
  const int il = blockIdx.x * (kBlock * 2 * NP) + threadIdx.x, c = blockIdx.y;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int il0 = il + (2 * p) * kBlock, il1 = il0 + kBlock;
    if (il0 < m) put(p, 0, (size_t)c * m + il0);
    if (il1 < m) put(p, 1, (size_t)c * m + il1);
  }
}

// Points in slabs whose partial rows fit the staging area (probe_slab_points(n_total, width) x j_split x width float4; the potential's
// rows are a quarter of the field's, the tidal tensor's and the jerk's twice the field's: width 2): run(NP, first, m, grid, j_split,
// j_chunk) per slab.  Which slab a point falls into, and which workgroup shape its slab gets, changes nothing it is summed from.
template <class Run>
void for_point_slabs(int n_total, int m_all, int width, Run run) {
  int j_split, j_chunk;
  probe_geometry(n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(n_total, width);
  for (size_t first = 0; first < (size_t)m_all; first += slab) {
    const int m = (int)std::min(slab, (size_t)m_all - first);
    // few points: half the points per workgroup, twice the workgroups (the same sums either way)
    const long long wgs2 = (long long)((m + 4 * kBlock - 1) / (4 * kBlock)) * j_split;
    if (wgs2 < 1024) run(std::integral_constant<int, 1>{}, first, m, dim3((m + 2 * kBlock - 1) / (2 * kBlock), j_split), j_split, j_chunk);
    else             run(std::integral_constant<int, 2>{}, first, m, dim3((m + 4 * kBlock - 1) / (4 * kBlock), j_split), j_split, j_chunk);
  }
}

}  // namespace
}  // namespace nbody
