// The bodies' field at points that are not bodies (nbody_field_at, the tracers of nbody_set_tracers) at theta = 0:
//   probe_tile_pk_kernel  <- the pair law OctreeSearch.h:101-104 of a massless point against every body, i.e. the loop
//                            OctreeSearch.cpp:83-86 with the i side taken from another array
//   probe_fold_kernel     <- the chunks' partial rows added in chunk order and, for tracers, OctreeSearch.cpp:29-30 (v += dt*a; x += dt*v)
// The theta > 0 counterpart — the walk of the last tree from a point — is bh_probe_walk_kernel (kernels_bh_walk.hip).
#include "kernels.h"

#include <algorithm>
#include <type_traits>

#include "../../include/nbody.h"
#include "pk_common.h"
#include "tracer_update.h"

namespace nbody {

namespace {

// forces_tile_pk_kernel (kernels.hip) with the i-bodies from `probe` [m] instead of posm: lanes hold their points two by two in
// register pairs, the bodies go through double-buffered LDS tiles as (x, y, z, G m), every constant in a VGPR.
//   grid.x : blocks of kBlock * 2 NP points (lane t holds points base + t + k * kBlock: coalesced)
//   grid.y : j chunks [c * j_chunk, min((c + 1) * j_chunk, n_total)); each writes its own partial row part[c][m]
// A point may sit on a body anywhere, so every tile runs the guarded law (there is no "own range" and no bare pass); ragged tiles
// are padded with zero-mass bodies on the origin, which every ZMODE here keeps out of the sum.  A point's sum over a chunk is one
// chain of fused multiply-adds in body order whatever NP is and wherever the point stands in the array.
template <int NP, int TILE, int ZMODE>
__global__ __launch_bounds__(kBlock) void probe_tile_pk_kernel(const float4 *__restrict__ posm, const float4 *__restrict__ probe,
                                                               float4 *__restrict__ part, int n_total, int m, int j_chunk,
                                                               float gscale, float zp, unsigned long long *__restrict__ clk) {
  constexpr int IPT = 2 * NP;
  constexpr int LPT = (TILE + kBlock - 1) / kBlock;
  const ClockStamp stamp = clock_begin(clk);
  __shared__ float4 sh[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  f2 xi[NP], yi[NP], zi[NP];
  Acc3pk<false> a[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float4 p0 = probe[min(ibase + t + (2 * p) * kBlock, m - 1)];
    const float4 p1 = probe[min(ibase + t + (2 * p + 1) * kBlock, m - 1)];
    xi[p] = f2{p0.x, p1.x}; yi[p] = f2{p0.y, p1.y}; zi[p] = f2{p0.z, p1.z};
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

  if (ntiles > 0) { load_tile(0); store_tile(0); }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
    constexpr int JB = (NP == 1) ? 4 : 2;
#pragma unroll 2
    for (int jj = 0; jj < TILE; jj += JB) {
      float4 pj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) pj[b] = sh[buf][jj + b];
      pair_group_pk<NP, JB, ZMODE, false, false>(xi, yi, zi, pj, zp2, one2, a);
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int il0 = ibase + t + (2 * p) * kBlock, il1 = il0 + kBlock;
    if (il0 < m) part[(size_t)c * m + il0] = make_float4(a[p].x.x, a[p].y.x, a[p].z.x, 0.f);
    if (il1 < m) part[(size_t)c * m + il1] = make_float4(a[p].x.y, a[p].y.y, a[p].z.y, 0.f);
  }
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

constexpr int kProbeTile = 256;

template <int NP>
void launch_probe_np(const ProbeLaunch &L, int m, const float4 *probe, float4 *part, int j_split, int j_chunk, hipStream_t s) {
  const dim3 grid((m + kBlock * 2 * NP - 1) / (kBlock * 2 * NP), j_split), block(kBlock);
  if (L.eps2 > 0.0)
    hipLaunchKernelGGL((probe_tile_pk_kernel<NP, kProbeTile, Z_SOFT>), grid, block, 0, s, (const float4 *)L.posm, probe, part, L.n_total, m,
                       j_chunk, (float)L.G, (float)L.eps2, (unsigned long long *)L.clk);
  else
    hipLaunchKernelGGL((probe_tile_pk_kernel<NP, kProbeTile, Z_CLAMP>), grid, block, 0, s, (const float4 *)L.posm, probe, part, L.n_total, m,
                       j_chunk, (float)L.G, -0x1p126f, (unsigned long long *)L.clk);
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

size_t probe_slab_points(int n_total) {
  int js, jc;
  probe_geometry(n_total, &js, &jc);
  const size_t pts = kProbePartBytes / ((size_t)js * sizeof(float4));
  return std::max<size_t>(1024, pts / 1024 * 1024);
}

// Points in slabs whose partial rows fit the staging area (L.part: probe_slab_points(n_total) x j_split float4); which slab a
// point falls into changes nothing it is summed from.
hipError_t launch_probe(const ProbeLaunch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.probe || !L.part || !L.acc) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total);
  const int integrate = L.dt > 0.0f ? 1 : 0;
  if (integrate && (!L.vel || !L.pos_out)) return hipErrorInvalidValue;
  for (size_t first = 0; first < (size_t)L.m; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.m - first);
    const float4 *probe = (const float4 *)L.probe + first;
    // few points: half the points per workgroup, twice the workgroups (the same sums either way)
    const long long wgs2 = (long long)((m + 4 * kBlock - 1) / (4 * kBlock)) * j_split;
    if (wgs2 < 1024) launch_probe_np<1>(L, m, probe, (float4 *)L.part, j_split, j_chunk, s);
    else             launch_probe_np<2>(L, m, probe, (float4 *)L.part, j_split, j_chunk, s);
    hipLaunchKernelGGL(probe_fold_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const float4 *)L.part, m, j_split,
                       (float4 *)L.acc + first, integrate ? (float4 *)L.pos_out + first : nullptr,
                       integrate ? (float4 *)L.vel + first : nullptr, L.dt, integrate);
  }
  return hipGetLastError();
}

}  // namespace nbody
