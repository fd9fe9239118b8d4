// The fp64 separation census of an fp64 state (nbody_get_pair_counts_f64, nbody_pair_counts_at_f64; build-defined: the reference computes
// none of it): how many pairs lie within r, for kPairs64Group radii in one N^2 pass.  For a row at x and body j, with d = x_j - x and
// contraction OFF:
//     d2 = (dx*dx + dy*dy) + dz*dz          the group census's expression in every operation
//     counted at threshold t iff d2 <= t    t = radius * radius, one fp64 multiply on the host
//   pairs_tile_f64_kernel<., G, SELF = true>    <- the rows are the bodies (i_first + il of posm): the ORDERED pairs i != j BY INDEX
//   pairs_tile_f64_kernel<., G, SELF = false>   <- the rows are caller points (ipos[il]); NO body is dropped by index
// A row scan (scan_tile64.h) and a sibling of groups_tile_f64_kernel<., MIN = false, COUNT = true, .>: its grid, chunks, double-buffered
// tiles, kJerk64Jb bodies at a time in ascending j, rows in registers.  What differs is what happens to d2.  There is NO per-row
// result, so nothing is kept per lane: the G thresholds are kernel arguments (wave-uniform, SGPRs), and for every vector of 64 d2 the
// WAVE counts on its scalar pipe — v_cmp_le_f64 into an SGPR pair, s_bcnt1_i32_b64, s_add_i32 —
//     cnt[q] += popcount(ballot(d2 <= t[q]))
// with the thresholds ASCENDING in q and visited from the largest down: once a mask is empty every smaller threshold's mask is empty
// too, and the wave leaves the chain (a wave-uniform branch).  No VGPR per threshold, no LDS, no atomics in the loop.  A launch of
// k < G thresholds has them in t[G - k .. G) and -1 below: no d2 is <= -1, so the chain ends there and k thresholds cost k + 1 compares
// at most.
//
// What must not count costs no per-pair work:
//   * the lanes past m, which repeat row m - 1:   their row's x is a NaN — every d2 of theirs is NaN and fails <=
//   * the padding of a chunk's last tile:         staged as NaNs here (not as zeros on the origin), the same way
//   * SELF, the pair (i, i):                      it is COUNTED in the loop and taken off at the end.  d2_ii is computed from x_i - x_i:
//     0 where the three coordinates are finite — and 0 <= t for every valid t —, NaN otherwise.  So the wave's rows that lie in this
//     chunk and have d2_ii == 0, one popcount per row vector ahead of the loop, is what every counter holds too much.
// A NaN d2 never counts, a +inf d2 never passes a finite t, a zero-mass body counts.
//
// A wave's counters are 32-bit and cannot wrap: a wave holds 64 * IPT <= 128 rows and a chunk at most n_total / 128 + kJerkTile bodies
// (probe_geometry), so a counter ends at most at n_total + 128 * kJerkTile <= 2^31 + 2^15 < 2^32 for every int32 n_total.  At the end
// the four waves' counters meet in LDS and the workgroup writes its G 64-bit totals into a slot of its own (partial[block][G]: no atomics
// in the tile kernel at all — one atomicAdd per wave and threshold was measured first, and at N = 65536, where a pass is 1.3 ms, a
// million adds onto sixteen words tripled it); pairs_fold_f64_kernel adds the slots up, at most kPairs64FoldBlocks workgroups, each
// ending in one 64-bit integer atomicAdd per threshold into count[].  Integer sums do not depend on the order: the same bytes every
// run.  No scratch, no fp atomics.
#include "kernels.h"

#include "scan_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

template <int G>
struct PairThresholds { double t[G]; };   // ascending; t[0 .. skip) = -1: no d2 is <= it

// local row il = blockIdx.x * (kBlock * IPT) + t + k * kBlock is
// SELF: body i_first + il of ipos (== posm);  else: point il of ipos — against the bodies of chunk blockIdx.y.  The workgroup's totals
// go to partial[(blockIdx.y * gridDim.x + blockIdx.x) * G + q].
template <int IPT, int G, bool SELF>
__global__ __launch_bounds__(kBlock) void pairs_tile_f64_kernel(const double4 *__restrict__ posm, const double4 *__restrict__ ipos,
                                                                unsigned long long *__restrict__ partial, int n_total, int m, int i_first,
                                                                int j_chunk, PairThresholds<G> th) {
  constexpr int JB = kJerk64Jb, TILE = kJerkTile;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  __shared__ double4 shp[2][TILE];
  __shared__ unsigned red[kBlock / 64][G];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  double xi[IPT], yi[IPT], zi[IPT];
  unsigned own = 0;                                                // SELF: the wave's pairs (i, i) the loop will count under every threshold
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    const int self = i_first + min(il, m - 1);                    // (the points' i_first is 0: the index into ipos)
    const double4 p = ipos[self];
    xi[k] = il < m ? p.x : nan; yi[k] = p.y; zi[k] = p.z;         // a repeated row counts nowhere
    if (SELF) {
      const double dx = p.x - xi[k], dy = p.y - yi[k], dz = p.z - zi[k];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      own += (unsigned)__popcll(__ballot(self >= j0 && self < j1 && d2 == 0.0));
    }
  }

  unsigned cnt[G];
#pragma unroll
  for (int q = 0; q < G; ++q) cnt[q] = 0;

  double4 rp;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) rp = posm[j];
    else        rp = make_double4(nan, nan, nan, 0.0);             // padding: never counted
  };

  if (ntiles > 0) { load_tile(0); shp[0][t] = rp; }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
#pragma unroll 2
    for (int jj = 0; jj < TILE; jj += JB) {
      double4 pj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) pj[b] = shp[buf][jj + b];
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double dx = pj[b].x - xi[k], dy = pj[b].y - yi[k], dz = pj[b].z - zi[k];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
#pragma unroll
          for (int q = G - 1; q >= 0; --q) {
            const unsigned long long in = __ballot(d2 <= th.t[q]);
            if (in == 0) break;                                    // wave-uniform: no smaller threshold holds a lane either
            cnt[q] += (unsigned)__popcll(in);
          }
        }
    }
    if (more) shp[buf ^ 1][t] = rp;
    __syncthreads();
  }

  if ((t & 63) == 0) {
#pragma unroll
    for (int q = 0; q < G; ++q) red[t >> 6][q] = cnt[q] > own ? cnt[q] - own : 0;   // (own <= cnt[q] wherever threshold q is >= 0: every
  }                                                                                  // one of those pairs passed it; an unused counter is 0)
  __syncthreads();
  if (t < G) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) sum += red[w][t];
    partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * G + t] = sum;
  }
}

// count[q - skip] += the sum over the nparts slots of partial[.][q], for the thresholds q >= skip: thread t takes threshold t % G of the
// slots blockIdx.x * (kBlock / G) + t / G, ... (coalesced), the workgroup's sums meet in LDS, one integer atomicAdd per threshold
constexpr int kPairs64FoldBlocks = 64;
template <int G>
__global__ __launch_bounds__(kBlock) void pairs_fold_f64_kernel(const unsigned long long *__restrict__ partial, int nparts, int skip,
                                                                unsigned long long *__restrict__ count) {
  static_assert(kBlock % G == 0, "a workgroup takes whole slots");
  __shared__ unsigned long long red[kBlock];
  const int t = threadIdx.x, q = t % G;
  unsigned long long sum = 0;
  for (int r = blockIdx.x * (kBlock / G) + t / G; r < nparts; r += gridDim.x * (kBlock / G)) sum += partial[(size_t)r * G + q];
  red[t] = sum;
  __syncthreads();
  if (t < G) {
    for (int k = G; k < kBlock; k += G) sum += red[t + k];
    if (q >= skip && sum) atomicAdd(&count[q - skip], sum);
  }
}

bool bad(const Pairs64Launch &L) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.count || !L.partial || L.k < 1 || L.k > kPairs64Group) return true;
  if (L.partial_words < pairs64_partial_words(L.n_total, L.m, L.ppos == nullptr, L.lanes)) return true;
  for (int q = 0; q < L.k; ++q)
    if (!(L.r2[q] >= 0.0) || !(L.r2[q] < HUGE_VAL) || (q > 0 && L.r2[q] < L.r2[q - 1])) return true;
  return false;
}

}  // namespace

size_t pairs64_partial_words(int n_total, int m, bool self, int lanes) {
  size_t words = 0;
  if (n_total > 0 && m > 0)
    for_row_slabs64(n_total, m, kPairs64Width, self, lanes, [&](const RowSlab64 &b) {
      words = std::max(words, (size_t)b.grid.x * b.grid.y * kPairs64Group);
    });
  return words;
}

// the pass over the slabs, every slab adding into count[] — over the bodies or, ppos given, over the points; nothing is launched where an
// argument is missing, a threshold is not finite and >= 0, they do not ascend, or the bodies' form is asked for other than all bodies
hipError_t launch_pair_counts_f64(const Pairs64Launch &L, hipStream_t s) {
  const bool self = L.ppos == nullptr;
  if (bad(L) || (self && L.m != L.n_total)) return hipErrorInvalidValue;
  constexpr int G = kPairs64Group;
  const double4 *posm = (const double4 *)L.posm;
  PairThresholds<G> th;
  const int skip = G - L.k;
  for (int q = 0; q < G; ++q) th.t[q] = q < skip ? -1.0 : L.r2[q - skip];
  for_row_slabs64(L.n_total, L.m, kPairs64Width, self, L.lanes, [&](const RowSlab64 &b) {
    if (self) {
      hipLaunchKernelGGL((pairs_tile_f64_kernel<kScan64Ipt, G, true>), b.grid, dim3(kBlock), 0, s, posm, posm, L.partial, L.n_total, b.m,
                         (int)b.first, b.j_chunk, th);
    } else {
      auto kernel = b.ipt == 2 ? pairs_tile_f64_kernel<2, G, false> : pairs_tile_f64_kernel<1, G, false>;
      hipLaunchKernelGGL(kernel, b.grid, dim3(kBlock), 0, s, posm, (const double4 *)L.ppos + b.first, L.partial, L.n_total, b.m, 0,
                         b.j_chunk, th);
    }
    const int nparts = (int)(b.grid.x * b.grid.y);
    const int fold = std::min(kPairs64FoldBlocks, (nparts + kBlock / G - 1) / (kBlock / G));
    hipLaunchKernelGGL(pairs_fold_f64_kernel<G>, dim3(fold), dim3(kBlock), 0, s, (const unsigned long long *)L.partial, nparts, skip, L.count);
  });
  return hipGetLastError();
}

}  // namespace nbody
