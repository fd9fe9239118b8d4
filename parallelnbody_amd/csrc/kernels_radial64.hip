// The fp64 radial census of an fp64 state (nbody_radial_order_f64, nbody_lagrange_radii_f64; build-defined: the reference computes none
// of it): the bodies in ascending (d2, index) order about a centre, the cumulative mass in that order, and the bodies at given fractions
// of the total mass — the Lagrangian radii.  include/nbody.h states every line of it so that numpy reproduces the bits.
//
//   radial_keys_hist_f64_kernel     d2 of every body in nbody_mass_within's convention (contraction off), as a 64-bit key in body order:
//                                   the bit pattern of d2 — never negative, never -0, so the pattern orders as the value — or ~0 for a NaN;
//                                   per tile of kRxTile bodies the eight digit histograms bh_hist_reduce_kernel and bh_radix_pass_kernel
//                                   read (part_hist[tile][digit][value], stride kRxHists, digits 0 .. 7), and the tile's count of finite keys
//   the sort                        bh_hist_reduce_kernel and eight launches of bh_radix_pass_kernel (kernels_bh_sort.hip) as they are: the
//                                   passes are stable, so equal keys stay in index order and the lowest index wins every tie
//   radial_scan_f64_kernel          the masses gathered through the order (a non-finite d2 adds +0.0), summed left to right inside blocks of
//                                   256 positions: one lane walks one block in LDS — the additions are what the definition fixes, and a
//                                   sequential sum has only one arrangement —, sixteen blocks to a workgroup, loaded and stored coalesced
//   radial_scan_offsets_f64_kernel  one workgroup: the blocks' offsets, sequentially, and the tiles' finite counts added up
//   radial_scan_apply_f64_kernel    mass_cum[p] = off[p / 256] + loc[p]
//   radial_select_f64_kernel        per target f * total the first position whose cumulative mass reaches it: every workgroup's minimum
//   radial_select_fold_f64_kernel   into a slot of its own, the slots folded in order by one workgroup, which writes the rows — no atomics
#include <algorithm>

#include "../../include/nbody.h"
#include "bh_common.h"
#include "pk_common.h"

namespace nbody {

namespace {

using bh::kKhT; using bh::kRxBins; using bh::kRxHists; using bh::kRxPasses; using bh::kRxSlices; using bh::kRxT; using bh::kRxTile;

constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;    // keys below it are finite d2
constexpr int kScanBlock = 256;                                   // positions per block of the cumulative mass (include/nbody.h)
constexpr int kScanPer = 16;                                      // blocks per workgroup of radial_scan_f64_kernel
constexpr int kNone = 0x7FFFFFFF;                                 // no position qualifies

struct Fractions { double v[kRadialFractionsMax]; };

__global__ __launch_bounds__(kKhT) void radial_keys_hist_f64_kernel(const double4 *__restrict__ posm, int n, double cx, double cy, double cz,
                                                                    unsigned long long *__restrict__ key,
                                                                    unsigned int *__restrict__ part_hist,
                                                                    unsigned int *__restrict__ fin_part) {
#pragma clang fp contract(off)
  __shared__ unsigned int s_h[kRxPasses][kRxBins];
  __shared__ unsigned int s_fin[kKhT / 64];
  const int t = threadIdx.x;
  for (int q = t; q < kRxPasses * kRxBins; q += kKhT) (&s_h[0][0])[q] = 0u;
  __syncthreads();
  unsigned int fin = 0u;
#pragma unroll
  for (int r = 0; r < kRxTile / kKhT; ++r) {
    const int i = blockIdx.x * kRxTile + r * kKhT + t;
    if (i < n) {
      const double4 p = posm[i];
      const double dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;             // nbody_mass_within's d2, operation by operation
      const unsigned long long k = d2 != d2 ? ~0ull : (unsigned long long)__double_as_longlong(d2);
      key[i] = k;
      fin += k < kInfBits ? 1u : 0u;
#pragma unroll
      for (int d = 0; d < kRxPasses; ++d) atomicAdd(&s_h[d][(k >> (8 * d)) & 0xFFull], 1u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) fin += __shfl_xor(fin, off, 64);
  if ((t & 63) == 0) s_fin[t >> 6] = fin;
  __syncthreads();
  unsigned int *out = part_hist + (size_t)blockIdx.x * (kRxHists * kRxBins);   // (the second word's eight histograms are never read)
  for (int q = t; q < kRxPasses * kRxBins; q += kKhT) out[q] = (&s_h[0][0])[q];
  if (t == 0) {
    unsigned int c = 0u;
#pragma unroll
    for (int w = 0; w < kKhT / 64; ++w) c += s_fin[w];
    fin_part[blockIdx.x] = c;
  }
}

// loc[p] = ((w_0 + w_1) + ...) + w_t inside block p / 256 (t = p % 256), blk_sum[b] = loc of the block's last entry — a short last block
// is padded with +0.0.  Lane b of a workgroup walks block 16 blockIdx.x + b; the rows are padded by one double, so the sixteen lanes
// read sixteen different banks.
__global__ __launch_bounds__(kBlock) void radial_scan_f64_kernel(const double4 *__restrict__ posm, const unsigned long long *__restrict__ key,
                                                                 const unsigned int *__restrict__ order, int n, double *__restrict__ loc,
                                                                 double *__restrict__ blk_sum) {
  static_assert(kScanBlock == kBlock, "a lane loads one entry per block");
  __shared__ double s_w[kScanPer][kScanBlock + 1];
  const int t = threadIdx.x;
  const int base = blockIdx.x * (kScanPer * kScanBlock);
#pragma unroll
  for (int r = 0; r < kScanPer; ++r) {
    const int p = base + r * kScanBlock + t;
    double w = 0.0;
    if (p < n && key[p] < kInfBits) w = posm[order[p]].w;
    s_w[r][t] = w;
  }
  __syncthreads();
  if (t < kScanPer && base + t * kScanBlock < n) {
    double acc = 0.0;
    for (int j0 = 0; j0 < kScanBlock; j0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = s_w[t][j0 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) { acc = (j0 + u == 0) ? v[u] : acc + v[u]; v[u] = acc; }   // (the first entry is taken, not added to 0)
#pragma unroll
      for (int u = 0; u < 8; ++u) s_w[t][j0 + u] = v[u];
    }
    blk_sum[blockIdx.x * kScanPer + t] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kScanPer; ++r) {
    const int p = base + r * kScanBlock + t;
    if (p < n) loc[p] = s_w[r][t];
  }
}

// off[0] = 0.0, off[b + 1] = off[b] + blk_sum[b]: thread 0, 256 blocks at a time through LDS; *n_finite = the tiles' finite counts
__global__ __launch_bounds__(kBlock) void radial_scan_offsets_f64_kernel(const double *__restrict__ blk_sum, int nblk, double *__restrict__ off,
                                                                         const unsigned int *__restrict__ fin_part, int tiles,
                                                                         int *__restrict__ n_finite) {
  __shared__ double s_b[kBlock];
  __shared__ unsigned int s_c[kBlock / 64];
  const int t = threadIdx.x;
  unsigned int c = 0u;
  for (int q = t; q < tiles; q += kBlock) c += fin_part[q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((t & 63) == 0) s_c[t >> 6] = c;
  double acc = 0.0;
  for (int b0 = 0; b0 < nblk; b0 += kBlock) {
    s_b[t] = b0 + t < nblk ? blk_sum[b0 + t] : 0.0;
    __syncthreads();
    if (t == 0) {
      for (int j0 = 0; j0 < kBlock; j0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s_b[j0 + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const double before = acc; acc += v[u]; v[u] = before; }
#pragma unroll
        for (int u = 0; u < 8; ++u) s_b[j0 + u] = v[u];
      }
    }
    __syncthreads();
    if (b0 + t < nblk) off[b0 + t] = s_b[t];
    __syncthreads();                                               // (s_b is the next round's)
  }
  if (t == 0) *n_finite = (int)(((s_c[0] + s_c[1]) + s_c[2]) + s_c[3]);   // (written before the first barrier; nblk >= 1)
}

__global__ __launch_bounds__(kBlock) void radial_scan_apply_f64_kernel(const double *__restrict__ off, int n, double *__restrict__ cum) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p < n) cum[p] = off[p / kScanBlock] + cum[p];
}

// part[workgroup][q] = the first position p of the workgroup's run [blockIdx.x per, ...) with mass_cum[p] >= F.v[q] * total (one
// multiply), kNone where there is none; total = mass_cum[n - 1].  Nothing qualifies unless total > 0 (a NaN target compares false).
__global__ __launch_bounds__(kBlock) void radial_select_f64_kernel(const double *__restrict__ cum, int n, int per, Fractions F, int k,
                                                                   int *__restrict__ part) {
  __shared__ double s_tgt[kRadialFractionsMax];
  __shared__ int s_red[kBlock / 64][kRadialFractionsMax];
  const int t = threadIdx.x;
  const double total = cum[n - 1];
  if (t < kRadialFractionsMax) s_tgt[t] = (t < k && total > 0.0) ? F.v[t] * total : __longlong_as_double(0x7FF8000000000000ll);
  __syncthreads();
  const long long lo64 = (long long)blockIdx.x * per;
  const int lo = (int)lo64, hi = (int)min(lo64 + per, (long long)n);
  int best[kRadialFractionsMax];
#pragma unroll
  for (int q = 0; q < kRadialFractionsMax; ++q) best[q] = kNone;
  for (int p = lo + t; p < hi; p += kBlock) {
    const double m = cum[p];
#pragma unroll
    for (int q = 0; q < kRadialFractionsMax; ++q)
      if (q < k) best[q] = (m >= s_tgt[q] && p < best[q]) ? p : best[q];   // (uniform: k is a kernel argument)
  }
#pragma unroll
  for (int q = 0; q < kRadialFractionsMax; ++q) {
    if (q < k) {
      int b = best[q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) b = min(b, __shfl_xor(b, off, 64));
      if ((t & 63) == 0) s_red[t >> 6][q] = b;
    }
  }
  __syncthreads();
  if (t < k) {
    int b = s_red[0][t];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) b = min(b, s_red[w][t]);
    part[(size_t)blockIdx.x * kRadialFractionsMax + t] = b;
  }
}

// One workgroup: wave w folds the slots of the fractions w, w + 4, ... (lane l the slots l, l + 64, ... in order, the shuffle tree joins
// the lanes) and writes the row; *total_out = mass_cum[n - 1]
__global__ __launch_bounds__(kBlock) void radial_select_fold_f64_kernel(const int *__restrict__ part, int slots, Fractions F, int k,
                                                                        const unsigned long long *__restrict__ key,
                                                                        const unsigned int *__restrict__ order,
                                                                        const double *__restrict__ cum, int n,
                                                                        nbody_lagrange *__restrict__ rows, double *__restrict__ total_out) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) *total_out = cum[n - 1];
  for (int q = threadIdx.x >> 6; q < k; q += kBlock / 64) {
    int p = kNone;
    for (int s = lane; s < slots; s += 64) p = min(p, part[(size_t)s * kRadialFractionsMax + q]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p = min(p, __shfl_xor(p, off, 64));
    if (lane == 0) {
      nbody_lagrange r;
      const double nan = __longlong_as_double(0x7FF8000000000000ll);
      r.fraction = F.v[q];
      if (p == kNone) { r.r2 = nan; r.radius = nan; r.mass = nan; r.body = -1; r.count = 0; }
      else {
        r.r2 = __longlong_as_double((long long)key[p]);
        r.radius = sqrt(r.r2);                                     // the correctly rounded fp64 root
        r.mass = cum[p]; r.body = (int)order[p]; r.count = p + 1;
      }
      rows[q] = r;
    }
  }
}

}  // namespace

Radial64Work radial64_work(int n) {
  Radial64Work W;
  const size_t N = (size_t)(n > 0 ? n : 1), tiles = (N + kRxTile - 1) / kRxTile, nblk = tiles * kScanPer;
  int slots, per;
  moments_geometry((int)N, &slots, &per);
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
  W.key[0] = take(N * 8); W.key[1] = take(N * 8);
  W.idx[0] = take(N * 4); W.idx[1] = take(N * 4);
  W.cum = take(N * 8);
  W.part_hist = take(tiles * kRxHists * kRxBins * 4);
  W.slice_hist = take((size_t)kRxSlices * kRxHists * kRxBins * 4);
  W.blk_sum = take(nblk * 8); W.off = take(nblk * 8);
  W.fin_part = take(tiles * 4);
  W.sel_part = take((size_t)slots * kRadialFractionsMax * 4);
  W.rows = take(kRadialFractionsMax * sizeof(nbody_lagrange));
  W.total = take(8); W.n_finite = take(4);
  // what is cleared before the first pass, side by side: the look-back words of all eight passes and the status word the passes read
  W.desc = take(tiles * kRxPasses * kRxBins * 4);
  W.status = take(4);
  W.clear_bytes = at - W.desc;
  W.bytes = at;
  return W;
}

hipError_t radial64_resident(int *resident) { return bh::radix_pass_resident(resident); }

hipError_t launch_radial_f64(const Radial64Launch &L, hipStream_t s) {
  const int n = L.n_total;
  if (n < 1 || !L.posm || !L.work || L.resident < 1 || L.k < 0 || L.k > kRadialFractionsMax) return hipErrorInvalidValue;
  const Radial64Work W = radial64_work(n);
  char *base = (char *)L.work;
  unsigned long long *key[2] = {(unsigned long long *)(base + W.key[0]), (unsigned long long *)(base + W.key[1])};
  unsigned int *idx[2] = {(unsigned int *)(base + W.idx[0]), (unsigned int *)(base + W.idx[1])};
  unsigned int *part_hist = (unsigned int *)(base + W.part_hist), *slice_hist = (unsigned int *)(base + W.slice_hist);
  unsigned int *desc = (unsigned int *)(base + W.desc), *fin_part = (unsigned int *)(base + W.fin_part);
  double *cum = (double *)(base + W.cum), *blk_sum = (double *)(base + W.blk_sum), *off = (double *)(base + W.off);
  const int tiles = (n + kRxTile - 1) / kRxTile, nblk = (n + kScanBlock - 1) / kScanBlock;
  auto mark = [&](int q) { return L.events ? hipEventRecord(L.events[q], s) : hipSuccess; };

  if (hipError_t e = mark(0)) return e;
  if (hipError_t e = hipMemsetAsync(desc, 0, W.clear_bytes, s)) return e;
  hipLaunchKernelGGL(radial_keys_hist_f64_kernel, dim3(tiles), dim3(kKhT), 0, s, (const double4 *)L.posm, n, L.centre[0], L.centre[1],
                     L.centre[2], key[0], part_hist, fin_part);
  if (hipError_t e = mark(1)) return e;
  hipLaunchKernelGGL(bh::bh_hist_reduce_kernel, dim3(kRxPasses, kRxSlices), dim3(kRxBins), 0, s, part_hist, tiles, slice_hist);
  // bh_radix_pass_kernel's workgroups wait for earlier tiles' look-back words: every workgroup of a pass must be resident at once, or
  // the launch hangs (the kernel's own comment, and bh_large_frame's pass_grid) — never more workgroups than radix_pass_resident says
  const int pass_grid = std::min(tiles, L.resident);
  for (int d = 0; d < kRxPasses; ++d) {                            // key[0] -> key[1] / idx[1] -> key[0] / idx[0] -> ... -> key[0] / idx[0]
    bh::RadixPass P;
    P.kin = key[d & 1]; P.vin = d == 0 ? nullptr : idx[d & 1];
    P.kout = key[(d & 1) ^ 1]; P.vout = idx[(d & 1) ^ 1];
    P.slice_hist = slice_hist; P.digit = d;
    P.desc = desc + (size_t)d * tiles * kRxBins;
    P.shift = 8 * d; P.n = n; P.status = (const int *)(base + W.status);
    hipLaunchKernelGGL(bh::bh_radix_pass_kernel, dim3(pass_grid), dim3(kRxT), 0, s, P);
  }
  if (hipError_t e = mark(2)) return e;
  hipLaunchKernelGGL(radial_scan_f64_kernel, dim3(tiles), dim3(kBlock), 0, s, (const double4 *)L.posm, key[0], idx[0], n, cum, blk_sum);
  hipLaunchKernelGGL(radial_scan_offsets_f64_kernel, dim3(1), dim3(kBlock), 0, s, blk_sum, nblk, off, fin_part, tiles,
                     (int *)(base + W.n_finite));
  hipLaunchKernelGGL(radial_scan_apply_f64_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, off, n, cum);
  if (hipError_t e = mark(3)) return e;
  if (L.k > 0) {
    int slots, per;
    moments_geometry(n, &slots, &per);
    Fractions F;
    for (int q = 0; q < kRadialFractionsMax; ++q) F.v[q] = q < L.k ? L.fractions[q] : 0.0;
    int *sel_part = (int *)(base + W.sel_part);
    hipLaunchKernelGGL(radial_select_f64_kernel, dim3(slots), dim3(kBlock), 0, s, cum, n, per, F, L.k, sel_part);
    hipLaunchKernelGGL(radial_select_fold_f64_kernel, dim3(1), dim3(kBlock), 0, s, sel_part, slots, F, L.k, key[0], idx[0], cum, n,
                       (nbody_lagrange *)(base + W.rows), (double *)(base + W.total));
  }
  if (hipError_t e = mark(4)) return e;
  return hipGetLastError();
}

}  // namespace nbody
