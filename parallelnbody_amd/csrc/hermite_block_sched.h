// The scheduler of the Hermite block time steps, written once for both orders (kernels_hermite_block.hip): the workgroup reductions of
// the segment kernels and the list kernels' whole body but the predictor — integers only, so nothing here depends on an order.
#pragma once
#include "kernels.h"
#include "pk_common.h"

namespace nbody {
namespace {

constexpr long long kNever = 0x7fffffffffffffffll;

__device__ __forceinline__ long long block_min_workgroup(long long v, long long (&red)[kBlock / 64]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  __syncthreads();                                                 // (red may still be read from the reduction before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = red[0];
  for (int w = 1; w < kBlock / 64; ++w) r = red[w] < r ? red[w] : r;
  return r;
}
__device__ __forceinline__ int block_sum_workgroup(int v, int (&red)[kBlock / 64]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
  for (int w = 1; w < kBlock / 64; ++w) r += red[w];
  return r;
}

// What a list kernel does, one workgroup per segment s = bodies [s seg_len, min(n, (s + 1) seg_len)): T_next = the smallest seg_min — JOINT:
// of BOTH sets of a session that carries tracers, this set's segments and the other's (other_min[0 .. other_slots)) —; record[0] = T_next,
// record[1] = m, the bodies of this set due at T_next (0 and an empty list where nobody is); list[0 .. m) those bodies in ascending index —
// a segment's place from the counts of the segments before it, a body's place in its segment by a ballot scan: no atomics, no order of
// arrival —; and predict(i, dt) for EVERY body i of the segment, dt = (double)(T_next - T[i]) tick: the order's predictor, the one thing
// the two list kernels do not share.
template <bool JOINT, class Predict>
__device__ __forceinline__ void hermite_block_list(const long long *__restrict__ T, const int *__restrict__ level,
                                                   const long long *__restrict__ seg_min, const int *__restrict__ seg_cnt, int slots, int n,
                                                   int seg_len, int levels, double tick, int *__restrict__ list,
                                                   long long *__restrict__ record, const long long *__restrict__ other_min,
                                                   int other_slots, Predict predict) {
  __shared__ long long redl[kBlock / 64];
  __shared__ int redi[kBlock / 64], wave_cnt[kBlock / 64];
  const int t = threadIdx.x, s = blockIdx.x;
  long long tn = kNever;
  for (int q = t; q < slots; q += kBlock) tn = seg_min[q] < tn ? seg_min[q] : tn;
  if (JOINT)
    for (int q = t; q < other_slots; q += kBlock) tn = other_min[q] < tn ? other_min[q] : tn;
  tn = block_min_workgroup(tn, redl);
  int before = 0, total = 0;
  for (int q = t; q < slots; q += kBlock) {
    const int c = seg_min[q] == tn ? seg_cnt[q] : 0;
    total += c;
    before += q < s ? c : 0;
  }
  before = block_sum_workgroup(before, redi);
  total = block_sum_workgroup(total, redi);
  if (s == 0 && t == 0) { record[0] = tn; record[1] = (long long)total; }

  const int b0 = min(n, s * seg_len), b1 = min(n, b0 + seg_len);
  int base = before;
  for (int i0 = b0; i0 < b1; i0 += kBlock) {                        // (uniform over the workgroup)
    const int i = i0 + t;
    bool act = false;
    if (i < b1) {
      const long long Ti = T[i];
      act = Ti + (1ll << (levels - level[i])) == tn;
      predict(i, (double)(tn - Ti) * tick);
    }
    const unsigned long long votes = __ballot(act);
    const int lane = t & 63, w = t >> 6;
    const int rank = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[w] = __popcll(votes);
    __syncthreads();
    int off = 0, all = 0;
    for (int q = 0; q < kBlock / 64; ++q) { off += q < w ? wave_cnt[q] : 0; all += wave_cnt[q]; }
    if (act) list[base + off + rank] = i;                          // base + off + rank < the count the next-kernel took: <= n
    base += all;
    __syncthreads();
  }
}

}  // namespace
}  // namespace nbody
