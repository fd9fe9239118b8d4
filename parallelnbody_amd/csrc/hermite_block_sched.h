// What the schedulers of the Hermite block time steps share (kernels_hermite_block.hip, kernels_hermite6_block.hip): the workgroup
// reductions of the segment kernels — integers only, so nothing here depends on an order.
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

}  // namespace
}  // namespace nbody
