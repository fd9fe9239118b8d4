// The gravitational potential from the walk of Octree::ComputeForces (OctreeSearch.h:99-108) over the last tree built
// (nbody_potential_at, nbody_get_potentials, nbody_energy_fast at theta > 0; build-defined: the reference computes no potential).
// The walk is bh_probe_walk_kernel's (kernels_bh_walk.hip), restated: the same opening test on the unsoftened d2, the same leaf rule,
// d == 0 ends the subtree; what an accepted node adds is the potential's term instead of the force's.
#include "bh_common.h"

namespace nbody {
namespace bh {

// One accepted node's term: G * (double)M / (double)ds, ds = sqrtf(d2 + eps2) correctly rounded (SOFT: the add is one fp32 add, not
// fused; false: eps2 is not read), the division a correctly rounded double division — what plain C computes with contraction off.
// The fast path is force_term's (kernels_bh_walk.hip): v_sqrt_f32 put right by the two fused residuals, and the compiler's own
// division sequence — reciprocal, two Newton steps, quotient, one residual step — without the operand scaling and the special cases that
// cannot occur: ds in [2^-48, 2^64), G M finite, so every value on the way is a normal double (a mass of +-0 gives +0 where the
// division gives the mass's sign: a term of +-0 either way, which changes no sum that started at +0).  A wave with an argument below
// 2^-96, an infinite / NaN one or a mass that is not finite in any of its lanes takes sqrtf and the division themselves.
template <bool SOFT>
__device__ __forceinline__ double pot_term(float d2, float M, double G, float eps2) {
#pragma clang fp contract(off)
  if constexpr (SOFT) d2 = d2 + eps2;                          // ds2 (d2 is never -0)
  if (__any(!(d2 >= 0x1p-96f) || d2 == __builtin_inff() || !(fabsf(M) <= 0x1.fffffep127f))) {
    const float d = sqrtf(d2);
    return G * (double)M / (double)d;
  }
  const float r = __builtin_amdgcn_sqrtf(d2);
  const float below = __uint_as_float(__float_as_uint(r) - 1u), above = __uint_as_float(__float_as_uint(r) + 1u);
  const float eb = __builtin_fmaf(-below, r, d2), ea = __builtin_fmaf(-above, r, d2);
  float d = eb <= 0.0f ? below : r;
  d = ea > 0.0f ? above : d;
  const double den = (double)d, num = G * (double)M;
  double rc = __builtin_amdgcn_rcp(den);
  rc = __builtin_fma(rc, __builtin_fma(-den, rc, 1.0), rc);
  rc = __builtin_fma(rc, __builtin_fma(-den, rc, 1.0), rc);
  const double q0 = num * rc;
  return __builtin_fma(__builtin_fma(-den, q0, num), rc, q0);
}

// One lane per point (BODY = false: pts[k], results at k) or per body (BODY = true: the body at sorted position k — neighbours in space
// walk side by side —, its position from posm, results at the body's index) over the tree the last frame left in its global arrays.
// HOP: the tree carries hop words and a step is the lane walk's own — the next node asked for before the term is worked out —;
// otherwise the plain loop on the node words and the levels' thresholds.  One fp64 accumulator, added to in walk order; phi = -sum.
// The kernel reads the frame's verdict and does nothing unless it is 0; it neither writes the verdict nor touches the tree.
template <bool HOP, bool SOFT, bool BODY>
__global__ __launch_bounds__(kB) void bh_pot_walk_kernel(SmallTree T, const float4 *__restrict__ pts, double *__restrict__ phi64,
                                                         float *__restrict__ phif, int m, double G, float eps2) {
#pragma clang fp contract(off)
  const int k = (BODY ? xcd_run_block() : (int)blockIdx.x) * kB + threadIdx.x;
  const bool valid = k < m;
  const int status = T.hdr[3], nodes_all = T.hdr[0];
  if (status != 0) return;
  const int nodes = valid ? nodes_all : 0;
  const int at = BODY ? (valid ? (int)T.sidx[k] : 0) : (valid ? k : 0);
  const float4 p = pts[at];
  double sum = 0.0;
  int node = 0;
  if constexpr (HOP) {
    float4 cm = T.com[0];
    uint2 h = T.hop[0];
    while (node < nodes) {
      const float ex = p.x - cm.x, ey = p.y - cm.y, ez = p.z - cm.z;
      float d2 = ex * ex + ey * ey;
      d2 = d2 + ez * ez;
      const bool take = (int)h.x < 0 || d2 >= __uint_as_float(h.y);   // .h:103: a leaf, or Size / d < Theta as a threshold on d2
      const int next = (take || d2 == 0.f) ? (int)(h.x & ~kLeafBit) : node + 1;   // .h:102: d == 0 ends the subtree
      const unsigned int fetch = (unsigned int)min(next, nodes - 1);   // (the last step fetches a node nobody looks at)
      const float M = cm.w;
      cm = *(const float4 *)((const char *)T.com + (fetch << 4));
      h = *(const uint2 *)((const char *)T.hop + (fetch << 3));
      if (take && d2 != 0.f) sum = sum + pot_term<SOFT>(d2, M, G, eps2);
      node = next;
    }
  } else {
    __shared__ float s_thr[kMaxLevels + 2];
    if (threadIdx.x <= kMaxLevels) s_thr[threadIdx.x] = T.thr[threadIdx.x];
    __syncthreads();
    while (node < nodes) {
      const float4 cm = T.com[node];
      const unsigned int w = T.meta[node];
      const bool leaf = (w & kLeafBit) != 0u;
      const int past = leaf ? node + 1 : (int)(w & kLinkMask);
      const float ex = p.x - cm.x, ey = p.y - cm.y, ez = p.z - cm.z;
      float d2 = ex * ex + ey * ey;
      d2 = d2 + ez * ez;
      const bool take = leaf || d2 >= s_thr[(w >> kLevelShift) & 63u];   // .h:103
      if (take && d2 != 0.f) sum = sum + pot_term<SOFT>(d2, cm.w, G, eps2);
      node = (take || d2 == 0.f) ? past : node + 1;           // .h:102
    }
  }
  if (!valid) return;
  const double phi = -sum;
  if (phi64 != nullptr) phi64[at] = phi;
  if (phif != nullptr) phif[at] = (float)phi;
}

#define BH_POT_KERNELS(HOP, SOFT)                                                                                            \
  template __global__ void bh_pot_walk_kernel<HOP, SOFT, false>(SmallTree, const float4 *, double *, float *, int, double, float); \
  template __global__ void bh_pot_walk_kernel<HOP, SOFT, true>(SmallTree, const float4 *, double *, float *, int, double, float);
BH_POT_KERNELS(false, false)
BH_POT_KERNELS(false, true)
BH_POT_KERNELS(true, false)
BH_POT_KERNELS(true, true)
#undef BH_POT_KERNELS

}  // namespace bh
}  // namespace nbody
