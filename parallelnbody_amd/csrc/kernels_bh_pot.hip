// The walk of Octree::ComputeForces (OctreeSearch.h:99-108) over the last tree built, from an arbitrary position: written once
// (walk_from_point), with what an accepted node adds left to its two users —
//   bh_probe_walk_kernel  <- the force's term (force_term): nbody_field_at's points and the tracers of nbody_set_tracers at theta > 0
//   bh_pot_walk_kernel    <- the potential's term (pot_term): nbody_potential_at, nbody_get_potentials, nbody_energy_fast at theta > 0
//                            (build-defined: the reference computes no potential)
//   bh_tidal_walk_kernel  <- the tidal tensor's term (tidal_term): nbody_tidal_at, nbody_get_tidal, nbody_tidal_time at theta > 0
//                            (build-defined as well)
#include "bh_common.h"
#include "bh_force_term.h"
#include "tracer_update.h"

namespace nbody {
namespace bh {

// One accepted node's term: G * (double)M / (double)ds, ds = sqrtf(d2 + eps2) correctly rounded (SOFT: the add is one fp32 add, not
// fused; false: eps2 is not read), the division a correctly rounded double division — what plain C computes with contraction off.
// The fast path is force_term's (bh_force_term.h): v_sqrt_f32 put right by the two fused residuals, and the compiler's own
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

// The walk from p over the tree the last frame left in its global arrays, `nodes` of them (0: the lane walks nothing): the opening test
// on the unsoftened d2, a leaf taken whatever its distance, d == 0 adds nothing and ends the subtree; on_accept(cm, d2) for every node
// that adds a term, in walk order.  A leaf's CoM is its body's position and mass, so from a body's own position this is
// bh_walk_lane_kernel's walk of that body (the body meets its own leaf at d == 0).  HOP: the tree carries hop words (the larger
// systems') and a step is the lane walk's own — the next node asked for before the term is worked out —; otherwise the plain loop on
// the node words and the levels' thresholds.  Every lane of the workgroup calls it (the thresholds go through LDS).
template <bool HOP, class OnAccept>
__device__ __forceinline__ void walk_from_point(const SmallTree &T, const float4 &p, int nodes, OnAccept on_accept) {
#pragma clang fp contract(off)
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
      const float4 cm2 = *(const float4 *)((const char *)T.com + (fetch << 4));   // 32-bit byte offsets: at most 2^25 nodes
      const uint2 h2 = *(const uint2 *)((const char *)T.hop + (fetch << 3));
      if (take && d2 != 0.f) on_accept(cm, d2);
      cm = cm2; h = h2; node = next;
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
      if (take && d2 != 0.f) on_accept(cm, d2);
      node = (take || d2 == 0.f) ? past : node + 1;           // .h:102
    }
  }
}

// The field: one lane per point in the caller's order; three fp32 sums, added to in walk order — at a body's own position that body's
// own sum in every bit.  The kernel reads the frame's verdict and does nothing unless it is 0 — a frame refused, given up or handed
// back, and every frame queued behind one, leaves tracers where they were —; it neither writes the verdict nor touches the tree.
// dt > 0: the point is a tracer and gets the bodies' update behind its walk (.cpp:29-30, multiply and add apart).
template <bool HOP, bool SOFT>
__global__ __launch_bounds__(kB) void bh_probe_walk_kernel(SmallTree T, float4 *__restrict__ pts, float4 *__restrict__ vel,
                                                           float4 *__restrict__ acc, int m, double G, float eps2, float dt) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * kB + threadIdx.x;
  const bool valid = k < m;
  const int status = T.hdr[3], nodes_all = T.hdr[0];
  if (status != 0) return;
  const float4 p = pts[valid ? k : 0];
  float ax = 0.f, ay = 0.f, az = 0.f;                          // Acceleration = ZeroVector, .cpp:84
  walk_from_point<HOP>(T, p, valid ? nodes_all : 0, [&](const float4 &cm, float) {
#pragma clang fp contract(off)
    float tx, ty, tz;
    force_term<SOFT>(cm.x, cm.y, cm.z, cm.w, p, G, eps2, tx, ty, tz);
    ax = ax + tx; ay = ay + ty; az = az + tz;
  });
  if (!valid) return;
  acc[k] = make_float4(ax, ay, az, 0.f);
  if (dt > 0.f) {
    float4 v = vel[k], x = p;
    tracer_kick_drift(dt, ax, ay, az, v, x);
    vel[k] = v;
    pts[k] = x;
  }
}

// The potential: one lane per point (BODY = false: pts[k], results at k) or per body (BODY = true: the body at sorted position k —
// neighbours in space walk side by side —, its position from posm, results at the body's index).  One fp64 accumulator, added to in
// walk order; phi = -sum.  The frame's verdict as above.
template <bool HOP, bool SOFT, bool BODY>
__global__ __launch_bounds__(kB) void bh_pot_walk_kernel(SmallTree T, const float4 *__restrict__ pts, double *__restrict__ phi64,
                                                         float *__restrict__ phif, int m, double G, float eps2) {
#pragma clang fp contract(off)
  const int k = (BODY ? xcd_run_block() : (int)blockIdx.x) * kB + threadIdx.x;
  const bool valid = k < m;
  const int status = T.hdr[3], nodes_all = T.hdr[0];
  if (status != 0) return;
  const int at = BODY ? (valid ? (int)T.sidx[k] : 0) : (valid ? k : 0);
  const float4 p = pts[at];
  double sum = 0.0;
  walk_from_point<HOP>(T, p, valid ? nodes_all : 0, [&](const float4 &cm, float d2) {
#pragma clang fp contract(off)
    sum = sum + pot_term<SOFT>(d2, cm.w, G, eps2);
  });
  if (!valid) return;
  const double phi = -sum;
  if (phi64 != nullptr) phi64[at] = phi;
  if (phif != nullptr) phif[at] = (float)phi;
}

// The tidal tensor T_ab = d a_a / d x_b: one lane per point or per body, as bh_pot_walk_kernel.  An accepted node (CoM c, mass M) adds, every
// operation one correctly rounded operation (contraction off):
//   e = p - c (fp32, the differences d2 was made of); ds = sqrtf(d2 [+ eps2]); u = 1.0 / (double)ds — pot_term with the numerator
//   1.0 (G = 1, M = 1: exactly that division; its preconditions on ds are the potential's own) —; u2 = u * u; gm = G * (double)M;
//   q3 = (gm * u) * u2; h = (3.0 * q3) * u2; hx = h * ex, ...; Sxx += hx * ex, Sxy += hx * ey, Sxz += hx * ez, Syy += hy * ey,
//   Syz += hy * ez, Szz += hz * ez; Q += q3
// to seven fp64 sums in walk order.  T = (Sxx - Q, Syy - Q, Szz - Q, Sxy, Sxz, Syz): six doubles to t64, rounded once to tf.
template <bool HOP, bool SOFT, bool BODY>
__global__ __launch_bounds__(kB) void bh_tidal_walk_kernel(SmallTree T, const float4 *__restrict__ pts, double *__restrict__ t64,
                                                           float *__restrict__ tf, int m, double G, float eps2) {
#pragma clang fp contract(off)
  const int k = (BODY ? xcd_run_block() : (int)blockIdx.x) * kB + threadIdx.x;
  const bool valid = k < m;
  const int status = T.hdr[3], nodes_all = T.hdr[0];
  if (status != 0) return;
  const int at = BODY ? (valid ? (int)T.sidx[k] : 0) : (valid ? k : 0);
  const float4 p = pts[at];
  double sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0, q = 0.0;
  walk_from_point<HOP>(T, p, valid ? nodes_all : 0, [&](const float4 &cm, float d2) {
#pragma clang fp contract(off)
    const double ex = (double)(p.x - cm.x), ey = (double)(p.y - cm.y), ez = (double)(p.z - cm.z);
    const double u = pot_term<SOFT>(d2, 1.0f, 1.0, eps2);
    const double u2 = u * u, gm = G * (double)cm.w;
    const double q3 = (gm * u) * u2;
    const double h = (3.0 * q3) * u2;
    const double hx = h * ex, hy = h * ey, hz = h * ez;
    sxx = sxx + hx * ex; sxy = sxy + hx * ey; sxz = sxz + hx * ez;
    syy = syy + hy * ey; syz = syz + hy * ez;
    szz = szz + hz * ez;
    q = q + q3;
  });
  if (!valid) return;
  const double t[6] = {sxx - q, syy - q, szz - q, sxy, sxz, syz};
  const size_t o = (size_t)at * 6;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if (t64 != nullptr) t64[o + c] = t[c];
    if (tf != nullptr) tf[o + c] = (float)t[c];
  }
}

#define BH_POINT_WALK_KERNELS(HOP, SOFT)                                                                                           \
  template __global__ void bh_probe_walk_kernel<HOP, SOFT>(SmallTree, float4 *, float4 *, float4 *, int, double, float, float);    \
  template __global__ void bh_pot_walk_kernel<HOP, SOFT, false>(SmallTree, const float4 *, double *, float *, int, double, float); \
  template __global__ void bh_pot_walk_kernel<HOP, SOFT, true>(SmallTree, const float4 *, double *, float *, int, double, float);  \
  template __global__ void bh_tidal_walk_kernel<HOP, SOFT, false>(SmallTree, const float4 *, double *, float *, int, double, float); \
  template __global__ void bh_tidal_walk_kernel<HOP, SOFT, true>(SmallTree, const float4 *, double *, float *, int, double, float);
BH_POINT_WALK_KERNELS(false, false)
BH_POINT_WALK_KERNELS(false, true)
BH_POINT_WALK_KERNELS(true, false)
BH_POINT_WALK_KERNELS(true, true)
#undef BH_POINT_WALK_KERNELS

}  // namespace bh
}  // namespace nbody
