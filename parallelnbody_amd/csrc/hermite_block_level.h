// The level rules of the Hermite block time steps (nbody_hermite_block_* and nbody_hermite6_block_*, both in
// kernels_hermite_block.hip), one function each for the device and the host: the correctors call them per active body,
// nbody_hermite_block_level and nbody_hermite6_block_level export them so that the CPU tests pin them without a device.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace nbody {

constexpr int kHermiteBlockMaxLevels = 40;

// The level a body wants whose criterion gives the step dt_c: the smallest k in 0 .. levels with ldexp(dt_max, -k) <= dt_c (level k
// steps by dt_max 2^-k).  If there is none — dt_c below the smallest step, 0, or not a number — the body is clamped to `levels` and
// *floor_hit = 1; otherwise *floor_hit = 0.  ldexp is exact while the steps are normal numbers (the session demands a normal tick).
__host__ __device__ inline int hermite_block_level(double dt_c, double dt_max, int levels, int *floor_hit) {
  *floor_hit = 0;
  for (int k = 0; k <= levels; ++k)
    if (ldexp(dt_max, -k) <= dt_c) return k;
  *floor_hit = 1;
  return levels;
}

// The sixth-order rule (nbody_hermite6_block_*).  kk is nbody_hermite6_timescale's per-body
// k = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2), whose step is eta kk^(-1/6).  A cube root is not correctly rounded, so the device and
// numpy could not agree on it in every bit; the rule therefore compares in the CUBED domain, where every operation is: r = sqrt(kk),
// e3 = (eta eta) eta, and the level is the smallest k in 0 .. levels with ((h h) h) r <= e3, h = ldexp(dt_max, -k) — which is
// h <= eta kk^(-1/6).  h^3 shrinks by exactly 2^-3 per level while it is normal (the session demands a normal tick^3), so the test is
// monotone in k.  kk == 0 gives level 0; kk = +inf or NaN makes every comparison false.  If no k passes the body is clamped to `levels`
// and *floor_hit = 1; otherwise *floor_hit = 0.
__host__ __device__ inline int hermite6_block_level(double kk, double dt_max, int levels, double eta, int *floor_hit) {
  const double r = sqrt(kk), e3 = (eta * eta) * eta;
  *floor_hit = 0;
  for (int k = 0; k <= levels; ++k) {
    const double h = ldexp(dt_max, -k);
    if (((h * h) * h) * r <= e3) return k;
  }
  *floor_hit = 1;
  return levels;
}

// The level an active body takes on from its level `k`, the level `kw` it wants and the time `t_next` (ticks) it has just reached:
// down (a smaller step) at once and by any amount — every multiple of a step is a multiple of the smaller ones —, up by ONE level
// and only where t_next is a multiple of the doubled step, 2^(levels - k + 1) ticks.
__host__ __device__ inline int hermite_block_next_level(int k, int kw, long long t_next, int levels) {
  if (kw > k) return kw;
  if (kw < k && (t_next & ((1ll << (levels - k + 1)) - 1)) == 0) return k - 1;
  return k;
}

}  // namespace nbody
