// One accepted node's term of the force walks (kernels_bh_walk.hip; bh_probe_walk_kernel in kernels_bh_pot.hip) — see bh_common.h.
#pragma once
#include "bh_common.h"

namespace nbody {
namespace bh {

// One accepted node's term of Octree::ComputeForces (.h:104): float(G * M / pow(d, 3)) * (CoM - Pos), d = Dist.
// The walks are bound by the instructions of this term (N = 2^20: 16 000 per wave), so:
//  * (CoM - Pos) is taken as -(Pos - CoM), the difference the squared distance was made of: a - b and -(b - a) agree in every bit
//    except that equal operands give +0 and -0 — and such a term goes into a sum that started at +0 and therefore never is -0, so
//    adding either zero leaves every bit of it alone;
//  * the correctly rounded square root is v_sqrt_f32 (one ulp) put right by the two fused residuals the compiler's own sqrtf uses,
//    without its scaling for arguments below 2^-96 and its special cases, and the double-precision division likewise without its
//    scaling and special cases: a wave with an argument below 2^-96, an infinite / NaN one or a mass that is not finite in any of
//    its lanes takes sqrtf and the division themselves.
// SOFT: Plummer softening — the same term of ds = sqrtf(d2 + eps2), one fp32 add (not fused) in front of the root; the fast path and
// its guard look at ds2 the same way.  Where the walk goes (.h:102-103) is decided on the unsoftened d2 by the walk itself.  false:
// eps2 is not read, and the term is the reference's, instruction for instruction.
template <bool SOFT>
__device__ __forceinline__ void force_term(float cx, float cy, float cz, float M, const float4 &p, double G, float eps2, float &tx,
                                           float &ty, float &tz) {
#pragma clang fp contract(off)
  const float ex = p.x - cx, ey = p.y - cy, ez = p.z - cz;
  float d2 = ex * ex + ey * ey;
  d2 = d2 + ez * ez;
  if constexpr (SOFT) d2 = d2 + eps2;                          // ds2 (eps2 == 0 would leave every bit of d2: it is never -0)
  float d, s;                                                  // FVector::Dist, .h:101 (correctly rounded); the scale factor
  if (__any(!(d2 >= 0x1p-96f) || d2 == __builtin_inff() || !(fabsf(M) <= 0x1.fffffep127f))) {
    d = sqrtf(d2);
    const double dd = (double)d;
    s = (float)(G * (double)M / ((dd * dd) * dd));             // (d*d)*d in double = the correctly rounded cube
  } else {
    const float r = __builtin_amdgcn_sqrtf(d2);
    const float below = __uint_as_float(__float_as_uint(r) - 1u), above = __uint_as_float(__float_as_uint(r) + 1u);
    const float eb = __builtin_fmaf(-below, r, d2), ea = __builtin_fmaf(-above, r, d2);
    d = eb <= 0.0f ? below : r;
    d = ea > 0.0f ? above : d;
    // ... and the correctly rounded double quotient is the compiler's own sequence — reciprocal, two Newton steps, quotient, one
    // residual step — without the operand scaling and the special cases that cannot occur here: d in [2^-48, 2^64), so d^3 in
    // [2^-144, 2^192), G M finite: every value on the way is a normal double (a mass of +-0 gives +0 where the division gives the
    // mass's sign: a term of +-0 either way, which changes no sum).
    const double dd = (double)d, den = (dd * dd) * dd, num = G * (double)M;
    double rc = __builtin_amdgcn_rcp(den);
    rc = __builtin_fma(rc, __builtin_fma(-den, rc, 1.0), rc);
    rc = __builtin_fma(rc, __builtin_fma(-den, rc, 1.0), rc);
    const double q0 = num * rc;
    s = (float)__builtin_fma(__builtin_fma(-den, q0, num), rc, q0);
  }
  tx = s * -ex; ty = s * -ey; tz = s * -ez;
}

}  // namespace bh
}  // namespace nbody
