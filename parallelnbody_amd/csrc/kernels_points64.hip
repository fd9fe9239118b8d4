// The fp64 jerk and snap passes at points that are not bodies (nbody_jerk_at_f64 and the fp64 tracers of the shared-step Hermite calls:
// nbody_set_tracers_f64, nbody_hermite_step, nbody_hermite6_step and their advances; build-defined: the reference computes none).
// The launchers of the POINTS forms of deriv_tile_f64_kernel (deriv_tile64.h): the i side taken from caller arrays — m points as double4
// positions and double4 velocities, the snap's input accelerations three doubles at pain[k * pain_stride] — against all n_total bodies.
//   <., ., false, true, .>  <- row il of the slab (ppos, pvel, pain), the chunks' rows folded by the fold kernels of kernels_jerk.hip
//                              and kernels_snap.hip
//   <., ., true, true, .>   <- the LIST forms: row list[il] — the ACTIVE tracers of a block step (nbody_hermite[6]_block_begin_tracers),
//                              rows of the tracers' predicted arrays —, the partial rows left unfolded for the block corrector
// A point's sums depend on the point and the bodies alone — not on m, the other points, the slab, the points per lane or the device:
// a body asked about as a point at its own (x, v) gets nbody_get_jerk_f64's bits (its own pair has s2 == 0, or q d = 0 and w = 0).
#include "kernels.h"

#include <algorithm>

#include "deriv_tile64.h"

namespace nbody {

namespace {

// what both launchers refuse: nothing to do, a missing array, or a staging area that does not hold a slab's rows
bool bad(const Points64Launch &L, int width, bool folds = true) {
  if (L.m <= 0 || L.n_total <= 0 || !L.posm || !L.vel || !L.ppos || !L.pvel || !L.part || (folds && !L.out)) return true;
  return L.part_elems < probe_part_elems(L.n_total, L.m, width);
}

// the kernel's arguments for m points from row `first` of the caller's arrays
DerivArgs<true, false> jerk_args(const Points64Launch &L, size_t first, int m, int j_chunk, const int *list) {
  return {(const double4 *)L.posm, (const double4 *)L.vel, (const double4 *)L.ppos + first, (const double4 *)L.pvel + first,
          L.n_total, m, j_chunk, L.G, L.eps2, list};
}
DerivArgs<true, true> snap_args(const Points64Launch &L, size_t first, int m, int j_chunk, const int *list) {
  return {(const double4 *)L.posm, (const double4 *)L.vel, L.ain, L.ain_stride, (const double4 *)L.ppos + first, (const double4 *)L.pvel + first,
          L.pain + first * (size_t)L.pain_stride, L.pain_stride, L.n_total, m, j_chunk, L.G, L.eps2, list};
}

}  // namespace

hipError_t launch_jerk_points_f64(const Points64Launch &L, hipStream_t s) {
  if (bad(L, 3)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;                              // eps == 0: the exact d == 0 rule, as the bodies' pass
  const int ipt = hermite_block_lanes(L.m, L.lanes);           // one or two points per lane, as the block evaluation picks them
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total, 3);         // a row of six doubles: three float4
  for (size_t first = 0; first < (size_t)L.m; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.m - first);
    const dim3 grid((m + kBlock * ipt - 1) / (kBlock * ipt), j_split);
    hipLaunchKernelGGL((deriv_tile_f64_form<false, true, false>(ipt, soft)), grid, dim3(kBlock), 0, s, jerk_args(L, first, m, j_chunk, nullptr), (double *)L.part);
    if (hipError_t e = launch_jerk_fold_f64(L.part, m, j_split, L.out + 6 * first, s)) return e;
  }
  return hipGetLastError();
}

hipError_t launch_snap_points_f64(const Points64Launch &L, hipStream_t s) {
  if (bad(L, kSnapRowWidth) || !L.ain || L.ain_stride < 3 || !L.pain || L.pain_stride < 3) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  const int ipt = hermite_block_lanes(L.m, L.lanes);
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const size_t slab = probe_slab_points(L.n_total, kSnapRowWidth);
  for (size_t first = 0; first < (size_t)L.m; first += slab) {
    const int m = (int)std::min(slab, (size_t)L.m - first);
    const dim3 grid((m + kBlock * ipt - 1) / (kBlock * ipt), j_split);
    hipLaunchKernelGGL((deriv_tile_f64_form<false, true, true>(ipt, soft)), grid, dim3(kBlock), 0, s, snap_args(L, first, m, j_chunk, nullptr), (double *)L.part);
    if (hipError_t e = launch_snap_fold_f64(L.part, m, j_split, L.out + 9 * first, s)) return e;
  }
  return hipGetLastError();
}

// The list forms: ONE slab — list[0 .. m), m <= the slab — into part, unfolded: the block corrector adds the chunks' rows itself.
hipError_t launch_jerk_points_list_f64(const Points64Launch &L, const int *list, hipStream_t s) {
  if (bad(L, 3, false) || !list || (size_t)L.m > probe_slab_points(L.n_total, 3) || (L.lanes != 1 && L.lanes != 2)) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const dim3 grid((L.m + kBlock * L.lanes - 1) / (kBlock * L.lanes), j_split);
  hipLaunchKernelGGL((deriv_tile_f64_form<true, true, false>(L.lanes, L.eps2 > 0.0)), grid, dim3(kBlock), 0, s, jerk_args(L, 0, L.m, j_chunk, list), (double *)L.part);
  return hipGetLastError();
}

hipError_t launch_snap_points_list_f64(const Points64Launch &L, const int *list, hipStream_t s) {
  if (bad(L, kSnapRowWidth, false) || !list || !L.ain || L.ain_stride < 3 || !L.pain || L.pain_stride < 3 ||
      (size_t)L.m > probe_slab_points(L.n_total, kSnapRowWidth) || (L.lanes != 1 && L.lanes != 2))
    return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_total, &j_split, &j_chunk);
  const dim3 grid((L.m + kBlock * L.lanes - 1) / (kBlock * L.lanes), j_split);
  hipLaunchKernelGGL((deriv_tile_f64_form<true, true, true>(L.lanes, L.eps2 > 0.0)), grid, dim3(kBlock), 0, s, snap_args(L, 0, L.m, j_chunk, list), (double *)L.part);
  return hipGetLastError();
}

}  // namespace nbody
