// Hermite block time steps of fp64 contexts, both orders (nbody_hermite_block_begin / _advance / _get, nbody_hermite6_block_*;
// build-defined: the reference has one integrator and one step) — per-body power-of-two steps around an ACTIVE-SET form of the fp64 jerk
// pass (fourth order, Makino & Aarseth) or snap pass (sixth order, Nitadori & Makino).  Time is counted in integer ticks,
// tick = dt_max 2^-levels; body i is at T[i] with level k = level[i], its step 2^(levels - k) ticks.  One block step:
//   hermite_block_next_kernel     <- per segment of bodies (a workgroup each): the smallest T[i] + step_i and how many bodies attain it
//   hermite[6]_block_list_kernel  <- hermite_block_list (hermite_block_sched.h): T_next = the smallest of those, the bodies that attain it
//                                    as a list in ascending body index; EVERY body predicted to T_next with its own dt by the order's
//                                    predictor (hermite_step64.h): (xp, vp), sixth order (xp, vp, ap)
//   deriv_tile_f64_kernel<., ., true, false, SNAP> (deriv_tile64.h: the jerk pass's / the snap pass's kernel)  <- the rows of the listed bodies
//                                    against all predicted bodies: one partial row per listed body and chunk, the chunks, the pair
//                                    operations and their order those of nbody_get_jerk_f64 / nbody_get_snap_f64
//   hermite[6]_block_correct_kernel <- the listed bodies: the chunks' rows added in chunk order (the fold kernels' sums), the order's
//                                    corrector (hermite_step64.h) with the body's own dt, T[i] := T_next, the new level (hermite_block_level.h)
//   hermite_block_init_kernel<ROW> <- T := 0 and the first levels, given or from eta_start |a| / |j| of the cached rows (ROW doubles each)
// A session that carries fp64 tracers (nbody_hermite[6]_block_begin_tracers) runs the same kernels on a second set of arrays, the tracers';
// the list kernels' <true> forms then take T_next over both sets, and the tracers' rows come from kernels_points64.hip.
// What is written once and what per order: DESIGN 4.16b.  EVERY operation outside the pair sums is one correctly rounded fp64 operation
// in the order written: contraction is off for the whole file, so that numpy (tests/hermite_block_ref.py, tests/hermite6_block_ref.py)
// reproduces a block step in every bit.  No scratch, no grid-wide waits; the one atomic is an integer count of floor hits.
#include "kernels.h"

#include "deriv_tile64.h"

#include "hermite_block_level.h"
#include "hermite_block_sched.h"
#include "hermite_step64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// segment s = bodies [s seg_len, min(n, (s + 1) seg_len)), seg_len a multiple of kBlock
__global__ __launch_bounds__(kBlock) void hermite_block_next_kernel(const long long *__restrict__ T, const int *__restrict__ level, int n,
                                                                    int seg_len, int levels, long long *__restrict__ seg_min,
                                                                    int *__restrict__ seg_cnt) {
  __shared__ long long redl[kBlock / 64];
  __shared__ int redi[kBlock / 64];
  const int b0 = min(n, (int)blockIdx.x * seg_len), b1 = min(n, b0 + seg_len);
  long long mn = kNever;
  for (int i = b0 + threadIdx.x; i < b1; i += kBlock) {
    const long long due = T[i] + (1ll << (levels - level[i]));
    mn = due < mn ? due : mn;
  }
  mn = block_min_workgroup(mn, redl);
  int cnt = 0;
  for (int i = b0 + threadIdx.x; i < b1; i += kBlock) cnt += (T[i] + (1ll << (levels - level[i])) == mn) ? 1 : 0;
  cnt = block_sum_workgroup(cnt, redi);
  if (threadIdx.x == 0) { seg_min[blockIdx.x] = mn; seg_cnt[blockIdx.x] = cnt; }
}

// hermite_block_list with the order's predictor on the constants of the body's own dt.  <false> is the kernel of a session without tracers.
template <bool JOINT>
__global__ __launch_bounds__(kBlock) void hermite_block_list_kernel(const long long *__restrict__ T, const int *__restrict__ level,
                                                                    const long long *__restrict__ seg_min, const int *__restrict__ seg_cnt,
                                                                    int slots, int n, int seg_len, int levels, double tick,
                                                                    const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                    const double *__restrict__ aj0, double4 *__restrict__ xp,
                                                                    double4 *__restrict__ vp, int *__restrict__ list,
                                                                    long long *__restrict__ record,
                                                                    const long long *__restrict__ other_min, int other_slots) {
  hermite_block_list<JOINT>(T, level, seg_min, seg_cnt, slots, n, seg_len, levels, tick, list, record, other_min, other_slots,
                            [&](int i, double dt) { hermite4_predict(hermite4_predict_consts(dt), posm, vel, aj0, xp, vp, i); });
}
template <bool JOINT>
__global__ __launch_bounds__(kBlock) void hermite6_block_list_kernel(const long long *__restrict__ T, const int *__restrict__ level,
                                                                     const long long *__restrict__ seg_min, const int *__restrict__ seg_cnt,
                                                                     int slots, int n, int seg_len, int levels, double tick,
                                                                     const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                     const double *__restrict__ ajs0, const double4 *__restrict__ a3,
                                                                     double4 *__restrict__ xp, double4 *__restrict__ vp,
                                                                     double4 *__restrict__ ap, int *__restrict__ list,
                                                                     long long *__restrict__ record,
                                                                     const long long *__restrict__ other_min, int other_slots) {
  hermite_block_list<JOINT>(T, level, seg_min, seg_cnt, slots, n, seg_len, levels, tick, list, record, other_min, other_slots,
                            [&](int i, double dt) { hermite6_predict(hermite6_predict_consts(dt), posm, vel, ajs0, a3, xp, vp, ap, i); });
}

// the session's rule as a corrector takes it: eta is root_eta at the fourth order
struct BlockRule { double tick, dt_max, eta; int levels; };

// One lane per listed body k < m, body i = list[k], dt = (double)(T_next - T[i]) tick — for a listed body exactly dt_max 2^-level —,
// (a1, j1) = the rows part[(c m + k) 6 ..] added in chunk order from 0, hermite4_correct on them:
// x := x1, v := v1, acc := (a1, 0), (a0, j0) := (a1, j1), a2, a3, T := T_next; then the level: hermite4_ratio of the NEW vectors — what is not
// finite left to time_of_k —, dt_c = root_eta / sqrt(k), kw = hermite_block_level(dt_c), level := hermite_block_next_level.  A body that
// no level fits adds one to *floor_hits (an integer count: the order of the additions does not show).
__global__ __launch_bounds__(kBlock) void hermite_block_correct_kernel(const int *__restrict__ list, int m, const double *__restrict__ part,
                                                                       int j_split, long long t_next, BlockRule r, long long *__restrict__ T,
                                                                       int *__restrict__ level, double4 *__restrict__ posm,
                                                                       double4 *__restrict__ vel, double4 *__restrict__ acc,
                                                                       double *__restrict__ aj0, double4 *__restrict__ a2,
                                                                       double4 *__restrict__ a3, unsigned long long *__restrict__ floor_hits) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  const int i = list[k];
  const Hermite4Correct c = hermite4_correct_consts((double)(t_next - T[i]) * r.tick);
  double s1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int ch = 0; ch < j_split; ++ch) {
    const double *row = part + ((size_t)ch * m + k) * 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) s1[q] = s1[q] + row[q];
  }
  const double4 x = posm[i], v = vel[i];
  const Aj s0 = load_aj(aj0, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  Hermite4Comp n1[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) n1[q] = hermite4_correct(c, xc[q], vc[q], s0.a[q], s0.j[q], s1[q], s1[3 + q]);
  posm[i] = make_double4(n1[0].x, n1[1].x, n1[2].x, x.w);
  vel[i] = make_double4(n1[0].v, n1[1].v, n1[2].v, v.w);
  acc[i] = make_double4(s1[0], s1[1], s1[2], 0.0);
  double2 *row0 = (double2 *)(aj0 + 6 * (size_t)i);
  row0[0] = make_double2(s1[0], s1[1]); row0[1] = make_double2(s1[2], s1[3]); row0[2] = make_double2(s1[4], s1[5]);
  a2[i] = make_double4(n1[0].a2, n1[1].a2, n1[2].a2, 0.0);
  a3[i] = make_double4(n1[0].a3, n1[1].a3, n1[2].a3, 0.0);
  T[i] = t_next;

  const double kk = ratio_k<false>(hermite4_ratio(norm3(s1[0], s1[1], s1[2]), norm3(s1[3], s1[4], s1[5]),
                                                  norm3(n1[0].a2, n1[1].a2, n1[2].a2), norm3(n1[0].a3, n1[1].a3, n1[2].a3)));
  const double dt_c = r.eta * time_of_k(kk);
  int floor_hit;
  const int kw = hermite_block_level(dt_c, r.dt_max, r.levels, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
  level[i] = hermite_block_next_level(level[i], kw, t_next, r.levels);
}

// The same with (a1, j1, s1) = the rows part[(c m + k) 9 ..] and hermite6_correct:  x := x1, v := v1, acc := (a1, 0), (a0, j0, s0) :=
// (a1, j1, s1), a3, a4, a5, T := T_next; then the level: hermite6_ratio of the NEW vectors (not finite = +inf), kw = hermite6_block_level(kk).
__global__ __launch_bounds__(kBlock) void hermite6_block_correct_kernel(const int *__restrict__ list, int m, const double *__restrict__ part,
                                                                        int j_split, long long t_next, BlockRule r,
                                                                        long long *__restrict__ T, int *__restrict__ level,
                                                                        double4 *__restrict__ posm, double4 *__restrict__ vel,
                                                                        double4 *__restrict__ acc, double *__restrict__ ajs0,
                                                                        double4 *__restrict__ a3, double4 *__restrict__ a4,
                                                                        double4 *__restrict__ a5,
                                                                        unsigned long long *__restrict__ floor_hits) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  const int i = list[k];
  const Hermite6Correct c = hermite6_correct_consts((double)(t_next - T[i]) * r.tick);
  double s1[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int ch = 0; ch < j_split; ++ch) {
    const double *row = part + ((size_t)ch * m + k) * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) s1[q] = s1[q] + row[q];
  }
  const double4 x = posm[i], v = vel[i];
  const Ajs s0 = load_ajs(ajs0, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  Hermite6Comp n1[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) n1[q] = hermite6_correct(c, xc[q], vc[q], s0.a[q], s0.j[q], s0.s[q], s1[q], s1[3 + q], s1[6 + q]);
  posm[i] = make_double4(n1[0].x, n1[1].x, n1[2].x, x.w);
  vel[i] = make_double4(n1[0].v, n1[1].v, n1[2].v, v.w);
  acc[i] = make_double4(s1[0], s1[1], s1[2], 0.0);
  double *row0 = ajs0 + 9 * (size_t)i;
#pragma unroll
  for (int q = 0; q < 9; ++q) row0[q] = s1[q];
  a3[i] = make_double4(n1[0].a3, n1[1].a3, n1[2].a3, 0.0);
  a4[i] = make_double4(n1[0].a4, n1[1].a4, n1[2].a4, 0.0);
  a5[i] = make_double4(n1[0].a5, n1[1].a5, n1[2].a5, 0.0);
  T[i] = t_next;

  const double kk = ratio_k<true>(hermite6_ratio(norm3(s1[0], s1[1], s1[2]), norm3(s1[3], s1[4], s1[5]), norm3(s1[6], s1[7], s1[8]),
                                                 norm3(n1[0].a3, n1[1].a3, n1[2].a3), norm3(n1[0].a4, n1[1].a4, n1[2].a4),
                                                 norm3(n1[0].a5, n1[1].a5, n1[2].a5)));
  int floor_hit;
  const int kw = hermite6_block_level(kk, r.dt_max, r.levels, r.eta, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
  level[i] = hermite_block_next_level(level[i], kw, t_next, r.levels);
}

// T := 0; level := level_in, or the start rule of both orders on the cached (a0, j0), the first six of a row's ROW doubles: the level of
// dt_c = eta_start t, t = 1 / sqrt(k) of nbody_jerk_time's k = |j|^2 / |a|^2
template <int ROW>
__global__ __launch_bounds__(kBlock) void hermite_block_init_kernel(const double *__restrict__ rows, const int *__restrict__ level_in, int n,
                                                                    double eta_start, double dt_max, int levels, long long *__restrict__ T,
                                                                    int *__restrict__ level, unsigned long long *__restrict__ floor_hits) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T[i] = 0;
  if (level_in != nullptr) { level[i] = level_in[i]; return; }
  const auto s = load_row<ROW>(rows, i);
  const double a2 = sqnorm3(s.a[0], s.a[1], s.a[2]), j2 = sqnorm3(s.j[0], s.j[1], s.j[2]);
  const double dt_c = eta_start * time_of_k(ratio_k<false>(Ratio{j2, a2}));
  int floor_hit;
  level[i] = hermite_block_level(dt_c, dt_max, levels, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
}

// ---- what a launcher asks of either order's arrays ----
inline bool bad_base(const HermiteBlockBase &L) {
  return L.n <= 0 || L.levels < 0 || L.levels > kHermiteBlockMaxLevels || !L.posm || !L.vel || !L.T || !L.level || !L.list || !L.seg_min ||
         !L.seg_cnt || !L.record || !L.floor_hits;
}
inline bool bad(const HermiteBlockLaunch &L) { return bad_base(L) || !L.aj0; }
inline bool bad(const Hermite6BlockLaunch &L) { return bad_base(L) || !L.ajs0 || !L.a3; }
inline bool no_prediction(const HermiteBlockLaunch &L) { return !L.xp || !L.vp; }
inline bool no_prediction(const Hermite6BlockLaunch &L) { return !L.xp || !L.vp || !L.ap; }
inline const double *rows_of(const HermiteBlockLaunch &L) { return L.aj0; }
inline const double *rows_of(const Hermite6BlockLaunch &L) { return L.ajs0; }

template <bool JOINT>
void launch_list(const HermiteBlockLaunch &L, int slots, int seg_len, const long long *other_min, int other_slots, hipStream_t s) {
  hipLaunchKernelGGL(hermite_block_list_kernel<JOINT>, dim3(slots), dim3(kBlock), 0, s, (const long long *)L.T, (const int *)L.level,
                     (const long long *)L.seg_min, (const int *)L.seg_cnt, slots, L.n, seg_len, L.levels, L.tick, (const double4 *)L.posm,
                     (const double4 *)L.vel, (const double *)L.aj0, (double4 *)L.xp, (double4 *)L.vp, L.list, L.record, other_min,
                     other_slots);
}
template <bool JOINT>
void launch_list(const Hermite6BlockLaunch &L, int slots, int seg_len, const long long *other_min, int other_slots, hipStream_t s) {
  hipLaunchKernelGGL(hermite6_block_list_kernel<JOINT>, dim3(slots), dim3(kBlock), 0, s, (const long long *)L.T, (const int *)L.level,
                     (const long long *)L.seg_min, (const int *)L.seg_cnt, slots, L.n, seg_len, L.levels, L.tick, (const double4 *)L.posm,
                     (const double4 *)L.vel, (const double *)L.ajs0, (const double4 *)L.a3, (double4 *)L.xp, (double4 *)L.vp,
                     (double4 *)L.ap, L.list, L.record, other_min, other_slots);
}

template <class Launch>
hipError_t block_init(const Launch &L, const int *level_in, double eta_start, hipStream_t s) {
  if (bad(L)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite_block_init_kernel<Launch::kRow>, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, rows_of(L),
                     level_in, L.n, eta_start, L.dt_max, L.levels, L.T, L.level, L.floor_hits);
  return hipGetLastError();
}

template <class Launch>
hipError_t block_schedule(const Launch &L, hipStream_t s) {
  if (bad(L) || no_prediction(L)) return hipErrorInvalidValue;
  int slots;
  const int seg_len = hermite_block_segment(L.n, &slots);
  if (hipError_t e = launch_hermite_block_next(L.T, L.level, L.n, L.levels, L.seg_min, L.seg_cnt, s)) return e;
  launch_list<false>(L, slots, seg_len, nullptr, 0, s);
  return hipGetLastError();
}

template <class Launch>
hipError_t block_schedule_joint(const Launch &B, const Launch &P, hipStream_t s) {
  if (bad(B) || no_prediction(B) || bad(P) || no_prediction(P) || B.levels != P.levels || B.tick != P.tick) return hipErrorInvalidValue;
  int slots[2];
  const Launch *set[2] = {&B, &P};
  for (const Launch *L : set)
    if (hipError_t e = launch_hermite_block_next(L->T, L->level, L->n, L->levels, L->seg_min, L->seg_cnt, s)) return e;
  const int seg_len[2] = {hermite_block_segment(B.n, &slots[0]), hermite_block_segment(P.n, &slots[1])};
  for (int k = 0; k < 2; ++k) launch_list<true>(*set[k], slots[k], seg_len[k], set[k ^ 1]->seg_min, slots[k ^ 1], s);
  return hipGetLastError();
}

// what both evaluations and both correctors refuse: a range of the list outside it
inline bool bad_range(const HermiteBlockBase &L, int first, int m) { return !L.part || first < 0 || m <= 0 || first + m > L.n; }

}  // namespace

int hermite_block_segment(int n, int *slots) {
  const int s = energy_fast_slots(n), chunks = (n + kBlock - 1) / kBlock;
  if (slots) *slots = s;
  return (chunks + s - 1) / s * kBlock;
}

int hermite_block_lanes(int m, int forced) {
  if (forced == 1 || forced == 2) return forced;
  return m <= kHermiteBlockOneLaneMax ? 1 : 2;
}

hipError_t launch_hermite_block_next(const long long *T, const int *level, int n, int levels, long long *seg_min, int *seg_cnt,
                                     hipStream_t s) {
  if (n <= 0 || levels < 0 || levels > kHermiteBlockMaxLevels || !T || !level || !seg_min || !seg_cnt) return hipErrorInvalidValue;
  int slots;
  const int seg_len = hermite_block_segment(n, &slots);
  hipLaunchKernelGGL(hermite_block_next_kernel, dim3(slots), dim3(kBlock), 0, s, T, level, n, seg_len, levels, seg_min, seg_cnt);
  return hipGetLastError();
}

hipError_t launch_hermite_block_init(const HermiteBlockLaunch &L, const int *level_in, double eta_start, hipStream_t s) {
  return block_init(L, level_in, eta_start, s);
}
hipError_t launch_hermite6_block_init(const Hermite6BlockLaunch &L, const int *level_in, double eta_start, hipStream_t s) {
  return block_init(L, level_in, eta_start, s);
}
hipError_t launch_hermite_block_schedule(const HermiteBlockLaunch &L, hipStream_t s) { return block_schedule(L, s); }
hipError_t launch_hermite6_block_schedule(const Hermite6BlockLaunch &L, hipStream_t s) { return block_schedule(L, s); }
hipError_t launch_hermite_block_schedule_joint(const HermiteBlockLaunch &B, const HermiteBlockLaunch &P, hipStream_t s) {
  return block_schedule_joint(B, P, s);
}
hipError_t launch_hermite6_block_schedule_joint(const Hermite6BlockLaunch &B, const Hermite6BlockLaunch &P, hipStream_t s) {
  return block_schedule_joint(B, P, s);
}

hipError_t launch_hermite_block_evaluate(const HermiteBlockLaunch &L, int first, int m, int lanes, hipStream_t s) {
  if (bad(L) || no_prediction(L) || bad_range(L, first, m) || (lanes != 1 && lanes != 2)) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n, &j_split, &j_chunk);
  if ((size_t)m > probe_slab_points(L.n, 3)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  const dim3 grid((m + kBlock * lanes - 1) / (kBlock * lanes), j_split);
  hipLaunchKernelGGL((deriv_tile_f64_form<true, false, false>(lanes, soft)), grid, dim3(kBlock), 0, s,
                     DerivArgs<false, false>{(const double4 *)L.xp, (const double4 *)L.vp, L.n, m, 0, j_chunk, L.G, L.eps2, (const int *)L.list + first},
                     (double *)L.part);
  return hipGetLastError();
}

hipError_t launch_hermite6_block_evaluate(const Hermite6BlockLaunch &L, int first, int m, int lanes, hipStream_t s) {
  if (bad(L) || no_prediction(L) || bad_range(L, first, m) || (lanes != 1 && lanes != 2)) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n, &j_split, &j_chunk);
  if ((size_t)m > probe_slab_points(L.n, kSnapRowWidth)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  const dim3 grid((m + kBlock * lanes - 1) / (kBlock * lanes), j_split);
  hipLaunchKernelGGL((deriv_tile_f64_form<true, false, true>(lanes, soft)), grid, dim3(kBlock), 0, s,
                     DerivArgs<false, true>{(const double4 *)L.xp, (const double4 *)L.vp, (const double *)L.ap, 4, L.n, m, 0, j_chunk, L.G, L.eps2,
                                            (const int *)L.list + first},
                     (double *)L.part);
  return hipGetLastError();
}

hipError_t launch_hermite_block_correct(const HermiteBlockLaunch &L, int first, int m, long long t_next, hipStream_t s) {
  if (bad(L) || !L.acc || !L.a2 || !L.a3 || bad_range(L, first, m)) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_field > 0 ? L.n_field : L.n, &j_split, &j_chunk);   // (the rows' chunks are those of the bodies that exert the field)
  const BlockRule r{L.tick, L.dt_max, L.root_eta, L.levels};
  hipLaunchKernelGGL(hermite_block_correct_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const int *)L.list + first, m,
                     (const double *)L.part, j_split, t_next, r, L.T, L.level, (double4 *)L.posm, (double4 *)L.vel, (double4 *)L.acc, L.aj0,
                     (double4 *)L.a2, (double4 *)L.a3, L.floor_hits);
  return hipGetLastError();
}

hipError_t launch_hermite6_block_correct(const Hermite6BlockLaunch &L, int first, int m, long long t_next, hipStream_t s) {
  if (bad(L) || !L.acc || !L.a4 || !L.a5 || bad_range(L, first, m)) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_field > 0 ? L.n_field : L.n, &j_split, &j_chunk);   // (the rows' chunks are those of the bodies that exert the field)
  const BlockRule r{L.tick, L.dt_max, L.eta, L.levels};
  hipLaunchKernelGGL(hermite6_block_correct_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const int *)L.list + first, m,
                     (const double *)L.part, j_split, t_next, r, L.T, L.level, (double4 *)L.posm, (double4 *)L.vel, (double4 *)L.acc, L.ajs0,
                     (double4 *)L.a3, (double4 *)L.a4, (double4 *)L.a5, L.floor_hits);
  return hipGetLastError();
}

}  // namespace nbody
