// Sixth-order Hermite block time steps of fp64 contexts (nbody_hermite6_block_begin / _advance / _get; build-defined: the reference has
// one integrator and one step) — Nitadori & Makino's scheme with a step per body, around an ACTIVE-SET form of the fp64 snap pass.  Times,
// ticks, levels and segments are those of kernels_hermite_block.hip, whose first scheduler kernel (launch_hermite_block_next: integers
// only) this file queues as it is.  One block step:
//   hermite_block_next_kernel      <- per segment of bodies: the smallest T[i] + step_i and how many bodies attain it
//   hermite6_block_list_kernel     <- T_next, the bodies that attain it as a list in ascending body index (segment offsets from the counts,
//                                     a body's place by a ballot scan: no atomics); EVERY body predicted to T_next with its own dt:
//                                     (xp, vp, ap) by the sixth-order predictor of kernels_snap.hip
//   snap_tile_f64_kernel<., ., true> (snap_tile64.h)  <- (a1, j1, s1) of the listed bodies against all predicted bodies given ap: one
//                                     partial row per listed body and chunk, the chunks, pair operations and order nbody_get_snap_f64's
//   hermite6_block_correct_kernel  <- the listed bodies: the chunks' rows added in chunk order (snap_fold_f64_kernel's sums), the corrector
//                                     of kernels_snap.hip with the body's own dt, T[i] := T_next, the new level (hermite_block_level.h)
//   hermite6_block_init_kernel     <- T := 0 and the first levels, given or from eta_start |a0| / |j0|
// A session that carries fp64 tracers (nbody_hermite6_block_begin_tracers) runs the same kernels on the tracers' arrays as a second
// set; hermite6_block_list_kernel<true> then takes T_next over both sets, and the tracers' rows come from snap_points_f64_kernel<., ., true>.
// EVERY operation outside the pair sums is one correctly rounded fp64 operation in the order written: contraction is off for the whole
// file, so that numpy (tests/hermite6_block_ref.py) reproduces a block step in every bit.  No scratch, no grid-wide waits; the one atomic
// is an integer count of floor hits.
#include "kernels.h"

#include "hermite_block_level.h"
#include "hermite_block_sched.h"
#include "snap_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// a body's (a, j, s) in the snap fold's rows: nine doubles, 72 bytes apart
struct Ajs { double a[3], j[3], s[3]; };
__device__ __forceinline__ Ajs load_ajs(const double *__restrict__ ajs, int i) {
  const double *r = ajs + 9 * (size_t)i;
  return Ajs{{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}};
}

// record[0] = T_next, record[1] = m; list[0 .. m) ascending; per body and component, with dt = (double)(T_next - T[i]) tick, d2 = dt dt,
// c2 = d2 0.5, c3 = (d2 dt) / 6, c4 = (d2 d2) / 24, c5 = ((d2 d2) dt) / 120:
//   xp = ((((x + dt v) + c2 a0) + c3 j0) + c4 s0) + c5 a3;  vp = (((v + dt a0) + c2 j0) + c3 s0) + c4 a3;  ap = ((a0 + dt j0) + c2 s0) + c3 a3
// xp.w = m, vp.w = 0, ap.w = 0
// JOINT: T_next is the smallest due time of BOTH sets of a session that carries tracers — this set's segments and the other's
// (other_min[0 .. other_slots)) —; a set with nobody due at T_next writes m = 0 and an empty list.  <false> is the kernel it was.
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
      const double dt = (double)(tn - Ti) * tick;
      const double d2 = dt * dt;
      const double c2 = d2 * 0.5, c3 = (d2 * dt) / 6.0, c4 = (d2 * d2) / 24.0, c5 = ((d2 * d2) * dt) / 120.0;
      const double4 x = posm[i], v = vel[i], d3 = a3[i];
      const Ajs q = load_ajs(ajs0, i);
      auto px = [&](double xc, double vc, double a, double j, double sn, double c) {
        return ((((xc + dt * vc) + c2 * a) + c3 * j) + c4 * sn) + c5 * c;
      };
      auto pv = [&](double vc, double a, double j, double sn, double c) { return (((vc + dt * a) + c2 * j) + c3 * sn) + c4 * c; };
      auto pa = [&](double a, double j, double sn, double c) { return ((a + dt * j) + c2 * sn) + c3 * c; };
      xp[i] = make_double4(px(x.x, v.x, q.a[0], q.j[0], q.s[0], d3.x), px(x.y, v.y, q.a[1], q.j[1], q.s[1], d3.y),
                           px(x.z, v.z, q.a[2], q.j[2], q.s[2], d3.z), x.w);
      vp[i] = make_double4(pv(v.x, q.a[0], q.j[0], q.s[0], d3.x), pv(v.y, q.a[1], q.j[1], q.s[1], d3.y), pv(v.z, q.a[2], q.j[2], q.s[2], d3.z), 0.0);
      ap[i] = make_double4(pa(q.a[0], q.j[0], q.s[0], d3.x), pa(q.a[1], q.j[1], q.s[1], d3.y), pa(q.a[2], q.j[2], q.s[2], d3.z), 0.0);
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

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
// the start rule's step 1 / sqrt(k) of k = |j|^2 / |a|^2: +inf for k == 0, 0 for a k that is not finite
__device__ __forceinline__ double time_of_k(double k) {
  if (k == 0.0) return __builtin_inf();
  if (!(k <= 0x1.fffffffffffffp1023)) return 0.0;
  return 1.0 / sqrt(k);
}

struct Block6Rule { double tick, dt_max, eta; int levels; };

// One lane per listed body k < m, body i = list[k], dt = (double)(T_next - T[i]) tick — for a listed body exactly dt_max 2^-level —,
// d2 = dt dt, d4 = d2 d2, ch = dt 0.5, c2 = d2 0.5, c10 = d2 / 10, c120 = (d2 dt) / 120, d3 = d2 dt, d5 = d4 dt (launch_hermite6_correct's
// order), (a1, j1, s1) = the rows part[(c m + k) 9 ..] added in chunk order from 0:
//   v1 = v + ((ch (a0 + a1) + c10 (j0 - j1)) + c120 (s0 + s1));   x1 = x + ((ch (v + v1) + c10 (a0 - a1)) + c120 (j0 + j1))
//   R1 = ((a1 - a0) - dt j0) - c2 s0;   R2 = dt ((j1 - j0) - dt s0);   R3 = d2 (s1 - s0)
//   X = ((60 R1) - (24 R2)) + (3 R3);   Y = ((168 R2) - (360 R1)) - (24 R3);   Z = ((720 R1) - (360 R2)) + (60 R3)
//   a3 = ((X + Y) + 0.5 Z) / d3;   a4 = (Y + Z) / d4;   a5 = Z / d5
// x := x1, v := v1, acc := (a1, 0), (a0, j0, s0) := (a1, j1, s1), a3, a4, a5, T := T_next; then the level: kk = (|a3| |a5| + |a4|^2) /
// (|a0| |s0| + |j0|^2) of the NEW vectors (0 / 0 = 0, not finite = +inf), kw = hermite6_block_level(kk), level :=
// hermite_block_next_level.  A body that no level fits adds one to *floor_hits (an integer count: the order of the additions does not show).
__global__ __launch_bounds__(kBlock) void hermite6_block_correct_kernel(const int *__restrict__ list, int m, const double *__restrict__ part,
                                                                        int j_split, long long t_next, Block6Rule r,
                                                                        long long *__restrict__ T, int *__restrict__ level,
                                                                        double4 *__restrict__ posm, double4 *__restrict__ vel,
                                                                        double4 *__restrict__ acc, double *__restrict__ ajs0,
                                                                        double4 *__restrict__ a3, double4 *__restrict__ a4,
                                                                        double4 *__restrict__ a5,
                                                                        unsigned long long *__restrict__ floor_hits) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  const int i = list[k];
  const double dt = (double)(t_next - T[i]) * r.tick;
  const double d2 = dt * dt, d4 = d2 * d2;
  const double ch = dt * 0.5, c2 = d2 * 0.5, c10 = d2 / 10.0, c120 = (d2 * dt) / 120.0, d3 = d2 * dt, d5 = d4 * dt;
  double n1[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) n1[q] = n1[q] + row[q];
  }
  const double4 x = posm[i], v = vel[i];
  const Ajs s0 = load_ajs(ajs0, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  double x1[3], v1[3], q3[3], q4[3], q5[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double a1 = n1[q], j1 = n1[3 + q], s1 = n1[6 + q];
    v1[q] = vc[q] + ((ch * (s0.a[q] + a1) + c10 * (s0.j[q] - j1)) + c120 * (s0.s[q] + s1));
    x1[q] = xc[q] + ((ch * (vc[q] + v1[q]) + c10 * (s0.a[q] - a1)) + c120 * (s0.j[q] + j1));
    const double R1 = ((a1 - s0.a[q]) - dt * s0.j[q]) - c2 * s0.s[q];
    const double R2 = dt * ((j1 - s0.j[q]) - dt * s0.s[q]);
    const double R3 = d2 * (s1 - s0.s[q]);
    const double X = ((60.0 * R1) - (24.0 * R2)) + (3.0 * R3);
    const double Y = ((168.0 * R2) - (360.0 * R1)) - (24.0 * R3);
    const double Z = ((720.0 * R1) - (360.0 * R2)) + (60.0 * R3);
    q3[q] = ((X + Y) + 0.5 * Z) / d3;
    q4[q] = (Y + Z) / d4;
    q5[q] = Z / d5;
  }
  posm[i] = make_double4(x1[0], x1[1], x1[2], x.w);
  vel[i] = make_double4(v1[0], v1[1], v1[2], v.w);
  acc[i] = make_double4(n1[0], n1[1], n1[2], 0.0);
  double *row0 = ajs0 + 9 * (size_t)i;
#pragma unroll
  for (int q = 0; q < 9; ++q) row0[q] = n1[q];
  a3[i] = make_double4(q3[0], q3[1], q3[2], 0.0);
  a4[i] = make_double4(q4[0], q4[1], q4[2], 0.0);
  a5[i] = make_double4(q5[0], q5[1], q5[2], 0.0);
  T[i] = t_next;

  const double A0 = norm3(n1[0], n1[1], n1[2]), J0 = norm3(n1[3], n1[4], n1[5]), S0 = norm3(n1[6], n1[7], n1[8]);
  const double A3 = norm3(q3[0], q3[1], q3[2]), A4 = norm3(q4[0], q4[1], q4[2]), A5 = norm3(q5[0], q5[1], q5[2]);
  const double num = A3 * A5 + A4 * A4, den = A0 * S0 + J0 * J0;
  double kk = (num == 0.0 && den == 0.0) ? 0.0 : num / den;
  if (!(kk <= 0x1.fffffffffffffp1023)) kk = __builtin_inf();
  int floor_hit;
  const int kw = hermite6_block_level(kk, r.dt_max, r.levels, r.eta, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
  level[i] = hermite_block_next_level(level[i], kw, t_next, r.levels);
}

// T := 0; level := level_in, or the fourth-order begin's start rule on the cached (a0, j0): the level of dt_c = eta_start t, t = 1 / sqrt(k)
// of nbody_jerk_time's k = |j|^2 / |a|^2 (each squared norm (x x + y y) + z z; 0 / 0 = 0)
__global__ __launch_bounds__(kBlock) void hermite6_block_init_kernel(const double *__restrict__ ajs0, const int *__restrict__ level_in, int n,
                                                                     double eta_start, double dt_max, int levels, long long *__restrict__ T,
                                                                     int *__restrict__ level, unsigned long long *__restrict__ floor_hits) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T[i] = 0;
  if (level_in != nullptr) { level[i] = level_in[i]; return; }
  const Ajs s = load_ajs(ajs0, i);
  const double a2 = (s.a[0] * s.a[0] + s.a[1] * s.a[1]) + s.a[2] * s.a[2], j2 = (s.j[0] * s.j[0] + s.j[1] * s.j[1]) + s.j[2] * s.j[2];
  const double k = (j2 == 0.0 && a2 == 0.0) ? 0.0 : j2 / a2;
  const double dt_c = eta_start * time_of_k(k);
  int floor_hit;
  level[i] = hermite_block_level(dt_c, dt_max, levels, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
}

inline bool bad(const Hermite6BlockLaunch &L) {
  return L.n <= 0 || L.levels < 0 || L.levels > kHermiteBlockMaxLevels || !L.posm || !L.vel || !L.ajs0 || !L.a3 || !L.T || !L.level ||
         !L.list || !L.seg_min || !L.seg_cnt || !L.record || !L.floor_hits;
}

}  // namespace

hipError_t launch_hermite6_block_init(const Hermite6BlockLaunch &L, const int *level_in, double eta_start, hipStream_t s) {
  if (bad(L)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite6_block_init_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)L.ajs0, level_in,
                     L.n, eta_start, L.dt_max, L.levels, L.T, L.level, L.floor_hits);
  return hipGetLastError();
}

hipError_t launch_hermite6_block_schedule(const Hermite6BlockLaunch &L, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp || !L.ap) return hipErrorInvalidValue;
  int slots;
  const int seg_len = hermite_block_segment(L.n, &slots);
  if (hipError_t e = launch_hermite_block_next(L.T, L.level, L.n, L.levels, L.seg_min, L.seg_cnt, s)) return e;
  hipLaunchKernelGGL(hermite6_block_list_kernel<false>, dim3(slots), dim3(kBlock), 0, s, (const long long *)L.T, (const int *)L.level,
                     (const long long *)L.seg_min, (const int *)L.seg_cnt, slots, L.n, seg_len, L.levels, L.tick, (const double4 *)L.posm,
                     (const double4 *)L.vel, (const double *)L.ajs0, (const double4 *)L.a3, (double4 *)L.xp, (double4 *)L.vp,
                     (double4 *)L.ap, L.list, L.record, (const long long *)nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_hermite6_block_schedule_joint(const Hermite6BlockLaunch &B, const Hermite6BlockLaunch &P, hipStream_t s) {
  if (bad(B) || !B.xp || !B.vp || !B.ap || bad(P) || !P.xp || !P.vp || !P.ap || B.levels != P.levels || B.tick != P.tick)
    return hipErrorInvalidValue;
  int slots[2];
  const Hermite6BlockLaunch *set[2] = {&B, &P};
  for (const Hermite6BlockLaunch *L : set)
    if (hipError_t e = launch_hermite_block_next(L->T, L->level, L->n, L->levels, L->seg_min, L->seg_cnt, s)) return e;
  const int seg_len[2] = {hermite_block_segment(B.n, &slots[0]), hermite_block_segment(P.n, &slots[1])};
  for (int k = 0; k < 2; ++k) {
    const Hermite6BlockLaunch &L = *set[k], &O = *set[k ^ 1];
    hipLaunchKernelGGL(hermite6_block_list_kernel<true>, dim3(slots[k]), dim3(kBlock), 0, s, (const long long *)L.T, (const int *)L.level,
                       (const long long *)L.seg_min, (const int *)L.seg_cnt, slots[k], L.n, seg_len[k], L.levels, L.tick,
                       (const double4 *)L.posm, (const double4 *)L.vel, (const double *)L.ajs0, (const double4 *)L.a3, (double4 *)L.xp,
                       (double4 *)L.vp, (double4 *)L.ap, L.list, L.record, (const long long *)O.seg_min, slots[k ^ 1]);
  }
  return hipGetLastError();
}

hipError_t launch_hermite6_block_evaluate(const Hermite6BlockLaunch &L, int first, int m, int lanes, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp || !L.ap || !L.part || first < 0 || m <= 0 || first + m > L.n || (lanes != 1 && lanes != 2))
    return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n, &j_split, &j_chunk);
  if ((size_t)m > probe_slab_points(L.n, kSnapRowWidth)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  const dim3 grid((m + kBlock * lanes - 1) / (kBlock * lanes), j_split);
  const auto kernel = lanes == 1 ? (soft ? snap_tile_f64_kernel<true, 1, true> : snap_tile_f64_kernel<false, 1, true>)
                                 : (soft ? snap_tile_f64_kernel<true, 2, true> : snap_tile_f64_kernel<false, 2, true>);
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const double4 *)L.xp, (const double4 *)L.vp, (const double *)L.ap, 4,
                     (double *)L.part, L.n, m, 0, j_chunk, L.G, L.eps2, (const int *)L.list + first);
  return hipGetLastError();
}

hipError_t launch_hermite6_block_correct(const Hermite6BlockLaunch &L, int first, int m, long long t_next, hipStream_t s) {
  if (bad(L) || !L.acc || !L.a4 || !L.a5 || !L.part || first < 0 || m <= 0 || first + m > L.n) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_field > 0 ? L.n_field : L.n, &j_split, &j_chunk);   // (the rows' chunks are those of the bodies that exert the field)
  const Block6Rule r{L.tick, L.dt_max, L.eta, L.levels};
  hipLaunchKernelGGL(hermite6_block_correct_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const int *)L.list + first, m,
                     (const double *)L.part, j_split, t_next, r, L.T, L.level, (double4 *)L.posm, (double4 *)L.vel, (double4 *)L.acc, L.ajs0,
                     (double4 *)L.a3, (double4 *)L.a4, (double4 *)L.a5, L.floor_hits);
  return hipGetLastError();
}

}  // namespace nbody
