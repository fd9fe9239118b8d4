// Hermite block time steps of fp64 contexts (nbody_hermite_block_begin / _advance / _get; build-defined: the reference has one
// integrator and one step) — per-body power-of-two steps around an ACTIVE-SET form of the fp64 jerk pass.  Time is counted in integer
// ticks, tick = dt_max 2^-levels; body i is at T[i] with level k = level[i], its step 2^(levels - k) ticks.  One block step:
//   hermite_block_next_kernel     <- per segment of bodies (a workgroup each): the smallest T[i] + step_i and how many bodies attain it
//   hermite_block_list_kernel     <- T_next = the smallest of those; the bodies that attain it as a list in ascending body index — a
//                                    segment's place in the list from the counts of the segments before it, a body's place in its segment
//                                    by a ballot scan: no atomics, no order of arrival —; EVERY body predicted to T_next with its own dt
//   jerk_tile_f64_kernel<., ., true> (jerk_tile64.h)  <- (a1, j1) of the listed bodies against all predicted bodies: one partial row per
//                                    listed body and chunk, the chunks, the pair operations and their order those of nbody_get_jerk_f64
//   hermite_block_correct_kernel  <- the listed bodies: the chunks' rows added in chunk order (jerk_fold_f64_kernel's sums), the corrector
//                                    of kernels_hermite.hip with the body's own dt, T[i] := T_next, the new level (hermite_block_level.h)
//   hermite_block_init_kernel     <- T := 0 and the first levels, given or from eta_start |a| / |j|
// A session that carries fp64 tracers (nbody_hermite_block_begin_tracers) runs the same kernels on a second set of arrays, the tracers';
// hermite_block_list_kernel<true> then takes T_next over both sets, and the tracers' rows come from jerk_points_f64_kernel<., ., true>.
// EVERY operation outside the pair sums is one correctly rounded fp64 operation in the order written: contraction is off for the whole
// file, so that numpy (tests/hermite_block_ref.py) reproduces a block step in every bit.
#include "jerk_tile64.h"
#include "kernels.h"

#include "hermite_block_level.h"
#include "hermite_block_sched.h"

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

// a body's (ax, ay, az, jx, jy, jz): six doubles, 48 bytes apart — three 16-byte accesses
struct Aj { double a[3], j[3]; };
__device__ __forceinline__ Aj load_aj(const double *__restrict__ aj, int i) {
  const double2 *r = (const double2 *)(aj + 6 * (size_t)i);
  const double2 r0 = r[0], r1 = r[1], r2 = r[2];
  return Aj{{r0.x, r0.y, r1.x}, {r1.y, r2.x, r2.y}};
}

// record[0] = T_next, record[1] = m; list[0 .. m) ascending; per body and component, with dt = (double)(T_next - T[i]) tick,
// c2 = (dt dt) 0.5 and c3 = ((dt dt) dt) / 6:  xp = ((x + dt v) + c2 a0) + c3 j0;  vp = (v + dt a0) + c2 j0;  xp.w = m, vp.w = 0
// JOINT: T_next is the smallest due time of BOTH sets of a session that carries tracers — this set's segments and the other's
// (other_min[0 .. other_slots)) —; a set with nobody due at T_next writes m = 0 and an empty list.  <false> is the kernel it was.
template <bool JOINT>
__global__ __launch_bounds__(kBlock) void hermite_block_list_kernel(const long long *__restrict__ T, const int *__restrict__ level,
                                                                    const long long *__restrict__ seg_min, const int *__restrict__ seg_cnt,
                                                                    int slots, int n, int seg_len, int levels, double tick,
                                                                    const double4 *__restrict__ posm, const double4 *__restrict__ vel,
                                                                    const double *__restrict__ aj0, double4 *__restrict__ xp,
                                                                    double4 *__restrict__ vp, int *__restrict__ list,
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
      const double c2 = (dt * dt) * 0.5, c3 = ((dt * dt) * dt) / 6.0;
      const double4 x = posm[i], v = vel[i];
      const Aj a = load_aj(aj0, i);
      auto px = [&](double xc, double vc, double ac, double jc) { return ((xc + dt * vc) + c2 * ac) + c3 * jc; };
      auto pv = [&](double vc, double ac, double jc) { return (vc + dt * ac) + c2 * jc; };
      xp[i] = make_double4(px(x.x, v.x, a.a[0], a.j[0]), px(x.y, v.y, a.a[1], a.j[1]), px(x.z, v.z, a.a[2], a.j[2]), x.w);
      vp[i] = make_double4(pv(v.x, a.a[0], a.j[0]), pv(v.y, a.a[1], a.j[1]), pv(v.z, a.a[2], a.j[2]), 0.0);
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

// Aarseth's k of hermite_time_parts_kernel from one body's four vectors, and the step 1 / sqrt(k) it stands for: +inf for k == 0, 0 for
// a k that is not finite
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
__device__ __forceinline__ double time_of_k(double k) {
  if (k == 0.0) return __builtin_inf();
  if (!(k <= 0x1.fffffffffffffp1023)) return 0.0;
  return 1.0 / sqrt(k);
}

struct BlockRule { double tick, dt_max, root_eta; int levels; };

// One lane per listed body k < m, body i = list[k], dt = (double)(T_next - T[i]) tick — for a listed body exactly dt_max 2^-level —,
// ch = dt 0.5, c12 = (dt dt) / 12, d2 = dt dt, d3 = (dt dt) dt, (a1, j1) = the rows part[(c m + k) 6 ..] added in chunk order from 0:
//   v1 = v + (ch (a0 + a1) + c12 (j0 - j1));   x1 = x + (ch (v + v1) + c12 (a0 - a1));   da = a0 - a1
//   a2_0 = ((-6 da) - dt ((4 j0) + (2 j1))) / d2;   a3 = ((12 da) + (6 dt) (j0 + j1)) / d3;   a2_1 = a2_0 + dt a3
// x := x1, v := v1, acc := (a1, 0), (a0, j0) := (a1, j1), a2 := a2_1, a3 := a3, T := T_next; then the level: k = (J C + S S) / (A S + J J)
// of the NEW vectors, dt_c = root_eta / sqrt(k), kw = hermite_block_level(dt_c), level := hermite_block_next_level.  A body that no
// level fits adds one to *floor_hits (an integer count: the order of the additions does not show).
__global__ __launch_bounds__(kBlock) void hermite_block_correct_kernel(const int *__restrict__ list, int m, const double *__restrict__ part,
                                                                       int j_split, long long t_next, BlockRule r, long long *__restrict__ T,
                                                                       int *__restrict__ level, double4 *__restrict__ posm,
                                                                       double4 *__restrict__ vel, double4 *__restrict__ acc,
                                                                       double *__restrict__ aj0, double4 *__restrict__ a2,
                                                                       double4 *__restrict__ a3, unsigned long long *__restrict__ floor_hits) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  const int i = list[k];
  const double dt = (double)(t_next - T[i]) * r.tick;
  const double ch = dt * 0.5, c12 = (dt * dt) / 12.0, d2 = dt * dt, d3 = (dt * dt) * dt;
  double s1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) s1[q] = s1[q] + row[q];
  }
  const double4 x = posm[i], v = vel[i];
  const Aj s0 = load_aj(aj0, i);
  const double xc[3] = {x.x, x.y, x.z}, vc[3] = {v.x, v.y, v.z};
  double x1[3], v1[3], q2[3], q3[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double a1 = s1[q], j1 = s1[3 + q];
    v1[q] = vc[q] + (ch * (s0.a[q] + a1) + c12 * (s0.j[q] - j1));
    x1[q] = xc[q] + (ch * (vc[q] + v1[q]) + c12 * (s0.a[q] - a1));
    const double da = s0.a[q] - a1;
    const double a20 = ((-6.0 * da) - dt * ((4.0 * s0.j[q]) + (2.0 * j1))) / d2;
    q3[q] = ((12.0 * da) + (6.0 * dt) * (s0.j[q] + j1)) / d3;
    q2[q] = a20 + dt * q3[q];
  }
  posm[i] = make_double4(x1[0], x1[1], x1[2], x.w);
  vel[i] = make_double4(v1[0], v1[1], v1[2], v.w);
  acc[i] = make_double4(s1[0], s1[1], s1[2], 0.0);
  double2 *row0 = (double2 *)(aj0 + 6 * (size_t)i);
  row0[0] = make_double2(s1[0], s1[1]); row0[1] = make_double2(s1[2], s1[3]); row0[2] = make_double2(s1[4], s1[5]);
  a2[i] = make_double4(q2[0], q2[1], q2[2], 0.0);
  a3[i] = make_double4(q3[0], q3[1], q3[2], 0.0);
  T[i] = t_next;

  const double A = norm3(s1[0], s1[1], s1[2]), J = norm3(s1[3], s1[4], s1[5]), S = norm3(q2[0], q2[1], q2[2]), C = norm3(q3[0], q3[1], q3[2]);
  const double num = J * C + S * S, den = A * S + J * J;
  const double kk = (num == 0.0 && den == 0.0) ? 0.0 : num / den;
  const double dt_c = r.root_eta * time_of_k(kk);
  int floor_hit;
  const int kw = hermite_block_level(dt_c, r.dt_max, r.levels, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
  level[i] = hermite_block_next_level(level[i], kw, t_next, r.levels);
}

// T := 0; level := level_in, or the level of dt_c = eta_start t, t = 1 / sqrt(k) of nbody_jerk_time's k = |j|^2 / |a|^2 (each squared norm
// (x x + y y) + z z; 0 / 0 = 0)
__global__ __launch_bounds__(kBlock) void hermite_block_init_kernel(const double *__restrict__ aj0, const int *__restrict__ level_in, int n,
                                                                    double eta_start, double dt_max, int levels, long long *__restrict__ T,
                                                                    int *__restrict__ level, unsigned long long *__restrict__ floor_hits) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T[i] = 0;
  if (level_in != nullptr) { level[i] = level_in[i]; return; }
  const Aj s = load_aj(aj0, i);
  const double a2 = (s.a[0] * s.a[0] + s.a[1] * s.a[1]) + s.a[2] * s.a[2], j2 = (s.j[0] * s.j[0] + s.j[1] * s.j[1]) + s.j[2] * s.j[2];
  const double k = (j2 == 0.0 && a2 == 0.0) ? 0.0 : j2 / a2;
  const double dt_c = eta_start * time_of_k(k);
  int floor_hit;
  level[i] = hermite_block_level(dt_c, dt_max, levels, &floor_hit);
  if (floor_hit) atomicAdd(floor_hits, 1ull);
}

inline bool bad(const HermiteBlockLaunch &L) {
  return L.n <= 0 || L.levels < 0 || L.levels > kHermiteBlockMaxLevels || !L.posm || !L.vel || !L.aj0 || !L.T || !L.level || !L.list ||
         !L.seg_min || !L.seg_cnt || !L.record || !L.floor_hits;
}

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

hipError_t launch_hermite_block_init(const HermiteBlockLaunch &L, const int *level_in, double eta_start, hipStream_t s) {
  if (bad(L)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hermite_block_init_kernel, dim3((L.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, L.aj0, level_in, L.n, eta_start,
                     L.dt_max, L.levels, L.T, L.level, L.floor_hits);
  return hipGetLastError();
}

hipError_t launch_hermite_block_next(const long long *T, const int *level, int n, int levels, long long *seg_min, int *seg_cnt,
                                     hipStream_t s) {
  if (n <= 0 || levels < 0 || levels > kHermiteBlockMaxLevels || !T || !level || !seg_min || !seg_cnt) return hipErrorInvalidValue;
  int slots;
  const int seg_len = hermite_block_segment(n, &slots);
  hipLaunchKernelGGL(hermite_block_next_kernel, dim3(slots), dim3(kBlock), 0, s, T, level, n, seg_len, levels, seg_min, seg_cnt);
  return hipGetLastError();
}

hipError_t launch_hermite_block_schedule(const HermiteBlockLaunch &L, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp) return hipErrorInvalidValue;
  int slots;
  const int seg_len = hermite_block_segment(L.n, &slots);
  if (hipError_t e = launch_hermite_block_next(L.T, L.level, L.n, L.levels, L.seg_min, L.seg_cnt, s)) return e;
  hipLaunchKernelGGL(hermite_block_list_kernel<false>, dim3(slots), dim3(kBlock), 0, s, (const long long *)L.T, (const int *)L.level,
                     (const long long *)L.seg_min, (const int *)L.seg_cnt, slots, L.n, seg_len, L.levels, L.tick, (const double4 *)L.posm,
                     (const double4 *)L.vel, (const double *)L.aj0, (double4 *)L.xp, (double4 *)L.vp, L.list, L.record,
                     (const long long *)nullptr, 0);
  return hipGetLastError();
}

hipError_t launch_hermite_block_schedule_joint(const HermiteBlockLaunch &B, const HermiteBlockLaunch &P, hipStream_t s) {
  if (bad(B) || !B.xp || !B.vp || bad(P) || !P.xp || !P.vp || B.levels != P.levels || B.tick != P.tick) return hipErrorInvalidValue;
  int slots[2];
  const HermiteBlockLaunch *set[2] = {&B, &P};
  for (const HermiteBlockLaunch *L : set)
    if (hipError_t e = launch_hermite_block_next(L->T, L->level, L->n, L->levels, L->seg_min, L->seg_cnt, s)) return e;
  const int seg_len[2] = {hermite_block_segment(B.n, &slots[0]), hermite_block_segment(P.n, &slots[1])};
  for (int k = 0; k < 2; ++k) {
    const HermiteBlockLaunch &L = *set[k], &O = *set[k ^ 1];
    hipLaunchKernelGGL(hermite_block_list_kernel<true>, dim3(slots[k]), dim3(kBlock), 0, s, (const long long *)L.T, (const int *)L.level,
                       (const long long *)L.seg_min, (const int *)L.seg_cnt, slots[k], L.n, seg_len[k], L.levels, L.tick,
                       (const double4 *)L.posm, (const double4 *)L.vel, (const double *)L.aj0, (double4 *)L.xp, (double4 *)L.vp, L.list,
                       L.record, (const long long *)O.seg_min, slots[k ^ 1]);
  }
  return hipGetLastError();
}

hipError_t launch_hermite_block_evaluate(const HermiteBlockLaunch &L, int first, int m, int lanes, hipStream_t s) {
  if (bad(L) || !L.xp || !L.vp || !L.part || first < 0 || m <= 0 || first + m > L.n || (lanes != 1 && lanes != 2)) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n, &j_split, &j_chunk);
  if ((size_t)m > probe_slab_points(L.n, 3)) return hipErrorInvalidValue;
  const bool soft = L.eps2 > 0.0;
  const dim3 grid((m + kBlock * lanes - 1) / (kBlock * lanes), j_split);
  const auto kernel = lanes == 1 ? (soft ? jerk_tile_f64_kernel<true, 1, true> : jerk_tile_f64_kernel<false, 1, true>)
                                 : (soft ? jerk_tile_f64_kernel<true, 2, true> : jerk_tile_f64_kernel<false, 2, true>);
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, (const double4 *)L.xp, (const double4 *)L.vp, (double *)L.part, L.n, m, 0, j_chunk,
                     L.G, L.eps2, (const int *)L.list + first);
  return hipGetLastError();
}

hipError_t launch_hermite_block_correct(const HermiteBlockLaunch &L, int first, int m, long long t_next, hipStream_t s) {
  if (bad(L) || !L.acc || !L.a2 || !L.a3 || !L.part || first < 0 || m <= 0 || first + m > L.n) return hipErrorInvalidValue;
  int j_split, j_chunk;
  probe_geometry(L.n_field > 0 ? L.n_field : L.n, &j_split, &j_chunk);   // (the rows' chunks are those of the bodies that exert the field)
  const BlockRule r{L.tick, L.dt_max, L.root_eta, L.levels};
  hipLaunchKernelGGL(hermite_block_correct_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const int *)L.list + first, m,
                     (const double *)L.part, j_split, t_next, r, L.T, L.level, (double4 *)L.posm, (double4 *)L.vel, (double4 *)L.acc, L.aj0,
                     (double4 *)L.a2, (double4 *)L.a3, L.floor_hits);
  return hipGetLastError();
}

}  // namespace nbody
