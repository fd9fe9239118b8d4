// Internal launcher interface between the C-ABI (capi.hip) and the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbody {

struct ForceLaunch {
  const void *posm;     // [n_total] float4 / double4 : x,y,z,m
  void *accp;           // [j_split][i_count] float4 / double4 partial accelerations
  int n_total;
  int i_begin;
  int i_count;
  int tile;             // LDS tile, bodies
  int ipt;              // i-bodies per lane
  int j_split;          // number of j chunks
  int j_chunk;          // bodies per chunk (multiple of tile)
  double G;
  double eps2;          // > 0: softened (also the "floor" mode); == 0: exact d == 0 skip
  int zero_mode;        // for eps2 == 0: 1 = clamp trick (default), 2 = compare+select (A/B only)
  int precision;        // NBODY_PREC_*
  int wave;             // 0: tile kernels; 2 ... 8: forces_block_pk_kernel (kernels_block.hip), a workgroup per `wave` register
                        // pairs of bodies, its lanes split the j range (j_split must be 1)
  int uni = 0;          // wave >= 2: 1 = the caller knows that every body has body 0's mass (equal-mass form only), 0 = it knows they
                        // do not (general form only), -1 = launch both, each looks at `general`
  int guarded = 0;      // wave >= 2: guard every pair (no optimistic bare pass)
  void *dup_table = nullptr;   // packed fp32 kernel, exact mode: coincident-body detector's table [dup_slots] + {flag, count};
  int dup_slots = 0;           // with it, tiles that hold no self pair run without the d == 0 guard when no two bodies coincide
  // packed fp32 kernel: device int that is 0 when every body has body 0's mass (equal-mass form: no mass factor in the
  // pair loop); nullptr = general form only.  check_masses: run mass_check_kernel on the positions first (somebody else
  // may have written the buffer since the host last looked).
  void *general = nullptr;
  int check_masses = 0;
  void *clk = nullptr;  // packed fp32 tile kernel: two device uint64 the workgroups add their shader-clock / reference-clock intervals to (pk_common.h)
};

// All-pairs force partials.  Returns hipSuccess or the launch error.
hipError_t launch_forces(const ForceLaunch &L, hipStream_t s);
// Small and mid-size single-context fp32 systems (L.wave != 0): the whole Tick body — forces, v += dt*a, x += dt*v — in one launch.
// New positions go to posm_out (a second buffer: the old one is still being read); the caller swaps them afterwards.
// stage / size_bits / size_zero (optional): see BlockLaunch — the frame's FParticle mirror and ComputeCubeSize from the same launch.
hipError_t launch_step_small(const ForceLaunch &L, void *posm_out, void *vel, void *acc, float dt, hipStream_t s,
                             void *stage = nullptr, void *size_bits = nullptr, void *size_zero = nullptr);
// Blocks / threads launch_forces will use for L (for logs).
void forces_geometry(const ForceLaunch &L, int *blocks, int *threads);

// Small and mid-size fp32 systems — kernels_block.hip: a workgroup owns `np` register pairs of bodies and its lanes split
// the j range; a body's whole sum is finished inside its workgroup, so with dt > 0 the Tick's update rides along (new
// positions into posm_out) and a step is one launch with no partial rows.
struct BlockLaunch {
  const void *posm = nullptr;   // [n_total] float4, read only
  void *posm_out = nullptr;     // dt > 0: [n_total] float4, the owned bodies' new (x, y, z, m); must not be posm
  void *vel = nullptr;          // dt > 0: [i_count] float4
  void *acc = nullptr;          // [i_count] float4
  int n_total = 0, i_begin = 0, i_count = 0;
  int np = 2;                   // register pairs per workgroup: 2 ... 8
  double G = 0.0, eps2 = 0.0;   // eps2 > 0 softened (also the floor mode); == 0 exact d == 0 skip
  float dt = 0.f;               // <= 0: accelerations only
  int uni = 0;                  // 1: every body has body 0's mass (the caller knows): no mass factor in the pair loop; 0: general form;
                                // -1: both forms are launched and *general (0 = equal masses) says which one runs
  const void *general = nullptr;
  // dt > 0, optional (the actor's frame in one launch): FParticle records of the owned bodies after the update (10 floats
  // each); a pre-zeroed word for the bit pattern of ComputeCubeSize over the positions before the update, and a second
  // word this launch clears for the next frame
  void *stage = nullptr;
  void *size_bits = nullptr, *size_zero = nullptr;
  int optimistic = 1;           // eps2 == 0: bare pair law outside the own group first, guarded walk only where a sum came out non-finite
};
hipError_t launch_block(const BlockLaunch &L, hipStream_t s);

// acc[i] = sum_c accp[c][i] in chunk order; if dt > 0 also v += dt*a; x += dt*v (owned slice of posm).
hipError_t launch_update(int precision, void *posm, void *vel, void *acc, const void *accp, int i_begin,
                         int i_count, int j_split, float dt, hipStream_t s);

// The bodies' field at `m` massless points, theta = 0 — kernels_probe.hip: acc[k] = sum over all n_total bodies of the pair law at
// probe[k], partial rows per j chunk added in chunk order.  The chunks follow from n_total alone (probe_geometry), so a point's bits
// do not depend on the other points, on m or on the device.  dt > 0: the points are tracers — v += dt*a; x += dt*v on (pos_out, vel)
// behind the sums, as the bodies get it (pos_out may be `probe` itself: a slab's positions are read before they are written).
constexpr size_t kProbePartBytes = 256u << 20;   // the partial rows' staging area at most: larger queries go in slabs of points
struct ProbeLaunch {
  const void *posm = nullptr;   // [n_total] float4: x, y, z, m
  const void *probe = nullptr;  // [m] float4: x, y, z, unused
  void *part = nullptr;         // [probe_part_elems(n_total, m)] float4: partial rows of one slab
  void *acc = nullptr;          // [m] float4
  void *pos_out = nullptr, *vel = nullptr;   // dt > 0: [m] float4 each
  int n_total = 0, m = 0;
  double G = 0.0, eps2 = 0.0;   // eps2 > 0 softened (also the floor mode); == 0 exact d == 0 skip (clamp form)
  float dt = 0.f;
  void *clk = nullptr;          // two device uint64 the workgroups add their clock intervals to (pk_common.h)
};
void probe_geometry(int n_total, int *j_split, int *j_chunk);
// width: the float4 a point has in a chunk's partial row at most (1: the field, the potential; 2: the tidal tensor, the jerk; 3: the fp64 jerk; 4: the fp64 tidal tensor)
size_t probe_slab_points(int n_total, int width = 1);         // points whose partial rows fit kProbePartBytes (a multiple of 1024)
inline size_t probe_part_elems(int n_total, int m, int width = 1) {   // float4 elements `part` must hold for a launch of m points
  int js, jc;
  probe_geometry(n_total, &js, &jc);
  const size_t slab = probe_slab_points(n_total, width);
  return (size_t)js * ((size_t)m < slab ? (size_t)m : slab) * (size_t)width;
}
hipError_t launch_probe(const ProbeLaunch &L, hipStream_t s);

// The bodies' potential at theta = 0 — kernels_probe.hip: phi[k] = -sum_j G m_j / sqrt(|probe[k] - x_j|^2 + eps2) over all n_total bodies:
// fp32 terms, one fused chain per chunk of probe_geometry in body order, the chunks' rows added in chunk order in fp64, negated.  With
// eps2 == 0 a pair at distance 0 adds nothing.  probe == nullptr: the points are the bodies themselves (m == n_total) and every body
// leaves itself out by index.  phi64 gets the fp64 value, phif the value rounded once; either may be null.
struct PotLaunch {
  const void *posm = nullptr;   // [n_total] float4: x, y, z, m
  const void *probe = nullptr;  // [m] float4: x, y, z, unused; nullptr: posm
  void *part = nullptr;         // the staging area of ProbeLaunch::part (one float per point and chunk of a slab: a quarter of it)
  double *phi64 = nullptr;      // [m]
  float *phif = nullptr;        // [m]
  int n_total = 0, m = 0;
  double G = 0.0, eps2 = 0.0;
  void *clk = nullptr;
};
hipError_t launch_pot(const PotLaunch &L, hipStream_t s);
// out[0] = sum_i 1/2 m_i v_i^2, out[1] = sum_i 1/2 m_i phi64[i] over n bodies (fp32 posm / vel), in a fixed order: per-workgroup pairs
// into `partials` (2 * energy_fast_slots(n) doubles), then one workgroup folds them — no atomics, reproducible bits.
constexpr int kEnergyFastSlots = 1024;
int energy_fast_slots(int n);
hipError_t launch_energy_fast(const void *posm, const void *vel, const double *phi64, int n, double *partials, double *out, hipStream_t s);

// The bodies' tidal tensor at theta = 0 — kernels_probe.hip: T_ab(x) = sum_j G m_j [3 d_a d_b / s^5 - delta_ab / s^3], d = x_j - x,
// s^2 = |d|^2 + eps2, over all n_total bodies.  Seven fp32 sums per point and chunk of probe_geometry — S_ab = sum (3 G m / s^3)(d_a / s)
// (d_b / s), Q = sum G m / s^3, no s^-5 anywhere —, each one fused chain in body order; a partial row is two float4 per point
// (probe_slab_points(n_total, 2)).  The chunks' rows are added in chunk order in fp64, T_aa = S_aa - Q there: t64 gets the six doubles
// (xx, yy, zz, xy, xz, yz), tf the same rounded once; either may be null.  With eps2 == 0 a pair at distance 0 adds nothing.
// probe == nullptr: the points are the bodies themselves (m == n_total) and every body leaves itself out by index.
struct TidalLaunch {
  const void *posm = nullptr;   // [n_total] float4: x, y, z, m
  const void *probe = nullptr;  // [m] float4: x, y, z, unused; nullptr: posm
  void *part = nullptr;         // [probe_part_elems(n_total, m, 2)] float4
  double *t64 = nullptr;        // [m][6]
  float *tf = nullptr;          // [m][6]
  int n_total = 0, m = 0;
  double G = 0.0, eps2 = 0.0;
  void *clk = nullptr;
};
hipError_t launch_tidal(const TidalLaunch &L, hipStream_t s);
// out[0] = max over the n bodies of n2 = (Txx^2 + Tyy^2) + Tzz^2 + 2 ((Txy^2 + Txz^2) + Tyz^2) from t64 (a value that is not finite counts
// as +inf), out[1] = the lowest index that attains it, as a double: per-workgroup pairs into `partials` (2 * energy_fast_slots(n) doubles),
// then one workgroup folds them — a fixed order, no atomics.
hipError_t launch_tidal_time(const double *t64, int n, double *partials, double *out, hipStream_t s);
// that fold on its own, for every reduction that leaves (value, index as a double) pairs of this kind in `partials`: out[0] = the largest
// value of partials[2 q], q < slots, out[1] = the lowest index partials[2 q + 1] that attains it — one workgroup, a fixed order
hipError_t launch_max_fold(const double *partials, int slots, double *out, hipStream_t s);

// The jerk j = da/dt beside the acceleration, a pair sum over all n_total bodies at every theta — kernels_jerk.hip: with d = x_j - x,
// w = v_j - v, s^2 = |d|^2 + eps2:  a = sum_j G m_j d / s^3,  j = sum_j G m_j [w / s^3 - 3 (d . w) d / s^5].  With eps2 == 0 a pair at
// distance 0 adds nothing to either sum.  probe == nullptr: the points are the bodies themselves (m == n_total, their velocities `vel`)
// and every body leaves itself out by index.
//   fp32 state (NBODY_PREC_F32, NBODY_PREC_F32_KAHAN): six fp32 sums per point and chunk of probe_geometry, each one fused chain in body
//     order on the potential's distance term, no s^-5 anywhere; a partial row is two float4 per point (probe_slab_points(n_total, 2)); the
//     chunks' rows are added in chunk order in fp64.
//   fp64 state (NBODY_PREC_F64; the bodies only): the same sums in fp64, a partial row six doubles per body (probe_slab_points(n_total, 3)).
// aj64 gets six doubles per point (ax, ay, az, jx, jy, jz), ajf the same rounded once; either may be null.
struct JerkLaunch {
  const void *posm = nullptr;   // [n_total] float4 / double4: x, y, z, m
  const void *vel = nullptr;    // [n_total] float4 / double4: vx, vy, vz, unused
  const void *probe = nullptr;  // [m] float4: x, y, z, unused; nullptr: posm
  const void *pvel = nullptr;   // [m] float4: the points' velocities (probe != nullptr)
  void *part = nullptr;         // [probe_part_elems(n_total, m, 2)] float4; fp64 state: [probe_part_elems(n_total, m, 3)]
  double *aj64 = nullptr;       // [m][6]
  float *ajf = nullptr;         // [m][6]
  int n_total = 0, m = 0;
  int precision = 0;            // NBODY_PREC_*
  double G = 0.0, eps2 = 0.0;
};
hipError_t launch_jerk(const JerkLaunch &L, hipStream_t s);
// out[0] = max over the n bodies of k = |j|^2 / |a|^2 from aj64, each squared norm (x x + y y) + z z (0 / 0 counts as 0, x / 0 and every
// value that is not finite as +inf), out[1] = the lowest index that attains it, as a double: launch_tidal_time's reduction.
hipError_t launch_jerk_time(const double *aj64, int n, double *partials, double *out, hipStream_t s);

// Fourth-order Hermite stepping of an fp64 state — kernels_hermite.hip: the predictor and the corrector around one launch_jerk on the
// predicted state (the caller's to queue in between), one lane per body, every operation one correctly rounded fp64 operation.
//   launch_hermite_predict: xp = ((x + dt v) + c2 a0) + c3 j0, vp = (v + dt a0) + c2 j0 per component; xp.w = m, vp.w = 0
//   launch_hermite_correct: (x, v) := the corrected state from (a0, j0) and (a1, j1), acc := (a1, 0), (a2, a3) := the second and third
//     derivative of a at the new time
// aj0 / aj1 are launch_jerk's rows, six doubles per body (ax, ay, az, jx, jy, jz).
struct HermiteLaunch {
  void *posm = nullptr, *vel = nullptr, *acc = nullptr;   // [n] double4 each: the live state (predict reads posm and vel)
  void *xp = nullptr, *vp = nullptr;                      // [n] double4 each: the predicted state
  const double *aj0 = nullptr, *aj1 = nullptr;            // [n][6]: (a, j) at the stored state / at the predicted one
  void *a2 = nullptr, *a3 = nullptr;                      // [n] double4 each
  int n = 0;
  double dt = 0.0;
};
hipError_t launch_hermite_predict(const HermiteLaunch &L, hipStream_t s);
hipError_t launch_hermite_correct(const HermiteLaunch &L, hipStream_t s);
// out[0] = max over the n bodies of Aarseth's k = (|j| |a3| + |a2|^2) / (|a| |a2| + |j|^2), norms sqrt((x x + y y) + z z) (0 / 0 counts
// as 0, x / 0 and every value that is not finite as +inf), out[1] = the lowest index that attains it, as a double: launch_jerk_time's
// reduction and its `partials`.
hipError_t launch_hermite_time(const double *aj0, const void *a2, const void *a3, int n, double *partials, double *out, hipStream_t s);

// Hermite block time steps of an fp64 state — kernels_hermite_block.hip: per-body times T (ticks of dt_max 2^-levels) and levels, a
// scheduler that lists the bodies due next in ascending index and predicts EVERY body to that time, the fp64 jerk pass on the listed
// bodies alone (deriv_tile64.h: nbody_get_jerk_f64's chunks, pair operations and order), and a corrector for the listed bodies that adds
// the chunks' rows, steps the body by its own dt and chooses its next level (hermite_block_level.h).
//   launch_hermite_block_init:      T := 0; level := level_in (device, may be null: the level of eta_start |a| / |j| from aj0)
//   launch_hermite_block_schedule:  record[0] = T_next, record[1] = m, list[0 .. m) ascending, (xp, vp) = every body at T_next
//   launch_hermite_block_evaluate:  the rows of list[first .. first + m) into part, m <= probe_slab_points(n, 3); lanes = bodies per lane
//   launch_hermite_block_correct:   those bodies corrected from part (the rows of that launch), their T, level, cache and state stored
// what both orders' sessions hold (HermiteBlockLaunch, Hermite6BlockLaunch): the state, the scheduler's arrays and the session's rule
struct HermiteBlockBase {
  void *posm = nullptr, *vel = nullptr, *acc = nullptr;   // [n] double4 each: the live state
  void *xp = nullptr, *vp = nullptr;                      // [n] double4 each: the predicted state
  void *part = nullptr;                                   // the evaluation's partial rows: [probe_part_elems(n, m, row width)] float4
  long long *T = nullptr;                                 // [n] ticks
  int *level = nullptr, *list = nullptr;                  // [n] each
  long long *seg_min = nullptr;                           // [slots of hermite_block_segment]
  int *seg_cnt = nullptr;                                 // [slots]
  long long *record = nullptr;                            // [2]: T_next, m
  unsigned long long *floor_hits = nullptr;               // [1]: bodies clamped to the deepest level since the session began
  int n = 0, levels = 0;
  int n_field = 0;   // the tracers' arrays: the bodies whose chunks (probe_geometry) the partial rows follow; 0: n
  double tick = 0.0, dt_max = 0.0, G = 0.0, eps2 = 0.0;
};
struct HermiteBlockLaunch : HermiteBlockBase {
  static constexpr int kRow = 6;                          // the doubles of a cached row
  double *aj0 = nullptr;                                  // [n][6]: every body's (a, j) at its own time
  void *a2 = nullptr, *a3 = nullptr;                      // [n] double4 each
  double root_eta = 0.0;
};
constexpr int kHermiteBlockOneLaneMax = 1024;   // listed bodies up to which the evaluation holds one body per lane (more workgroups)
int hermite_block_segment(int n, int *slots);   // bodies per scheduler workgroup (a multiple of 256); *slots = the workgroups
int hermite_block_lanes(int m, int forced);     // bodies per lane for m listed bodies; forced 1 or 2 overrides (A/B runs, tests)
hipError_t launch_hermite_block_init(const HermiteBlockLaunch &L, const int *level_in, double eta_start, hipStream_t s);
hipError_t launch_hermite_block_schedule(const HermiteBlockLaunch &L, hipStream_t s);
hipError_t launch_hermite_block_evaluate(const HermiteBlockLaunch &L, int first, int m, int lanes, hipStream_t s);
hipError_t launch_hermite_block_correct(const HermiteBlockLaunch &L, int first, int m, long long t_next, hipStream_t s);
// the schedule of a session that carries fp64 tracers — B the bodies' arrays, P the tracers' —: T_next is the smallest due time of
// BOTH sets; each set gets its own record (T_next, m: 0 and an empty list where nobody is due) and every row of both is predicted
hipError_t launch_hermite_block_schedule_joint(const HermiteBlockLaunch &B, const HermiteBlockLaunch &P, hipStream_t s);
// the schedule's first kernel alone — seg_min[q], seg_cnt[q] of every segment q: the smallest T[i] + step_i and how many bodies attain it —,
// which the sixth-order session queues ahead of a list kernel of its own (integers only: it reads no cache)
hipError_t launch_hermite_block_next(const long long *T, const int *level, int n, int levels, long long *seg_min, int *seg_cnt, hipStream_t s);

// The snap s = d^2 a / dt^2 beside the acceleration and the jerk of an fp64 state, the bodies only — kernels_snap.hip: with d = x_j - x_i,
// w = v_j - v_i, b = ain_j - ain_i (ain: a per-body INPUT acceleration), s^2 = |d|^2 + eps2, t = 1 / s, al = (d . w) t^2,
// be = (w . w + d . b) t^2 + al^2:  A = G m_j d t^3,  J = G m_j w t^3 - 3 al A,  S = G m_j b t^3 - 6 al J - 3 be A, summed over j != i.
// The chunks, tiles, rsq, zero rule and — up to A and J — the per-pair operations are launch_jerk's on fp64 state, so a body's a and j
// are launch_jerk's in every bit whatever ain holds.  A partial row is nine doubles per body: probe_slab_points(n_total, kSnapRowWidth).
constexpr int kSnapRowWidth = 5;   // the float4 that hold nine doubles
struct SnapLaunch {
  const void *posm = nullptr;   // [n_total] double4: x, y, z, m
  const void *vel = nullptr;    // [n_total] double4: vx, vy, vz, unused
  const double *ain = nullptr;  // body i's input acceleration: ain[i * ain_stride + 0 .. 2]
  int ain_stride = 0;           // in doubles, >= 3 (4: double4 rows; 6: launch_jerk's aj64)
  void *part = nullptr;         // [probe_part_elems(n_total, n_total, kSnapRowWidth)] float4
  double *ajs64 = nullptr;      // [n_total][9]: ax, ay, az, jx, jy, jz, sx, sy, sz
  int n_total = 0;
  double G = 0.0, eps2 = 0.0;
};
hipError_t launch_snap(const SnapLaunch &L, hipStream_t s);

// Sixth-order Hermite stepping of an fp64 state (Nitadori & Makino) — kernels_snap.hip: the predictor and the corrector around one
// launch_snap on the predicted state with the predicted accelerations as its input (the caller's to queue in between), one lane per
// body, every operation one correctly rounded fp64 operation.
//   launch_hermite6_predict: (xp, vp, ap) = the Taylor series of x, v, a to a3 (fifth, fourth, third order in dt); xp.w = m, vp.w = ap.w = 0
//   launch_hermite6_correct: (x, v) := the corrected state from (a0, j0, s0) and (a1, j1, s1), acc := (a1, 0), (a3, a4, a5) := the third
//     to fifth derivative of a at the new time, from the quintic through both ends
// ajs0 / ajs1 are launch_snap's rows, nine doubles per body.
struct Hermite6Launch {
  void *posm = nullptr, *vel = nullptr, *acc = nullptr;   // [n] double4 each: the live state (predict reads posm and vel)
  void *xp = nullptr, *vp = nullptr, *ap = nullptr;       // [n] double4 each: the predicted state and its predicted accelerations
  const double *ajs0 = nullptr, *ajs1 = nullptr;          // [n][9]: (a, j, s) at the stored state / at the predicted one
  void *a3 = nullptr, *a4 = nullptr, *a5 = nullptr;       // [n] double4 each (predict reads a3)
  int n = 0;
  double dt = 0.0;
};
hipError_t launch_hermite6_predict(const Hermite6Launch &L, hipStream_t s);
hipError_t launch_hermite6_correct(const Hermite6Launch &L, hipStream_t s);
// out[0] = max over the n bodies of k = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2), norms sqrt((x x + y y) + z z) — derivs == false:
// launch_jerk_time's k = |j0|^2 / |a0|^2 — (0 / 0 counts as 0, x / 0 and every value that is not finite as +inf), out[1] = the lowest
// index that attains it, as a double: launch_jerk_time's reduction and its `partials`.
hipError_t launch_hermite6_time(const double *ajs0, const void *a3, const void *a4, const void *a5, int n, bool derivs, double *partials,
                                double *out, hipStream_t s);

// Sixth-order Hermite block time steps of an fp64 state — kernels_hermite_block.hip: HermiteBlockLaunch's times, levels, segments and
// scheduler around the ACTIVE-SET form of the snap pass (deriv_tile64.h: nbody_get_snap_f64's chunks, pair operations and order) and the
// sixth-order predictor and corrector with a dt per body; the level rule is hermite6_block_level (hermite_block_level.h).
//   launch_hermite6_block_init:      T := 0; level := level_in (device, may be null: the level of eta_start |a0| / |j0| from ajs0)
//   launch_hermite6_block_schedule:  record[0] = T_next, record[1] = m, list[0 .. m) ascending, (xp, vp, ap) = every body at T_next
//   launch_hermite6_block_evaluate:  the rows of list[first .. first + m) into part, m <= probe_slab_points(n, kSnapRowWidth)
//   launch_hermite6_block_correct:   those bodies corrected from part (the rows of that launch), their T, level, cache and state stored
struct Hermite6BlockLaunch : HermiteBlockBase {
  static constexpr int kRow = 9;                          // the doubles of a cached row
  void *ap = nullptr;                                     // [n] double4: the predicted accelerations
  double *ajs0 = nullptr;                                 // [n][9]: every body's (a, j, s) at its own time
  void *a3 = nullptr, *a4 = nullptr, *a5 = nullptr;       // [n] double4 each
  double eta = 0.0;
};
hipError_t launch_hermite6_block_init(const Hermite6BlockLaunch &L, const int *level_in, double eta_start, hipStream_t s);
hipError_t launch_hermite6_block_schedule(const Hermite6BlockLaunch &L, hipStream_t s);
hipError_t launch_hermite6_block_evaluate(const Hermite6BlockLaunch &L, int first, int m, int lanes, hipStream_t s);
hipError_t launch_hermite6_block_correct(const Hermite6BlockLaunch &L, int first, int m, long long t_next, hipStream_t s);
// the schedule of a session that carries fp64 tracers — B the bodies' arrays, P the tracers' —: T_next is the smallest due time of
// BOTH sets; each set gets its own record (T_next, m: 0 and an empty list where nobody is due) and every row of both is predicted
hipError_t launch_hermite6_block_schedule_joint(const Hermite6BlockLaunch &B, const Hermite6BlockLaunch &P, hipStream_t s);

// The fp64 jerk and snap passes at m points that are not bodies — kernels_points64.hip: launch_jerk's / launch_snap's pair sums on fp64
// state with the i side taken from (ppos, pvel[, pain]) instead of from the bodies, over the same chunks and tiles in the same order,
// but with NO pair dropped by index: t = (s2 > 0) ? rsq(s2) : 0.  eps2 == 0: a point exactly on a body drops that pair; eps2 > 0: that
// pair adds G m w / eps^3 to the jerk, G m b / eps^3 to the snap and nothing to a.  A point's sums depend on the point and the bodies
// alone (not on m, the other points, the slab or the points per lane); a zero-mass body adds exactly nothing.  The points go in slabs
// of probe_slab_points(n_total, 3) (kSnapRowWidth: the snap); the rows are folded by launch_jerk_fold_f64 / launch_snap_fold_f64.
struct Points64Launch {
  const void *posm = nullptr;   // [n_total] double4: x, y, z, m
  const void *vel = nullptr;    // [n_total] double4: vx, vy, vz, unused
  const double *ain = nullptr;  // the snap: body j's input acceleration, ain[j * ain_stride + 0 .. 2]
  int ain_stride = 0;           // in doubles, >= 3
  const void *ppos = nullptr;   // [m] double4: x, y, z, unused
  const void *pvel = nullptr;   // [m] double4: vx, vy, vz, unused
  const double *pain = nullptr; // the snap: point k's input acceleration, pain[k * pain_stride + 0 .. 2]
  int pain_stride = 0;          // in doubles, >= 3 (4: double4 rows; 6: the jerk's rows)
  void *part = nullptr;         // the partial rows of one slab
  size_t part_elems = 0;        // the float4 `part` holds: at least probe_part_elems(n_total, m, 3 / kSnapRowWidth), or nothing is launched
  double *out = nullptr;        // [m][6]: ax, ay, az, jx, jy, jz — the snap: [m][9], sx, sy, sz behind them
  int n_total = 0, m = 0;
  int lanes = 0;                // points per lane: 1 or 2; 0: hermite_block_lanes(m, 0).  It enters no sum.
  double G = 0.0, eps2 = 0.0;
};
hipError_t launch_jerk_points_f64(const Points64Launch &L, hipStream_t s);
hipError_t launch_snap_points_f64(const Points64Launch &L, hipStream_t s);
// The list forms, for a block step's active tracers: point k < m is row list[k] of (ppos, pvel[, pain]); ONE slab (m <=
// probe_slab_points(n_total, 3 / kSnapRowWidth)) into part[(c * m + k) * 6 / 9], left unfolded for the block corrector; `out` is not
// used, lanes is 1 or 2.
hipError_t launch_jerk_points_list_f64(const Points64Launch &L, const int *list, hipStream_t s);
hipError_t launch_snap_points_list_f64(const Points64Launch &L, const int *list, hipStream_t s);
// jerk_fold_f64_kernel / snap_fold_f64_kernel on their own: out[k][0 .. 6) / [0 .. 9) = the rows part[(c * m + k) * 6 / 9] added from 0.0
// in chunk order
hipError_t launch_jerk_fold_f64(const void *part, int m, int j_split, double *aj64, hipStream_t s);
hipError_t launch_snap_fold_f64(const void *part, int m, int j_split, double *ajs64, hipStream_t s);

// What every fp64 row scan is launched with (scan_tile64.h: the potential and the tidal tensor, the pair, neighbour and group censuses):
// rows — the bodies themselves or m points that are not bodies — against all bodies, a slab's partial rows in `part`.
struct RowScan64Launch {
  const void *posm = nullptr;   // [n_total] double4: x, y, z, m
  const void *ppos = nullptr;   // [m] double4: x, y, z, unused; nullptr: the bodies themselves (m == n_total)
  void *part = nullptr;         // the partial rows of one slab
  size_t part_elems = 0;        // the float4 `part` holds: at least probe_part_elems(n_total, m, the pass's width), or nothing is launched
  int n_total = 0, m = 0;
  int lanes = 0;                // points per lane: 1 or 2; 0: hermite_block_lanes(m, 0).  It enters no result (the bodies: always 2)
};

// The potential and the tidal tensor of an fp64 state, at the bodies or at m points that are not bodies — kernels_pot64.hip: with
// d = x_j - x, s^2 = |d|^2 + eps2, t = 1 / s:  phi = -sum_j G m_j t,  T_ab = sum_j G m_j [3 d_a d_b t^5 - delta_ab t^3], fp64 sums over
// launch_jerk's chunks and tiles on fp64 state in the same order, with its s2 and rsq.  ppos == nullptr: the rows are the bodies
// (m == n_total), each leaves itself out BY INDEX; else no pair is dropped by index: t = (s2 > 0) ? rsq(s2) : 0.  eps2 == 0: a pair at
// distance 0 adds nothing; eps2 > 0: a point exactly on body i feels -G m_i / eps in phi and -G m_i / eps^3 on the diagonal of T.  A
// row's sums depend on its point and the bodies alone; a zero-mass body adds exactly nothing.  A partial row is one double (the
// potential: probe_slab_points(n_total, 1), half of it used) or eight (the tensor's seven sums and a pad: probe_slab_points(n_total, 4));
// the rows go in slabs of that many and are folded from 0.0 in chunk order: phi = -P, T_aa = S_aa - Q.
constexpr int kPot64Width = 1, kTidal64Width = 4;   // the float4 of a partial row: one double (half a float4 unused), eight doubles
struct Pot64Launch : RowScan64Launch {
  double *out = nullptr;        // [m]: phi — the tensor: [m][6], xx, yy, zz, xy, xz, yz
  double G = 0.0, eps2 = 0.0;
};
hipError_t launch_pot_f64(const Pot64Launch &L, hipStream_t s);
hipError_t launch_tidal_f64(const Pot64Launch &L, hipStream_t s);

// The pair census of an fp64 state, at the bodies or at m points that are not bodies — kernels_census64.hip: an argmin pass over
// launch_pot_f64's chunks and tiles.  With d = x_j - x, w = v_j - v, d2 = |d|^2 (never softened), s2 = d2 + eps2, t = 1 / s and the
// row's mass term g (a body: G m_i; a point: 0):
//   launch_nearest_f64:  index = the body with the smallest d2, value = that d2 — no root; vel, pvel, d2 and eps2 are not read
//   launch_partner_f64:  index = the body with the smallest e = fma(-(G m_j + g), t, 0.5 |w|^2), value = that e, d2 = that body's d2
// under strict < in ascending j: the lowest index wins a tie; a value that is NaN and a body whose d2 is not finite are never chosen;
// no body chosen: (-1, +inf, +inf).  ppos == nullptr: the rows are the bodies (m == n_total), each leaves itself out BY INDEX; else no
// body is dropped by index.  The zero padding of a chunk's last tile is kept out by index (j < j1); a zero-mass body is a candidate.  A
// row's result depends on the row and the bodies alone.  A partial row is (d2, index) — probe_slab_points(n_total, 1) — or (e, d2,
// index, pad) — probe_slab_points(n_total, 2) —; the rows go in slabs of that many and are folded in chunk order under strict <.
constexpr int kNearest64Width = 1, kPartner64Width = 2;   // the float4 of a partial row: (d2, index), (e, d2, index, pad)
struct Census64Launch : RowScan64Launch {
  const void *vel = nullptr;    // [n_total] double4: vx, vy, vz, unused (the partner pass)
  const void *pvel = nullptr;   // [m] double4: the points' velocities (the partner pass, ppos != nullptr)
  int *index = nullptr;         // [m]
  double *value = nullptr;      // [m]: d2 (nearest), e (partner)
  double *d2 = nullptr;         // [m]: the partner's d2 (the partner pass)
  double G = 0.0, eps2 = 0.0;
};
hipError_t launch_nearest_f64(const Census64Launch &L, hipStream_t s);
hipError_t launch_partner_f64(const Census64Launch &L, hipStream_t s);
// out[0] = the smallest value[i] over the n rows, out[1] = the lowest row i that attains it, out[2] = index[i], out[3] = aux[i] (aux ==
// nullptr: the value) — (+inf, -1, -1, +inf) where no value is below +inf: launch_tidal_time's two launches and fixed order, for a
// minimum; `partials` holds 2 * energy_fast_slots(n) doubles
hipError_t launch_census_pair(const double *value, const int *index, const double *aux, int n, double *partials, double *out, hipStream_t s);

// The neighbour census of an fp64 state, at the bodies or at m points that are not bodies — kernels_neighbours64.hip: launch_nearest_f64's
// pass with a sorted list of K (d2, index) per row where that keeps one.  Per row the k bodies with the smallest d2 (never softened), in
// lexicographic (d2, index) order: strict < in ascending j, so the lowest index wins every tie; a d2 that is NaN or +inf is never
// listed; the empty slots read (-1, +inf).  ppos == nullptr: the rows are the bodies (m == n_total), each leaves itself out BY INDEX;
// else no body is dropped by index.  The padding of a chunk's last tile is kept out by index; a zero-mass body is a candidate.  The
// compiled width is neighbours64_width(k) (4, 6 or 8); the answer for k is the first k entries of the list whichever width ran, and a
// row's list depends on the row and the bodies alone.  A partial row is K x (d2, index) — probe_slab_points(n_total, K) —; the rows go
// in slabs of that many and are merged in chunk order under strict <.
//   index, d2:  [m * k] each, rows of k; either may be null
//   rho, rk2:   [m] each, the bodies' form with 2 <= k only; either may be null.  The Casertano-Hut density: rho = msum / ((4 pi / 3)
//               (r2 sqrt(r2))) with msum the raw masses of the k - 1 nearest added in neighbour order and r2 = rk2 = d2 of the k-th;
//               rho = 0 where the k-th is missing (rk2 = +inf) or the quotient is NaN
constexpr int kNeighbours64Max = 8;   // == NBODY_NEIGHBOURS_MAX
struct Neighbours64Launch : RowScan64Launch {   // (the partial rows' width: neighbours64_width(k))
  int *index = nullptr;
  double *d2 = nullptr, *rho = nullptr, *rk2 = nullptr;
  int k = 0;
  double G = 0.0;               // the tiles hold G m as the census's do; no result reads it
};
int neighbours64_width(int k);
hipError_t launch_neighbours_f64(const Neighbours64Launch &L, hipStream_t s);
// The density centre and core radius of n bodies from their densities rho (weights w = rho where 0 < rho < +inf, else 0), two O(N)
// passes in launch_energy_fast's fixed order, no atomics: out[0] = S0 = sum w, out[1 .. 3] = centre = (sum w x) / S0, out[4] = used (the
// bodies with w > 0), out[5] = the largest w, out[6] = the lowest body that attains it, out[7] = Q0 = sum w^2, out[8] = core radius =
// sqrt(sum w^2 |x - centre|^2 / Q0).  used == 0: centre and radius NaN, out[5] = 0, out[6] = -1.  `partials` holds
// 8 * energy_fast_slots(n) doubles.
hipError_t launch_density_centre(const void *posm, const double *rho, int n, double *partials, double *out, hipStream_t s);

// The radial census of an fp64 state about a centre — kernels_radial64.hip: the bodies in ascending (d2, index) order with d2 in
// nbody_mass_within's convention (finite d2, then +inf, then NaN, each group in index order), the cumulative mass in that order in blocks
// of 256 (include/nbody.h: a function of the sorted masses and n alone), and for k fractions f of the total mass the first position whose
// cumulative mass reaches f * total.  The order comes from the Barnes-Hut radix passes (kernels_bh_sort.hip) on the bit patterns of d2.
// Everything lives in one work area of radial64_work(n).bytes bytes; the offsets of the results in it (bytes, multiples of 256):
constexpr int kRadialFractionsMax = 64;   // == NBODY_LAGRANGE_MAX
struct Radial64Work {
  size_t key[2], idx[2];   // the passes' two key and two index arrays; behind the launch key[0] holds the sorted keys — read as doubles the
                           // sorted d2, a NaN as all ones — and idx[0] the order
  size_t cum;              // [n] doubles: mass_cum
  size_t part_hist, slice_hist, desc, status, blk_sum, off, fin_part, sel_part;
  size_t rows;             // [k] nbody_lagrange
  size_t total;            // one double: mass_cum[n - 1]
  size_t n_finite;         // one int
  size_t clear_bytes;      // desc .. status, cleared before the first pass
  size_t bytes;
};
Radial64Work radial64_work(int n);
// workgroups of the radix pass the current device holds at once: a pass is never launched with more (its workgroups wait for each other)
hipError_t radial64_resident(int *resident);
struct Radial64Launch {
  const void *posm = nullptr;        // [n_total] double4: x, y, z, m
  int n_total = 0;
  double centre[3] = {0.0, 0.0, 0.0};
  const double *fractions = nullptr; // [k], host; k == 0: the order and the cumulative mass alone
  int k = 0;
  int resident = 0;                  // radial64_resident's answer
  void *work = nullptr;              // device, radial64_work(n_total).bytes
  const hipEvent_t *events = nullptr;   // five events recorded ahead of the keys, the sort, the scan, the selection and behind it; or null
};
hipError_t launch_radial_f64(const Radial64Launch &L, hipStream_t s);

// The group census of an fp64 state, at the bodies or at m points that are not bodies — kernels_groups64.hip: a pass over
// launch_nearest_f64's chunks and tiles that counts and takes an integer minimum where that one takes an argmin.  With d = x_j - x and
// contraction off, d2 = (dx*dx + dy*dy) + dz*dz (nbody_mass_within's expression); row and body j are LINKED iff d2 <= r2 — a NaN d2 and a
// +inf d2 never are.  ppos == nullptr: the rows are the bodies (m == n_total), each leaves itself out BY INDEX; else no body is dropped by
// index.  The padding of a chunk's last tile is kept out by index; a zero-mass body links like any other.  A partial row is two int32
// (minimum, count) in a width-1 slot — probe_slab_points(n_total, 1) —; the rows go in slabs of that many and are folded in chunk order.
//   launch_radius_counts_f64:  count = the number of linked bodies per row; parent and mn are not read
//   launch_groups_pass_f64:    the bodies only: mn[i] = min(parent[i], parent[j] over the linked j) and, first_round, count as above
constexpr int kGroups64Width = 1;   // the float4 of a partial row: two int32, half a float4 unused
struct Groups64Launch : RowScan64Launch {
  const int *parent = nullptr;  // [n_total]: every body's current parent label (the groups' pass)
  int *mn = nullptr;            // [m]: the smallest parent among the row's own and its linked bodies' (the groups' pass)
  int *count = nullptr;         // [m]: the linked bodies
  double r2 = 0.0;              // radius * radius: finite and >= 0, or nothing is launched
};
hipError_t launch_radius_counts_f64(const Groups64Launch &L, hipStream_t s);
hipError_t launch_groups_pass_f64(const Groups64Launch &L, bool first_round, hipStream_t s);
// The O(N) kernels of the groups, the connected components of the links.  parent[i] = i (identity); then per round, after a pass:
// launch_groups_merge copies parent to `hooked`, lowers hooked[parent[i]] to mn[i] where mn[i] < parent[i] (integer atomicMin: the
// result does not depend on the order), writes parent[i] = the fixed point of hooked from i (hooked is read-only meanwhile and never
// ascends) and sets *changed to 1 where a parent changed, else 0.  Converged parents are the labels: the lowest index of each group.
hipError_t launch_groups_identity(int *parent, int n, hipStream_t s);
hipError_t launch_groups_merge(int *parent, const int *mn, int *hooked, int n, int *changed, hipStream_t s);
// members[i] = the size of label[i]'s group (`size`: [n] work), and sum[4]: the groups, those of two or more, sum of degree, and
// max over the groups of (size << 32 | 0x7fffffff - label) — integer atomics on cleared words, the same values whatever the order
hipError_t launch_groups_members(const int *label, const int *degree, int n, int *size, int *members, unsigned long long *sum, hipStream_t s);

// The separation census of an fp64 state, over the bodies or over m points that are not bodies — kernels_pairs64.hip: the group census's
// pass (its grid, chunks, tiles, d2 and <=) with NO per-row result: how many (row, body) pairs have d2 <= t, for kPairs64Group thresholds
// t at once.  ppos == nullptr: the rows are the bodies (m == n_total) and the pairs i != j BY INDEX are counted, ORDERED (each unordered
// pair twice: d2 is symmetric in every bit); else no body is dropped by index.  A NaN d2 and a +inf d2 never count; the padding and the
// repeated rows never count; a zero-mass body counts.  Every wave counts on its scalar pipe; a workgroup's kPairs64Group totals go to a
// slot of its own in `partial`, and a fold adds the slots into count[] with integer atomicAdd: the same words whatever the order.
// `part` is not used (there are no partial rows); the rows still go in the slabs of a width-1 pass, every slab through the same
// `partial` (the stream orders them) into the same words.
#ifndef NBODY_PAIRS64_GROUP
#define NBODY_PAIRS64_GROUP 16   // A/B builds: 8, 16, 32 (profiles/pairs_f64_kernel_resources.txt)
#endif
constexpr int kPairs64Group = NBODY_PAIRS64_GROUP;   // thresholds per launch: two SGPRs each and one per counter
constexpr int kPairs64Width = 1;                     // the slabs' width (no partial row is written)
struct Pairs64Launch : RowScan64Launch {
  double r2[kPairs64Group] = {};        // r2[0 .. k): ascending (repeats allowed), each finite and >= 0, or nothing is launched
  int k = 0;                            // 1 .. kPairs64Group.  The kernel's unused thresholds sit BELOW r2[0] and hold no d2 (-1): the
                                        // wave leaves the chain at the first of them, so a launch of few thresholds pays for few
  unsigned long long *count = nullptr;  // [k], device, cleared by the caller: count[q] += the pairs with d2 <= r2[q]
  unsigned long long *partial = nullptr;   // device work area, written before it is read
  size_t partial_words = 0;             // the words `partial` holds: at least pairs64_partial_words(n_total, m, ...), or nothing is launched
};
size_t pairs64_partial_words(int n_total, int m, bool self, int lanes);   // kPairs64Group words per workgroup of the largest slab
hipError_t launch_pair_counts_f64(const Pairs64Launch &L, hipStream_t s);

// The minimum spanning forest of an fp64 state in Boruvka rounds — kernels_mst64.hip: launch_nearest_f64's argmin pass with the group
// census's d2 and its label in the tile's fourth component.  Edges are the pairs i < j with a finite d2 = (dx*dx + dy*dy) + dz*dz
// (contraction off), ordered by the key (d2, i, j): a strict total order, so the forest is unique.
//   launch_mst_pass_f64:  the bodies only (m == n_total, ppos == nullptr): per row the body j of ANOTHER label with the smallest d2 under
//                         strict < in ascending j — for a fixed row the smallest key —; none: (-1, +inf).  A d2 that is NaN or +inf is
//                         never taken; the padding is kept out by index, the row's own component (itself included) by label.  A
//                         partial row is (d2, index), kNearest64Width, folded in chunk order under strict <.
constexpr int kMst64Width = kNearest64Width;
struct Mst64Launch : RowScan64Launch {
  const int *label = nullptr;   // [n_total]: every body's component label (a body of that component, whose own label is itself)
  int *index = nullptr;         // [m]
  double *d2 = nullptr;         // [m]
};
hipError_t launch_mst_pass_f64(const Mst64Launch &L, hipStream_t s);
// The O(N) kernels of a round, integer atomics only — every array comes out the same whatever the order.  W is carved from one work area:
struct Mst64Work {
  double *near_d2 = nullptr;               // [n] the pass's answer, with near_j
  unsigned long long *best = nullptr;      // [n] per label: the smallest d2 of an edge that leaves the component, as its bit pattern
  unsigned long long *pair = nullptr;      // [n] per label: the smallest (lo << 32 | hi) among the edges of that d2     (best, pair: adjacent)
  double *edge_d2 = nullptr;               // [n] the edges in the order they were appended               (edge_d2, edge_i, edge_j, component:
  int *edge_i = nullptr, *edge_j = nullptr;   // [n] each, i < j                                            adjacent, read back in one copy)
  int *component = nullptr;                // [n] the lowest index of every body's component (launch_mst_components)
  int *label = nullptr, *near_j = nullptr, *succ = nullptr, *lowest = nullptr;   // [n] each
  int *cursor = nullptr;                   // the edges appended so far
};
// label[i] = lowest[i] = i, *cursor = 0
hipError_t launch_mst_begin(const Mst64Work &W, int n, hipStream_t s);
// best = pair = all ones, ahead of a round's pass
hipError_t launch_mst_clear(const Mst64Work &W, int n, hipStream_t s);
// behind the pass: pick (atomicMin of the d2 bits into best[label], then of the packed pair among the bodies that attain it), hook (a
// label's successor is the label at the foreign end of its edge; where two labels chose the same edge the lower one stays a root; the
// edge is appended once, at atomicAdd(cursor), by the label that is not the higher of such two), compress (label[i] = the root the
// successors lead to from label[i]: succ is read-only meanwhile, a forest by the total order, and the chase is capped at n)
hipError_t launch_mst_merge(const Mst64Work &W, int n, hipStream_t s);
// component[i] = the lowest body index among those of label[i]
hipError_t launch_mst_components(const Mst64Work &W, int n, hipStream_t s);

// Symmetric (each unordered pair once) force pass — kernels_sym.hip (fp32), kernels_sym64.hip (fp64).  Who evaluates
// which pairs, where the partial sums go and in which order they are added is the plan of sym_plan.h, uploaded once.
struct SymLaunch {
  const void *posm;     // [n_total] float4 / double4, all bodies
  void *posg;           // fp32 only: [n_pad] float4 (x, y, z, G m) + zero-mass padding, rewritten every pass
  void *pool;           // [pool_elems] float4 / double4: the items' partial-sum segments
  const void *items;    // [n_items] SymItem: one workgroup each
  int n_items;
  const void *i_ptr, *i_off;   // CSR over own 64-body granules: i-side segments
  const void *j_ptr, *j_off;   // CSR over all granules: j-side segments
  void *send;           // [n_total] float4: this rank's j-side contribution to every body (n_src segments of i_count)
  const void *recv;     // [n_src][i_count] float4: what every rank contributed to the own bodies (== send when n_src == 1)
  int n_total;
  int n_pad;            // blocks * bodies per i-set
  int n_src;            // ranks sharing the bodies
  int np;               // fp32: register pairs of i-bodies per lane (1, 2, 4, 8); fp64: bodies per lane / 2 (1, 2)
  int precision;        // NBODY_PREC_F32 (float4 rows) or NBODY_PREC_F64 (double4 rows)
  int kahan;            // fp32 only: Kahan-compensated accumulation
  double G;
  double eps2;          // > 0 softened / floor; == 0 exact d == 0 skip (clamp form)
  void *dup_table;      // eps2 == 0 only: dup_slots x 8-byte hash slots + one flag word; nullptr = always run the guarded kernel
  int dup_slots;        // power of two >= 2 * n_total
  // fused single-device fp32 stepping (update_sym_fused_kernel): the update folds the j-side rows itself and prepares the
  // next pass (posg, the other detector table); a force pass then launches no prep and no reduce_j kernel
  int fused = 0;              // launch_forces_sym: no reduce_j; launch_update_sym: the fused kernel
  int skip_prep = 0;          // posg and dup_table are already those of the current positions
  void *dup_table_next = nullptr;
  // equal-mass form (forces_sym_pk_kernel / forces_sym_f64_kernel, UNI): `general` is a device int the preparation
  // kernel (fp64: mass_check_kernel) raises when a body's mass differs from body 0's; nullptr = general kernels only.  uni_host: 1 = the host knows the masses are equal
  // and nobody else writes the buffer (equal-mass launches only), 0 = it knows they are not (general launches only),
  // -1 = launch both, each looks at `general`.
  void *general = nullptr;
  int uni_host = 0;
  // Sharded fp32 contexts can run the pass in two goes, so that the strips inside the own slice need not wait for the other
  // ranks' positions: phase 1 = prepare the own slice [own_begin, own_begin + own_count) and run items [0, n_local);
  // phase 2 = prepare the rest, run items [n_local, n_items) and fold the j-side rows; phase 0 = everything at once.
  // Same plan, same segments, same summation order: the bits do not depend on how the pass is cut.
  int phase = 0;
  int n_local = 0;
  int own_begin = 0, own_count = 0;
  // What one call of launch_forces_sym does (fp32; the fp64 launcher runs a whole pass): prepare (phase says which bodies),
  // launch the items [item0, item1) of the launch order (item1 < 0: phase's own range), fold the j-side lists j_ptr / j_off
  // into `send` — on top of what is there when fold_accumulate (pool phases after the first, sym_plan.h).
  int item0 = 0, item1 = -1;
  int do_prep = 1, do_fold = -1;     // do_fold < 0: as the phase says (phases 0 and 2 fold)
  int fold_accumulate = 0;
  int clear_detector = 1;            // the fold also clears the coincident-body table for the next pass (the pass's LAST fold only)
  // even-share plan (sym_plan.h, plain fp32 on one context): the items carry first / last steps and follow the ring order,
  // which goes on at body 0 past `wrap` bodies (64 x granules of the system)
  int even = 0, wrap = 0;
  void *clk = nullptr;               // fp32: two device uint64 the force kernel's workgroups add their clock intervals to (pk_common.h)
};
// forces + fold of the j-side rows into L.send
hipError_t launch_forces_sym(const SymLaunch &L, hipStream_t s);
// acc = own i-side rows + L.recv segments; dt > 0: kick-drift of the owned slice
hipError_t launch_update_sym(const SymLaunch &L, void *posm, void *vel, void *acc, int i_begin, int i_count, float dt,
                             hipStream_t s);

// GPU Barnes-Hut with the reference's tree and opening rule — bh_frame.hip (host side), kernels_bh_{small,sort,build,walk}.hip, bh_common.h.  fp32.
struct BhState;
// n bodies; the context owns [i_begin, i_begin + i_count) of them (all: 0, n) — a slice builds the whole tree and walks its own bodies
hipError_t bh_create(BhState **out, int n, int i_begin, int i_count);   // *out is set even on failure: bh_destroy it
void bh_destroy(BhState *b);
void bh_positions_changed(BhState *b);                         // a body was moved by something other than a frame's walk
void bh_positions_external(BhState *b);                        // the caller holds the position buffer from now on
hipError_t bh_reset_root(BhState *b, hipStream_t s);          // previous CoM := 0 (a new scene, OctreeSearch.cpp:77)
// One frame = CreateOctree (OctreeSearch.cpp:74-89: ComputeCubeSize, the tree rooted at the previous CoM, ComputeMass), the walk
// Octree::ComputeForces(body, theta) of every body and — with dt > 0 — the Tick's update of (posm, vel) in place, QUEUED on the
// stream: nothing waits for the host (small systems, bh_is_small: two launches; larger ones up to 2^20 bodies: nine; beyond, one
// wait inside for the deepest level).  bh_collect waits for the stream and reports the frames queued since the last collect:
// *status is one of the kBhStatus verdicts below; a refused frame (bh_refused) and everything queued behind it leave the state
// untouched, a frame given up (kBhStatusRetry) or handed back (kBhStatusDeep) and the ones behind it did nothing and are the
// caller's to queue again (bh_driver.h).  keep_root != 0: the next tree's root centre stays what it was (a diagnostic pass).
// stage (optional): the walk also writes every body's FParticle record (10 floats, body order) there — the frame's mirror.
// eps2: Plummer softening, (float)(eps * eps).  > 0: every accepted node's term is that of ds = sqrtf(d^2 + eps2) (the walks' SOFT
// instantiations); where the walk goes is the reference's, on the unsoftened d.  0: the reference's term.
bool bh_is_small(const BhState *b);
hipError_t bh_frame(BhState *b, void *posm, void *vel, void *acc, float theta, double G, float eps2, float dt, int keep_root,
                    float *stage, hipStream_t s);
// bh_collect's verdicts (the frames' header word 3; bh_common.h's kStatus names are these)
constexpr int kBhStatusOk = 0;
constexpr int kBhStatusTooDeep = 1;                       // refused: the tree would be deeper than the context's limit (42 levels unless raised)
constexpr int kBhStatusNodePool = 2;                      // refused: node pool exhausted
constexpr int kBhStatusRetry = 3;                         // given up by the warm sort: queue it and the frames behind it again (the first sorts cold)
constexpr int kBhStatusUnsorted = 4;                      // refused: a COLD sort left keys out of order (an internal error, never seen)
constexpr int kBhStatusDeep = 5;                          // a deep context's frame handed back: build it again with bh_deep_frame, then the rest
constexpr int kBhStatusDeepRun = 6;                       // refused: a deep frame's cell of level 42 holds more bodies than kDeepRunMax
// refused: the state is untouched and the context carries an error text (bh_status_error)
inline bool bh_refused(int status) {
  return status == kBhStatusTooDeep || status == kBhStatusNodePool || status == kBhStatusUnsorted || status == kBhStatusDeepRun;
}
hipError_t bh_set_max_depth(BhState *b, int levels);      // the deepest tree answered, 42 .. 200 (above 42: deep frames, bh_deep_frame)
hipError_t bh_deep_frame(BhState *b, void *posm, void *vel, void *acc, float theta, double G, float eps2, float dt, int keep_root,
                         float *stage, hipStream_t s);    // the frame bh_collect handed back (kBhStatusDeep), built with its deep clusters
float bh_last_size(const BhState *b);                         // Size of the last frame bh_collect has seen
hipError_t bh_collect(BhState *b, hipStream_t s, int *status, int *frames);   // *frames: how many were built
hipError_t bh_debug_clocks(BhState *b, long long out[16 + 3 * 512], hipStream_t s);   // tuning builds only (tools/bh_phases.py)
hipError_t bh_debug_poison(BhState *b, int kind, hipStream_t s);   // tests: kind 1 = the warm sort's bucket counts := 3 each (a fill that never ran)
void bh_debug_sort_counts(const BhState *b, long long *warm_frames, long long *retries);   // frames sorted from the previous order; times frames were queued again
const float *bh_root_device(const BhState *b);                // device (ox, oy, oz, Size) of the last tree (small systems)
hipError_t bh_get_tree_com(BhState *b, float out[3], hipStream_t s);   // root CoM of the last tree built
void bh_set_div_mode(BhState *b, int div_mode);            // 0: `/=` in ComputeMass multiplies by the reciprocal; 1: divides
// order[k] = the body whose leaf a depth-first walk (children 0..7) meets k-th in the last tree built (host array, n ints)
hipError_t bh_leaf_order(BhState *b, int *out_host, hipStream_t s);
hipError_t bh_stats(BhState *b, hipStream_t s, int *nodes, int *levels);   // waits for the stream when the last tree's counts are still on their way
// out[body] = (ox, oy, oz, Size) of the leaf holding the body, for the last tree built
hipError_t bh_leaf_boxes(BhState *b, void *out, hipStream_t s);
// Octree::ComputeForces (OctreeSearch.h:99-108) from m points that are not bodies (kernels_bh_pot.hip; pts: float4 x, y, z, unused), over the tree the
// frame queued last on `s` has built — the body walks' step test and term, one lane per point in the caller's order.  The kernel looks at
// the frame's verdict and does nothing behind a frame refused or given up; it writes neither the verdict nor the tree.  dt > 0: the points
// are tracers and get the bodies' kick-drift on (pts, vel) behind their walk.  Not for the tree of a deep frame (bh_last_deep).
hipError_t bh_probe_walk(BhState *b, void *pts, void *vel, void *acc, int m, double G, float eps2, float dt, hipStream_t s);
// The potential from the same walk: an accepted node adds G * M / ds in fp64, ds = sqrtf(d2 + eps2) correctly rounded;
// phi = -(the fp64 sum in walk order) to phi64 and, rounded, to phif (either may be null).  pts == nullptr: the points are the bodies
// (posm, n of them), walked in key order and written at the body's index — a body meets its own leaf at d == 0, which adds nothing.
hipError_t bh_pot_walk(BhState *b, const void *posm, const void *pts, double *phi64, float *phif, int m, double G, float eps2, hipStream_t s);
// The tidal tensor from the same walk: seven fp64 sums in walk order (kernels_bh_pot.hip: tidal_term), T_aa = S_aa - Q; six doubles per
// point to t64 and, rounded, six floats to tf (either may be null).  pts == nullptr: the bodies, as bh_pot_walk takes them.
hipError_t bh_tidal_walk(BhState *b, const void *posm, const void *pts, double *t64, float *tf, int m, double G, float eps2, hipStream_t s);
bool bh_last_deep(const BhState *b);                          // the last frame queued was built by the deep path
hipError_t bh_get_root_com(BhState *b, float out[3], hipStream_t s);
hipError_t bh_set_root_com(BhState *b, const float in[3], hipStream_t s);

// out_bits (uint32, pre-zeroed) = bit pattern of max_i max(|x|,|y|,|z|) over the owned slice.
// zero_word (optional): a second word this launch clears — for callers that alternate between two result words.
hipError_t launch_bounds(int precision, const void *posm, int i_begin, int i_count, unsigned int *out_bits,
                         hipStream_t s, unsigned int *zero_word = nullptr);

// out_bits (uint32, pre-zeroed) = bit pattern of max_j |m_j| over all n_total bodies.
hipError_t launch_massmax(int precision, const void *posm, int n_total, unsigned int *out_bits, hipStream_t s);

// Device-side repack for the renderer hand-off: FParticle records (10 floats) of the owned slice / packed xyz.
hipError_t launch_pack_particles(int precision, const void *posm, const void *vel, const void *acc, float *out,
                                 int i_begin, int i_count, hipStream_t s);
hipError_t launch_pack_positions(int precision, const void *posm, float *out, int first, int count, hipStream_t s);

// fp64 energy pieces: out[0] = KE of owned bodies, out[1] = sum_i 1/2 m_i phi_i.  Two launches: per-workgroup parts into
// `partials` (energy_partials(n_total, i_count) doubles), then a fixed-order fold — no atomics, reproducible bits.
size_t energy_partials(int n_total, int i_count);
hipError_t launch_energy(int precision, const void *posm, const void *vel, int n_total, int i_begin, int i_count,
                         double G, double eps2, double *partials, double *out, hipStream_t s);

// O(N) bulk diagnostics of the owned bodies — kernels_moments.hip.  Two launches each: per-workgroup slots, then one workgroup folds them
// in a fixed order — no atomics, nothing to clear, reproducible bits.  The geometry (slots, bodies per slot) follows from i_count alone.
// `scratch`: moments_scratch_bytes(i_count) of device memory; the results arrive at its start — launch_moments: kMomentValues doubles
// in the field order of nbody_moments (mass ... torque[3]); launch_mass_within: kMassWithinMax doubles (the masses of the k radii), then
// kMassWithinMax int64 (the counts).
constexpr int kMomentValues = 24;
constexpr int kMomentSlotCap = 1024;
constexpr int kMassWithinMax = 64;
void moments_geometry(int i_count, int *slots, int *per);
size_t moments_scratch_bytes(int i_count);
hipError_t launch_moments(int precision, const void *posm, const void *vel, const void *acc, int i_begin, int i_count, void *scratch,
                          hipStream_t s);
hipError_t launch_mass_within(int precision, const void *posm, int i_begin, int i_count, const double centre[3], const double *radii,
                              int k, void *scratch, hipStream_t s);

}  // namespace nbody
