// Launch policy (launch_policy.h): argument checks, launch geometry, algorithm and work plan, and what a context allocates for
// them.  Host-only C++; every threshold below is a measured cross-over (the profiles named next to it).
#include "launch_policy.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

namespace nbody {

int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  if (!e || !*e) return dflt;
  const int v = atoi(e);
  return v > 0 ? v : dflt;
}

int env_flag(const char *name) {
  const char *e = getenv(name);
  return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
}

namespace {

int refuse(std::string *why, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  *why = buf;
  return code;
}

// Up to N = 16384 a workgroup owns a few bodies and spreads the j range over its lanes (forces_block_pk_kernel,
// kernels_block.hip: one launch per step, no partial rows; 2 ... 8 register pairs of bodies per workgroup).  Above it the
// symmetric pass (plain fp32; Kahan and fp64 go through the tile kernels up to their own threshold).  Whole steps without
// events, same box (profiles/r03_block_kernel_by_n.txt): N = 14336 0.0538 ms against the symmetric pass's 0.0630, 16384 —
// four full workgroups per CU — 0.0674 / 0.0735, 17408 0.0922 / 0.0710; round 2's one-pair-per-workgroup kernel
// (small_pk_kernel, gone): N = 2000 0.0067 ms against 0.0053 now, 4096 0.0143 / 0.0096, 6000 0.0246 / 0.0150.
constexpr int kSmallSystem = 6656;      // the threshold of rounds 1-2 (tile kernel above it); still Kahan's and the forced geometries'
int block_max_n() { static const int v = env_int("NBODY_BLOCK_MAX_N", 16385); return v; }   // latched at first use

// forces_block_kernel (Kahan, fp64): 4 or 8 bodies per workgroup by the rule of block_pairs
int block_bodies(int n_total, int cus) {
  { const int v = env_int("NBODY_BLOCK_NB", 0); if (v == 4 || v == 8) return v; }   // tuning only
  // on a tie eight, unless all workgroups of four are resident at once anyway (measured, whole steps in both precisions:
  // N = 2000 6.8 - 7.5 us with four against 7.7 with eight; N = 4096 16.8 - 18.9 against 15.9 - 18.1)
  const long long r8 = ((n_total + 7) / 8 + cus - 1) / cus, r4 = ((n_total + 3) / 4 + cus - 1) / cus;
  return (r4 * 4 < r8 * 8 || (r4 * 4 == r8 * 8 && r4 <= 2)) ? 4 : 8;
}

int floor_pow2(long long v) { int p = 1; while ((long long)p * 2 <= v) p *= 2; return p; }

// Launch geometry.  j_split is a function of n_total only, so that the per-body summation order
// (and hence every bit of the trajectory) does not depend on how many GPUs share the bodies.
void choose_geometry(const nbody_params &p, int cus, LaunchPolicy *c) {
  c->tile = p.tile > 0 ? p.tile : 256;
  if (p.i_per_thread > 0) c->ipt = p.i_per_thread > 4 ? 4 : p.i_per_thread;   // 8 and 16 exist for the symmetric kernel only
  // whole steps without events (profiles/r02_small_system_thresholds.txt): N = 8192 0.0277 ms with four bodies per lane, 0.0258 with
  // two; 10240 0.0444 / 0.0427; N = 16384: 0.102 with four, 0.106 with two
  else c->ipt = (p.precision == NBODY_PREC_F64) ? 1 : (p.n_total >= 12288 ? 4 : (p.n_total >= kSmallSystem ? 2 : 1));
  int js;
  if (p.j_split > 0) {
    js = p.j_split;
  } else {
    // aim at >= 2048 workgroups (8 per CU) down to an 8-way body partition; a chunk may be a single tile — small
    // systems are short of workgroups, not of work per workgroup (N = 8192: 52 us with 8 chunks, 29 us with 32)
    const long long per_block = 256LL * c->ipt;
    long long iblocks8 = (p.n_total / 8 + per_block - 1) / per_block;
    if (iblocks8 < 1) iblocks8 = 1;
    js = floor_pow2((2048 + iblocks8 - 1) / iblocks8);
    const int max_js = p.n_total / c->tile;
    if (js > max_js) js = max_js;
    if (js < 1) js = 1;
  }
  int chunk = (p.n_total + js - 1) / js;
  chunk = (chunk + c->tile - 1) / c->tile * c->tile;
  js = (p.n_total + chunk - 1) / chunk;
  c->j_split = js;
  c->j_chunk = chunk;
  // Small and mid-size systems (the reference ships N = 2000): a workgroup owns a few bodies and its lanes split the j range
  // (forces_block_pk_kernel; forces_block_kernel in the other two precisions) — one lane per body cannot fill the chip
  // there.  Only when the caller left the geometry to us.  c->wave: register pairs per workgroup (plain fp32), bodies
  // per workgroup (Kahan, fp64).
  c->wave = 0;
  const bool ours = p.algorithm != NBODY_ALGO_SYMMETRIC && p.tile == 0 && p.i_per_thread == 0 && p.j_split == 0;
  if (ours && p.precision == NBODY_PREC_F32 && p.zero_mode != NBODY_ZERO_SELECT && p.n_total < block_max_n()) {
    c->wave = block_pairs(p.n_total, cus);
  } else if (ours && p.precision == NBODY_PREC_F32_KAHAN && p.zero_mode != NBODY_ZERO_SELECT &&
             p.n_total < env_int("NBODY_BLOCK_MAX_N_KAHAN", kSmallSystem)) {
    // above kSmallSystem the packed Kahan tile kernel is faster (whole steps: profiles/r03_block_kernel_other_precisions.txt)
    c->wave = block_bodies(p.n_total, cus);
  } else if (ours && p.precision == NBODY_PREC_F64 && p.n_total < env_int("NBODY_BLOCK_MAX_N_F64", kSmallSystem)) {
    c->wave = block_bodies(p.n_total, cus);
  }
  if (c->wave != 0) {
    c->j_split = 1;
    c->j_chunk = (p.n_total + c->tile - 1) / c->tile * c->tile;
  }
}

// Which plain fp32 systems take the even-share plan by default: whole steps without events, one box, both forms of the kernel,
// every bodies-per-lane choice under both plans (profiles/r05_even_share_vs_guided_by_n.txt; distinct / equal masses, best
// guided -> best even-share): N = 20480 95.2 / 88.7 us -> 92.3 / 86.4, 24576 128.2 / 119.3 -> 123.7 / 113.4, 32768 206.7 /
// 190.7 -> 199.6 / 182.3, 40960 302.9 / 281.1 -> 289.8 / 260.6, 65536 722.6 / 658.9 -> 703.3 / 630.7, 81920 1103.8 / 1014.1 ->
// 1081.2 / 967.3, 98304 1555.6 / 1421.7 -> 1552.3 / 1392.5; N = 18432 and 131072: nothing in it.
bool sym_even_default(int n_total, bool kahan) {
  // Kahan contexts (eight bodies per lane at most, two waves per SIMD): profiles/r05_even_share_vs_guided_by_n_kahan.txt — N = 12288
  // 51.1 / 49.3 us -> 49.8 / 47.5, 16384 77.8 / 75.0 -> 74.4 / 70.2, 24576 134.0 / 125.2 -> 127.6 / 116.1, 32768 212.8 / 196.1 ->
  // 210.8 / 189.2; from 49152 on the guided strips are ahead (427.8 / 391.8 against 439.0 / 394.6)
  if (kahan) return n_total >= env_int("NBODY_SYM_EVEN_KAHAN_MIN_N", 12288) && n_total < env_int("NBODY_SYM_EVEN_KAHAN_MAX_N", 40960);
  // (with the detector's sparse table, profiles/r05_even_share_vs_block_kernel_13k_to_19k.txt: N = 17408 73.0 / 67.7 -> 70.2 / 67.1
  // with four bodies per lane, 18432 78.4 / 74.6 -> 76.9 / 73.7, 19456 83.8 / 78.3 -> 83.2 / 79.7: everything the symmetric pass
  // runs below 106496 bodies (and, below, up to 139264).  The same table has even shares ahead of the block kernel from N = 15360 — 61.1 / 57.6 -> 57.4 / 54.8,
  // 16384 67.8 / 63.9 -> 64.4 / 61.2 —; the block kernel keeps those sizes for its one-launch step and what nbody_tick gets from it.)
  // Upper end, with TWO items per slot from 90112 bodies on — passes of 1.5 ms and more: slots of unequal speed drift apart —
  // (profiles/r05_even_share_rounds_at_larger_n.txt; guided -> one round -> two, distinct | equal masses): N = 98304 1596 -> 1590 ->
  // 1566 us | 1450 -> 1420 -> 1403, 114688 2073 -> 2063 -> 2037 | 1894 -> 1855 -> 1831, 131072 2650 -> 2664 -> 2645 | 2428 -> 2392 ->
  // 2381; from 147456 on nothing in it either way (3453 -> 3535 -> 3484 | 3160 -> 3185 -> 3118): even shares below 139264 bodies.
  return n_total >= env_int("NBODY_SYM_EVEN_MIN_N", 16385) && n_total < env_int("NBODY_SYM_EVEN_MAX_N", 139264);
}

// Symmetric algorithm: applicability, bodies per lane, and the work plan (sym_plan.h).  *reason: why a plan that was tried could not be
// built ("symmetric plan: ...") — AUTO then stays with the one-sided kernels, NBODY_ALGO_SYMMETRIC is refused with it.
void choose_algorithm(const nbody_params &p, int cus, uint64_t total_bytes, LaunchPolicy *c, std::string *reason) {
  c->sym = false;
  if (p.algorithm == NBODY_ALGO_TILED) return;
  if (p.zero_mode == NBODY_ZERO_SELECT) return;                         // compare+select lives in the one-sided kernel only
  // whole steps, one box, final kernels (profiles/r02_threshold_symmetric_vs_one_sided.txt): N = 10240 one-sided 0.0597 ms vs
  // symmetric 0.0597, N = 12288 0.0763 vs 0.0700, 14336 0.0934 vs 0.0841, 16384 (the one-sided geometry's best case) 0.0978
  // vs 0.0948, 18432 0.1287 vs 0.1024, 20480 0.147 vs 0.116; Kahan and fp64 likewise from 12288 (0.0735 vs 0.0639, 0.129 vs 0.119)
  // Round 3 (the fused update folds its two lists side by side; whole steps without events, same box: N = 8192 0.0266 ms
  // one-sided vs 0.0366 symmetric, 9216 0.0351 vs 0.0325, 10240 0.0423 vs 0.0393, 11264 0.0438 vs 0.0413; Kahan 9216 0.0326 vs
  // 0.0289, fp64 0.0774 vs 0.0658; distinct masses 0.0362 vs 0.0340): the symmetric pass from N = 9216
  if (p.algorithm == NBODY_ALGO_AUTO && c->wave != 0) return;            // the block kernels' one-launch step (choose_geometry)
  if (p.algorithm == NBODY_ALGO_AUTO && p.n_total < env_int("NBODY_SYM_MIN_N", 9216)) return;
  const bool f64 = p.precision == NBODY_PREC_F64, kahan = p.precision == NBODY_PREC_F32_KAHAN;
  if (f64 && !(p.eps > 0.0 || p.zero_mode == NBODY_ZERO_EXACT)) return;
  // bodies per lane.  fp32: 2 * register pairs; more of them amortise the travelling sums' dpp moves over more
  // arithmetic (tools/microbench6.hip) but make the i-set — the quantum of work — larger.  fp64: 2, or 4 at 2 waves/SIMD.
  // The even-share plan (sym_plan.h): plain fp32, one context owning all bodies, two register pairs per lane and more —
  // exactly one workgroup per slot, all of equal cost.  NBODY_SYM_EVEN = 0 / 1 forces the choice (A/B measurements, tests).
  const int even_env = env_flag("NBODY_SYM_EVEN");
  // (not where a test forces pool phases on a small system: the phased pass is the guided plan's)
  const bool even_wanted = !f64 && p.i_count == p.n_total && env_int("NBODY_SYM_POOL_BUDGET_MB", 0) == 0 &&
                           (even_env == 1 || (even_env < 0 && sym_even_default(p.n_total, kahan)));
  int ipt = p.i_per_thread;
  if (f64) {
    if (ipt == 0) ipt = p.n_total >= 65536 ? 4 : 2;
    if (ipt != 2 && ipt != 4) return;
  } else {
    if (ipt == 0 && even_wanted) {
      // even shares have no quantum of work to keep small: sixteen bodies per lane (the fewest instructions per interaction)
      // from N = 24576, eight from 20480, four below (same table: N = 20480 93.0 / 86.4 us with eight, 94.3 / 86.5 with sixteen; 22528 107.5 /
      // 99.2 against 115.4 / 105.4; 24576 125.1 / 115.4 against 123.7 / 113.4; 32768 205.5 / 190.3 against 199.6 / 182.3)
      // (Kahan: four below 22528 — N = 20480 95.0 / 88.7 us with four, 96.6 / 91.0 with eight —, eight above)
      ipt = env_int("NBODY_SYM_IPT", kahan ? (p.n_total >= 22528 ? 8 : 4) : (p.n_total >= 24576 ? 16 : (p.n_total >= 20480 ? 8 : 4)));
    } else if (ipt == 0) {
      // measured on one box, sustained load (profiles/r02_sweep_symmetric_by_n.txt, r02_tune_mid_sizes.txt): sixteen bodies
      // per lane win wherever the symmetric pass runs (N = 32768: 0.206 vs 0.211 ms with eight, 65536: 0.691 vs 0.718,
      // 131072: 2.62 vs 2.70, 2^20: 162 vs 170.5 ms); the Kahan form has no sixteen (its running compensated sums double the
      // accumulators) and runs eight
      if (!kahan && p.n_total >= 40960) ipt = 16;      // whole step, N = 32768: 0.2353 ms with eight, 0.2408 with sixteen; 40960: 0.3355 / 0.3336
      else if (p.n_total >= 24576) ipt = 8;
      else if (p.n_total >= 17408) ipt = 4;
      else ipt = 2;                                    // N = 12288: 0.0700 ms with two, 0.0713 with four; 16384: 0.0948 / 0.0964; 18432: 0.1037 / 0.1024
      ipt = env_int("NBODY_SYM_IPT", ipt);
      if (kahan && ipt == 16) ipt = 8;
      // sharded slices must be whole i-sets
      while (ipt > 2 && p.i_count != p.n_total && p.i_count % (256 * ipt) != 0) ipt /= 2;
    }
    if (ipt != 2 && ipt != 4 && ipt != 8 && ipt != 16) return;
    if (ipt == 16 && kahan) return;
  }
  const int bi = 256 * ipt;
  // workgroups the chip holds at a time: one wave of each per SIMD -> (waves per SIMD) per CU
  const int np = ipt / 2;
  const int wps = f64 ? (ipt == 4 ? 2 : 4) : (np == 8 ? 2 : (np == 4 ? (kahan ? 2 : 3) : (kahan && np == 2 ? 3 : 4)));
  c->sym_slots = cus * wps;
  // A strip = 1/(K * slots) of the work still to hand out.  Large K = many short strips = best balance of the force pass but
  // one i-side segment (bodies-per-i-set x 16 B, written and read back) per strip; small K = a first round of long strips.
  // Long passes want K = 6 (N = 2^20, force pass: K = 3 170.1 ms — slots of unequal speed drift apart over 100 ms —, 6
  // 164.1, 24 163.3 at three times the segments; profiles/r02_tune_guided_k_n2p20.txt).  Short passes do not care about K
  // but their update pays for every segment (whole step, profiles/r02_tune_whole_step_mid_sizes.txt: N = 65536 K = 6
  // 0.781 ms, K <= 3 0.752; N = 131072 2.780 vs 2.653; N = 32768 0.2675 vs 0.2518).
  // What decides is how long the pass runs (fp64 at N = 262144 takes 25 ms and wants K = 6: 25.5 vs 26.9 ms with 3), so K
  // follows the expected duration of this context's share: >= 15 ms 6, >= 5 ms 3, >= 0.5 ms 1.5, below 1.
  {
    const double rate = f64 ? 2.7e12 : (kahan ? 6.0e12 : 6.6e12);                      // interactions per second, measured
    const double est_ms = (double)p.n_total * (double)p.i_count / rate * 1e3;
    c->sym_k = est_ms >= 15.0 ? 6.0 : (est_ms >= 5.0 ? 3.0 : (est_ms >= 0.5 ? 1.5 : 1.0));
  }
  { const int v = env_int("NBODY_SYM_K", 0); if (v >= 1) c->sym_k = v; }                     // tuning only
  { const int v = env_int("NBODY_SYM_K_X10", 0); if (v >= 5) c->sym_k = v / 10.0; }          // tuning only
  // shortest strip, in 64-body subtiles: whole 256-body tiles from N = 131072, half tiles below (same table)
  // (round 3, whole steps without events, four bodies per lane: N = 20480 0.0921 ms with two subtiles, 0.0888 with one; two
  // bodies per lane — N = 16384 — do not care: 0.0737 / 0.0738)
  c->sym_min_sub = env_int("NBODY_SYM_MIN_SUB", p.n_total >= 131072 ? 4 : (!f64 && ipt == 4 ? 1 : 2));
  SymPlan *plan = &c->plan;
  std::string why;
  bool planned = false;
  const bool even = even_wanted && np >= 2;
  try {
    if (even) {
      const int rounds = env_int("NBODY_SYM_EVEN_ROUNDS", (!kahan && p.n_total >= 90112) ? 2 : 1);       // items per slot (sym_even_default)
      planned = build_sym_plan_even(p.n_total, bi, std::max(1, (int)((long long)c->sym_slots * rounds * env_int("NBODY_SYM_EVEN_ITEMS_PCT", 100) / 100)), plan, &why,
                                    env_int("NBODY_SYM_EVEN_COST_SYM", 82), env_int("NBODY_SYM_EVEN_COST_ONE", 74),
                                    env_int("NBODY_SYM_EVEN_COST_MOVE", 26), env_int("NBODY_SYM_EVEN_OWN_PCT", kSymEvenOwnPct));
      if (planned) { c->sym_k = 0.0; c->sym_min_sub = 0; }
    } else
    planned = build_sym_plan(p.n_total, p.i_begin, p.i_count, bi, c->sym_slots, c->sym_k, c->sym_min_sub, f64 ? 2 : 1, plan, &why,
                             0, env_int("NBODY_SYM_MAX_SUB", 0));
  } catch (const std::bad_alloc &) {
    why = "out of host memory";
  }
  // The partial-sum pool must fit comfortably: at most a third of the card's TOTAL memory (and 2^32 elements).  Beyond that
  // (N = 2^23 on one 288 GB card: the j-side segments alone are 137 GB) the fp32 pass runs in PHASES that share one j-side
  // area, sized so that the whole pool stays within 32 GB (sym_plan.h); fp64 has no phased form and leaves to the
  // one-sided kernel.  NBODY_SYM_POOL_BUDGET_MB forces phases at any size (tests).
  const int forced_mb = f64 ? 0 : env_int("NBODY_SYM_POOL_BUDGET_MB", 0);
  const bool too_big = !planned ? why.find("2^32") != std::string::npos
                                : (total_bytes > 0 && (double)plan->pool_elems * (f64 ? 32.0 : 16.0) > (double)total_bytes / 3.0);
  if (!f64 && !even && (forced_mb > 0 || too_big)) {
    const double cap = 32.0 * 1073741824.0 / 16.0;                                    // elements
    double budget = forced_mb > 0 ? (double)forced_mb * 1048576.0 / 16.0 : 20.0 * 1073741824.0 / 16.0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      try {
        planned = build_sym_plan(p.n_total, p.i_begin, p.i_count, bi, c->sym_slots, c->sym_k, c->sym_min_sub, 1, plan, &why,
                                 (uint64_t)budget);
      } catch (const std::bad_alloc &) { why = "out of host memory"; planned = false; }
      if (!planned || forced_mb > 0 || (double)plan->pool_elems <= cap) break;
      budget -= (double)plan->pool_elems - cap;                                       // the i-side segments took more than 12 GB
      if (budget < 2.0 * 1073741824.0 / 16.0) { planned = false; why = "the i-side segments leave no room for a shared j-side area"; break; }
    }
    if (planned && forced_mb == 0 && (double)plan->pool_elems > cap) { planned = false; why = "the partial-sum pool would exceed 32 GB even in phases"; }
  } else if (planned && too_big) {
    planned = false; why = "the partial-sum pool would exceed a third of the device memory";
  }
  if (!planned) {
    *reason = "symmetric plan: " + why;
    *plan = SymPlan();
    return;
  }
  c->sym_bi = bi; c->sym_np = f64 ? ipt / 2 : np; c->sym_pad = plan->n_pad; c->sym_items_n = (int)plan->items.size();
  c->sym_nsrc = plan->n_src; c->sym_pool_elems = plan->pool_elems; c->sym_n_local = plan->n_local;
  c->sym_n_gran = plan->n_gran;
  c->sym_even = plan->even;
  c->sym = true;
  c->wave = 0;            // the small-system one-launch step belongs to the one-sided path
}

// How sparse the coincident-body detector's table is: a body's entry is a chain of dependent device-scope compare-and-swaps (linear
// probing), each a round trip to memory, and the update kernel ends with the LONGEST chain of the system.  At a power of two >= 2 N
// slots (load up to 0.5; rounds 1-4) that chain was most of the fused update of a mid-size system: update kernel, slots >= 2 N / 4 N /
// 16 N / 64 N (profiles/r05_ab_detector_table_sparsity.txt, r05_ab_update_kernel_parts.txt): N = 20480 12.6 / 10.6 / 9.8 / 11.3 us,
// 32768 20.3 / 12.8 / 11.0 / 12.4, 65536 23.6 / 15.8 / 14.0 / 16.1 — and the table is cleared once per pass, which is what
// large systems see: N = 262144 153 / 155 / 166 / 193 us.  Hence 16 N below 131072 bodies, 4 N from there on.
int detector_slots(int n_total) {
  int slots = 1024;
  const int factor = env_int("NBODY_SYM_DUP_FACTOR", n_total < 131072 ? 16 : 4);
  while ((long long)slots < (long long)factor * n_total && slots < (1 << 30)) slots *= 2;
  return slots;
}

// What nbody_create allocates besides the state and the plan: the detector's tables and the equal-mass word.
void choose_allocations(const nbody_params &p, LaunchPolicy *c) {
  // NBODY_SYM_GUARDED=1 (A/B measurements only): always run the guarded kernel, no coincident-body detector.
  // NBODY_SYM_NO_UNI=1 (A/B measurements only) keeps every context on the general kernels.
  const bool exact = p.eps == 0.0 && p.zero_mode == NBODY_ZERO_EXACT && env_flag("NBODY_SYM_GUARDED") != 1;
  const bool uni_allowed = p.zero_mode != NBODY_ZERO_FLOOR && env_flag("NBODY_SYM_NO_UNI") != 1;
  c->recv_is_send = !(c->sym && c->sym_nsrc > 1);
  if (c->sym) {
    if (exact) {
      c->dup_slots = detector_slots(p.n_total);
      c->dup_tables = (p.precision != NBODY_PREC_F64 && c->sym_nsrc == 1) ? 2 : 1;   // fused stepping alternates between two tables
    }
    // equal-mass kernels (not with the eps floor, which is sized for G m |d|^-3, not for a bare |d|^-3)
    c->equal_mass_word = uni_allowed;
    return;
  }
  // packed one-sided kernel, exact d == 0: the same detector lets the tiles that hold no self pair run unguarded
  // (N = 2^20: 276.8 -> 248.8 ms).  Below N = 32768 the detector's two extra launches cost more than they save
  // (N = 8192: 27 -> 43 us).
  const bool packed = p.precision != NBODY_PREC_F64 && !c->wave && c->ipt % 2 == 0;
  if (packed && exact && p.n_total >= 32768) {
    c->dup_slots = detector_slots(p.n_total);                        // as sparse as the symmetric pass's: short chains
    c->dup_tables = 1;
  }
  // equal-mass form of the packed one-sided kernel and of the block kernel (not small_pk_kernel)
  c->equal_mass_word = p.precision != NBODY_PREC_F64 && ((c->wave >= 2 && p.precision == NBODY_PREC_F32) || packed) &&
                       p.zero_mode != NBODY_ZERO_SELECT && uni_allowed;
}

}  // namespace

// Register pairs per workgroup for the block kernel.  A CU works through its workgroups two at a time (2 waves per SIMD at
// ~200 VGPRs) and a workgroup left alone runs about twice as fast, so a CU's time is its number of workgroups times the
// pairs each one carries: the bodies are cut so that ceil(workgroups / CUs) * pairs is smallest, larger workgroups first on
// a tie (fewer prologues).  Measured against all of 2 ... 8 at fifteen sizes (profiles/r03_block_kernel_np_by_n.txt): the
// rule picks the fastest or within 6 % of it.  A function of n_total and the CU count only.
int block_pairs(int n_total, int cus) {
  { const int v = env_int("NBODY_BLOCK_NP", 0); if (v >= 1 && v <= 8) return v; }   // tuning only
  if (cus <= 0) cus = 256;
  int best = 8;
  long long best_cost = -1;
  for (int np = 8; np >= 2; --np) {
    const long long wgs = (n_total + 2 * np - 1) / (2 * np);
    const long long cost = (wgs + cus - 1) / cus * np;
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = np; }
  }
  return best;
}

size_t detector_table_bytes(int slots) { return (size_t)slots * 8 + 64; }

int validate_params(const nbody_params &p, std::string *why) {
  if (p.struct_size != sizeof(nbody_params))
    return refuse(why, NBODY_ERR_INVALID, "nbody_create: struct_size %u != %zu", p.struct_size, sizeof(nbody_params));
  if (p.n_total <= 0) return refuse(why, NBODY_ERR_INVALID, "nbody_create: n_total must be > 0");
  if (p.i_begin < 0 || p.i_begin >= p.n_total) return refuse(why, NBODY_ERR_INVALID, "nbody_create: i_begin out of range");
  const int i_count = owned_count(p);
  if (i_count < 0 || p.i_begin + i_count > p.n_total)
    return refuse(why, NBODY_ERR_INVALID, "nbody_create: owned range [%d,%d) exceeds n_total %d", p.i_begin, p.i_begin + i_count, p.n_total);
  if (p.precision != NBODY_PREC_F32 && p.precision != NBODY_PREC_F32_KAHAN && p.precision != NBODY_PREC_F64)
    return refuse(why, NBODY_ERR_INVALID, "nbody_create: unknown precision %d", p.precision);
  if (!(p.eps >= 0.0) || !std::isfinite(p.G)) return refuse(why, NBODY_ERR_INVALID, "nbody_create: bad G/eps");
  if (!(p.theta >= 0.0f)) return refuse(why, NBODY_ERR_INVALID, "nbody_create: theta must be >= 0");
  if (p.tile != 0 && p.tile != 64 && p.tile != 128 && p.tile != 256 && p.tile != 512)
    return refuse(why, NBODY_ERR_INVALID, "nbody_create: tile must be 64, 128, 256 or 512");
  if (p.i_per_thread != 0 && p.i_per_thread != 1 && p.i_per_thread != 2 && p.i_per_thread != 4 && p.i_per_thread != 8 &&
      p.i_per_thread != 16)
    return refuse(why, NBODY_ERR_INVALID, "nbody_create: i_per_thread must be 1, 2, 4, 8 or 16");
  if (p.i_per_thread == 16 && (p.algorithm == NBODY_ALGO_TILED || p.precision != NBODY_PREC_F32))
    return refuse(why, NBODY_ERR_UNSUPPORTED, "nbody_create: i_per_thread 16 exists for the plain fp32 symmetric kernel only");
  if (p.i_per_thread == 8 && (p.algorithm == NBODY_ALGO_TILED || p.precision == NBODY_PREC_F64))
    return refuse(why, NBODY_ERR_UNSUPPORTED, "nbody_create: i_per_thread 8 exists for the fp32 symmetric kernels only");
  if (p.j_split < 0) return refuse(why, NBODY_ERR_INVALID, "nbody_create: j_split must be >= 0");
  if (p.zero_mode < 0 || p.zero_mode > NBODY_ZERO_FLOOR) return refuse(why, NBODY_ERR_INVALID, "nbody_create: unknown zero_mode %d", p.zero_mode);
  if (p.algorithm < 0 || p.algorithm > NBODY_ALGO_SYMMETRIC) return refuse(why, NBODY_ERR_INVALID, "nbody_create: unknown algorithm %d", p.algorithm);
  if (p.bh_div_mode != 0 && p.bh_div_mode != 1) return refuse(why, NBODY_ERR_INVALID, "nbody_create: bh_div_mode must be 0 or 1");
  return NBODY_OK;
}

int choose_policy(const nbody_params &p, DeviceFacts dev, LaunchPolicy *out, std::string *why) {
  *out = LaunchPolicy();
  const int cus = dev.cus > 0 ? dev.cus : 256;
  std::string reason;
  choose_geometry(p, cus, out);
  choose_algorithm(p, cus, dev.total_bytes, out, &reason);
  if ((p.i_per_thread == 8 || p.i_per_thread == 16) && !(out->sym && out->sym_bi == 256 * p.i_per_thread))
    return refuse(why, NBODY_ERR_UNSUPPORTED,
                  "nbody_create: i_per_thread %d needs the fp32 symmetric kernel (N >= 9216 or NBODY_ALGO_SYMMETRIC; "
                  "sharded slices in multiples of %d bodies)", p.i_per_thread, 256 * p.i_per_thread);
  if (p.algorithm == NBODY_ALGO_SYMMETRIC && !out->sym)
    return refuse(why, NBODY_ERR_UNSUPPORTED,
                  "nbody_create: NBODY_ALGO_SYMMETRIC needs fp32 (i_per_thread 2, 4, 8 or 16, zero_mode != SELECT) or "
                  "fp64 (i_per_thread 2 or 4) and, when sharded, equal slices that are a multiple of 256*i_per_thread bodies%s%s",
                  reason.empty() ? "" : " — ", reason.c_str());
  choose_allocations(p, out);
  return NBODY_OK;
}

void forces_geometry(int wave, int precision, int ipt, int j_split, int i_count, int *blocks, int *threads) {
  constexpr int kBlock = 256;
  if (threads) *threads = kBlock;
  if (!blocks) return;
  if (wave != 0) {
    const int per = precision == NBODY_PREC_F32 ? 2 * wave : wave;   // bodies of a workgroup
    *blocks = (i_count + per - 1) / per;
  } else {
    *blocks = (i_count + kBlock * ipt - 1) / (kBlock * ipt) * j_split;
  }
}

const char *force_kernel_name(bool sym, int wave, int ipt, const nbody_params &p, float theta) {
  if (theta > 0.0f) return p.n_total <= 4096 ? "bh_walk_compact_kernel (+ bh_small_build_kernel)" : "bh_walk_lane_kernel (+ tree build)";
  if (sym) return p.precision == NBODY_PREC_F64 ? "forces_sym_f64_kernel" : "forces_sym_pk_kernel";
  if (wave) return p.precision == NBODY_PREC_F32 ? "forces_block_pk_kernel" : "forces_block_kernel";
  if (p.precision != NBODY_PREC_F64 && ipt % 2 == 0 && (p.eps > 0.0 || p.zero_mode != NBODY_ZERO_SELECT))
    return "forces_tile_pk_kernel";
  return "forces_tile_kernel";
}

}  // namespace nbody

extern "C" int32_t nbody_block_pairs_describe(int32_t n_total, int32_t compute_units) {
  return n_total > 0 ? nbody::block_pairs(n_total, compute_units) : 0;
}

extern "C" int nbody_launch_policy_describe(const nbody_params *pin, int32_t compute_units, uint64_t device_total_bytes,
                                            nbody_launch_policy *out) try {
  using nbody::g_create_error;
  if (!pin || !out || out->struct_size != sizeof(nbody_launch_policy)) { g_create_error = "nbody_launch_policy_describe: null argument or struct_size"; return NBODY_ERR_INVALID; }
  std::string why;
  if (int rc = nbody::validate_params(*pin, &why)) { g_create_error = why; return rc; }
  nbody_params p = *pin;
  p.i_count = nbody::owned_count(p);
  nbody::LaunchPolicy pol;
  if (int rc = nbody::choose_policy(p, nbody::DeviceFacts{compute_units, device_total_bytes}, &pol, &why)) { g_create_error = why; return rc; }
  g_create_error.clear();
  memset(out, 0, sizeof *out);
  out->struct_size = (uint32_t)sizeof *out;
  out->tile = pol.tile; out->i_per_thread = pol.sym ? pol.sym_bi / 256 : pol.ipt; out->j_split = pol.j_split;
  nbody::forces_geometry(pol.wave, p.precision, pol.ipt, pol.j_split, p.i_count, &out->blocks, &out->threads);
  if (pol.sym) { out->blocks = pol.sym_items_n; out->threads = 256; }
  out->algorithm = pol.sym ? NBODY_ALGO_SYMMETRIC : NBODY_ALGO_TILED;
  out->super_tile = pol.sym ? pol.sym_bi : 0;
  out->plan_is_even = pol.sym && pol.sym_even ? 1 : 0;
  out->phases = pol.sym ? (int32_t)pol.plan.phase_item0.size() - 1 : 0;
  out->pool_bytes = pol.sym ? pol.sym_pool_elems * (p.precision == NBODY_PREC_F64 ? 32u : 16u) : 0;
  out->exchange_ranks = pol.sym && pol.sym_nsrc > 1 ? pol.sym_nsrc : 0;
  out->wave = pol.wave;
  out->detector_slots = pol.dup_slots;
  if (pol.sym) { out->sym_slots = pol.sym_slots; out->sym_min_sub = pol.sym_min_sub; out->sym_k = pol.sym_k; }
  snprintf(out->kernel, sizeof out->kernel, "%s", nbody::force_kernel_name(pol.sym, pol.wave, pol.ipt, p, p.theta));
  return NBODY_OK;
} catch (const std::bad_alloc &) {
  nbody::g_create_error = "nbody_launch_policy_describe: out of host memory";
  return NBODY_ERR_NOMEM;
}
