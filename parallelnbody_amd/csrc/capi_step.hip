// The passes of the C-ABI (include/nbody.h) and what drives them: the launch structs of the all-pairs passes, the two-go sharded force
// pass and the one-launch step, the step calls, nbody_tick, and the reductions over the bodies (bounds, energy, moments).  Host C++
// like capi.hip; what it shares with the other host units: capi_common.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bh_driver.h"
#include "capi_common.h"
#include "ctx.h"

namespace {
using nbody::check_ready; using nbody::detector_table_bytes; using nbody::ensure_floor; using nbody::ensure_probe_part; using nbody::env_flag; using nbody::env_int; using nbody::fail; using nbody::make_launch; using nbody::mirror_device_ptr; using nbody::multi_rc;
using nbody::multi_unsupported; using nbody::queue_particle_mirror; using nbody::queue_probe; using nbody::read_energy; using nbody::run_forces; using nbody::run_update; using nbody::scatter_records; using nbody::timed_launch; using nbody::use_device;

// eps^2 of the context's pair law: its own, or the floor of NBODY_ZERO_FLOOR once ensure_floor has computed it
double pair_eps2(const nbody_ctx *c) {
  const double eps2 = c->p.eps * c->p.eps;
  return (eps2 == 0.0 && c->p.zero_mode == NBODY_ZERO_FLOOR && c->floor_eps2 > 0.0) ? c->floor_eps2 : eps2;
}

// the coincident-body detector's table, cleared on the context's stream
hipError_t clear_dup_table(const nbody_ctx *c, void *table) {
  return hipMemsetAsync(table, 0, detector_table_bytes(c->sym_dup_slots), c->stream);
}

// Fused stepping (update_sym_fused_kernel) is for fp32 symmetric contexts that own all bodies AND their position buffer:
// then nothing but this library's kernels moves a body, and the update can prepare the next pass.
bool sym_fused(const nbody_ctx *c) {
  static const bool off = env_flag("NBODY_SYM_NO_FUSE") == 1;   // A/B measurements only; latched at first use
  return !off && c->sym && c->p.precision != NBODY_PREC_F64 && c->sym_nsrc == 1 && c->own_posm && !c->posm_escaped &&
         c->sym_phase_item0.size() == 2 &&
         (c->sym_dup_table == nullptr || c->sym_dup_table2 != nullptr);
}

nbody::SymLaunch make_sym_launch(const nbody_ctx *c) {
  nbody::SymLaunch L;
  L.posm = c->posm; L.posg = c->sym_posg; L.pool = c->sym_pool; L.items = c->sym_items; L.n_items = c->sym_items_n;
  L.i_ptr = c->sym_iptr; L.i_off = c->sym_ioff; L.j_ptr = c->sym_jptr; L.j_off = c->sym_joff;
  L.send = c->sym_send; L.recv = c->sym_recv;
  L.n_total = c->p.n_total; L.n_pad = c->sym_pad; L.n_src = c->sym_nsrc;
  L.np = c->sym_np;
  L.even = c->sym_even ? 1 : 0; L.wrap = c->sym_n_gran * 64;
  L.precision = c->p.precision == NBODY_PREC_F64 ? NBODY_PREC_F64 : NBODY_PREC_F32;
  L.kahan = c->p.precision == NBODY_PREC_F32_KAHAN ? 1 : 0;
  L.G = c->p.G; L.eps2 = pair_eps2(c);
  L.dup_table = c->sym_dup_table; L.dup_slots = c->sym_dup_slots;
  L.general = c->sym_general;
  L.n_local = c->sym_n_local; L.own_begin = c->p.i_begin; L.own_count = c->p.i_count;
  // the host's own finding is final while nothing but this library writes the position buffer; otherwise "not equal"
  // still is (the device word is sticky), "equal" is only the state of things at the last upload
  // (fp64 always asks the device: its test also looks for bodies out where the padding is)
  L.uni_host = c->masses_equal == 0 ? 0 : ((c->masses_equal == 1 && c->own_posm && !c->posm_escaped &&
                                            c->p.precision != NBODY_PREC_F64) ? 1 : -1);
  if (sym_fused(c)) {
    L.fused = 1;
    L.skip_prep = c->sym_posg_valid ? 1 : 0;
    if (c->sym_dup_table) {
      L.dup_table = c->sym_dup_cur ? c->sym_dup_table2 : c->sym_dup_table;
      L.dup_table_next = c->sym_dup_cur ? c->sym_dup_table : c->sym_dup_table2;
    }
  }
  L.clk = c->clk;
  return L;
}

}  // namespace

nbody::ForceLaunch nbody::make_launch(const nbody_ctx *c) {
  nbody::ForceLaunch L;
  L.posm = c->posm; L.accp = c->accp;
  L.n_total = c->p.n_total; L.i_begin = c->p.i_begin; L.i_count = c->p.i_count;
  L.tile = c->tile; L.ipt = c->ipt; L.j_split = c->j_split; L.j_chunk = c->j_chunk;
  L.G = c->p.G; L.eps2 = pair_eps2(c); L.precision = c->p.precision;
  L.zero_mode = (c->p.zero_mode == NBODY_ZERO_SELECT) ? 2 : 1;
  L.wave = c->wave;
  L.guarded = env_int("NBODY_SYM_GUARDED", 0) == 1 ? 1 : 0;        // A/B measurements and tests: no bare pair law anywhere
  L.dup_table = c->sym_dup_table; L.dup_slots = c->sym_dup_slots;
  // equal-mass form of the packed one-sided kernel: the host's scan of the uploaded state stands while nothing else writes
  // the position buffer ("not equal" always stands: the device word is sticky); otherwise the device looks before the launch
  L.general = c->sym_general;
  L.check_masses = (c->sym_general && c->masses_equal != 0 && !(c->masses_equal == 1 && c->own_posm && !c->posm_escaped)) ? 1 : 0;
  // block kernel: which form to launch — the host's finding if it stands, both (each looks at the device word) otherwise
  L.uni = (!c->sym_general || c->masses_equal == 0) ? 0 : (L.check_masses ? -1 : 1);
  L.clk = c->clk;
  return L;
}

// NBODY_ZERO_FLOOR: the smallest eps^2 for which G*m_max*(eps^2)^(-3/2) stays below FLT_MAX/8.
int nbody::ensure_floor(nbody_ctx *c) {
  if (c->p.zero_mode != NBODY_ZERO_FLOOR || c->p.eps > 0.0 || c->floor_eps2 > 0.0) return NBODY_OK;
  HIP_TRY(c, hipMemsetAsync(c->scratch, 0, 4, c->stream));
  HIP_TRY(c, nbody::launch_massmax(c->p.precision, c->posm, c->p.n_total, (unsigned int *)c->scratch, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_scratch, c->scratch, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  float mmax;
  memcpy(&mmax, c->h_scratch, 4);
  const double gm = std::fabs(c->p.G) * (double)mmax;
  const double lim = (c->p.precision == NBODY_PREC_F64) ? 1e300 : 3.0e38 / 8.0;
  double f = gm > 0 ? std::pow(gm / lim, 2.0 / 3.0) : 0.0;
  const double tiny = (c->p.precision == NBODY_PREC_F64) ? 1e-280 : 1e-30;
  c->floor_eps2 = f > tiny ? f : tiny;
  return NBODY_OK;
}

// theta == 0: the field of the bodies at their CURRENT positions at m points, queued (the context's own pair law: G, eps, zero_mode —
// compare+select contexts get the clamp form, which drops the same pairs).  dt > 0: the points are the tracers and move.
int nbody::queue_probe(nbody_ctx *c, void *pts, void *vel, void *acc, int m, float dt) {
  nbody::ProbeLaunch L;
  L.posm = c->posm; L.probe = pts; L.part = c->probe_part; L.acc = acc; L.pos_out = pts; L.vel = vel;
  L.n_total = c->p.n_total; L.m = m;
  L.G = c->p.G; L.eps2 = pair_eps2(c);
  L.dt = dt;
  L.clk = c->clk;
  HIP_TRY(c, nbody::launch_probe(L, c->stream));
  return NBODY_OK;
}

namespace {
// The tracers' share of a theta == 0 step, queued IN FRONT of the bodies' force and update launches of that step: it reads the
// positions the step's force pass uses, and the stream's order does the rest.  dt == 0: accelerations only.
int queue_tracers(nbody_ctx *c, float dt) {
  if (c->tr_n <= 0) return NBODY_OK;
  if (int rc = ensure_probe_part(c, c->tr_n)) return rc;         // (the first theta == 0 pass with these tracers makes it: a theta > 0 context never does)
  return queue_probe(c, c->tr_pos, c->tr_vel, c->tr_acc, c->tr_n, dt);
}

// the all-pairs force pass, queued.  phase (SymLaunch::phase): 0 the whole pass; 1 / 2 the two goes of a sharded fp32 symmetric context (sym_two_goes)
int queue_forces(nbody_ctx *c, int phase) {
  if (c->sym) {
    nbody::SymLaunch L = make_sym_launch(c);
    L.phase = phase;
    // a fused context about to run the preparation kernel again (new state): its current table may hold the entries
    // the last update left for positions that are gone
    if (L.fused && !L.skip_prep && L.dup_table && L.eps2 == 0.0)
      HIP_TRY(c, clear_dup_table(c, L.dup_table));
    if (c->p.precision == NBODY_PREC_F64) {
      HIP_TRY(c, nbody::launch_forces_sym(L, c->stream));          // the fp64 launcher runs its whole pass
    } else {
      // this go's items (phase: 0 all, 1 the strips inside the own slice, 2 the others), pool phase by pool phase: a pool
      // phase's j-side sums are folded into `send` as soon as its last item has been launched, and the next one reuses
      // the area (sym_plan.h).  One pool phase and phase 0: a single call, as ever.
      const int r0 = phase == 2 ? c->sym_n_local : 0, r1 = phase == 1 ? c->sym_n_local : c->sym_items_n;
      const int n_ph = (int)c->sym_phase_item0.size() - 1;
      bool first = true;
      for (int q = 0; q < n_ph; ++q) {
        const int a = std::max(c->sym_phase_item0[(size_t)q], r0), b = std::min(c->sym_phase_item0[(size_t)q + 1], r1);
        if (a >= b && !(first && q == n_ph - 1)) continue;           // nothing of this pool phase in this go (but every go prepares)
        L.item0 = a < b ? a : r0; L.item1 = a < b ? b : r0;
        L.do_prep = first ? 1 : 0;
        // a go with nothing to launch (a plan without remote strips: every item — and with its last item every pool phase's
        // fold — went out in the first go) prepares and folds NOTHING again: a second fold of the last pool phase would add its
        // j-side sums to `send` twice.  What the go's preparation entered into the coincident-body table is cleared by hand.
        const bool folded_in_first_go = phase == 2 && c->sym_n_local >= c->sym_phase_item0[(size_t)q + 1];
        L.do_fold = (a < b && b == c->sym_phase_item0[(size_t)q + 1]) || (phase != 1 && q == n_ph - 1 && a >= b && !folded_in_first_go) ? 1 : 0;
        L.fold_accumulate = q > 0 ? 1 : 0;
        L.clear_detector = q == n_ph - 1 ? 1 : 0;
        L.j_ptr = (const unsigned int *)c->sym_jptr + (size_t)q * ((size_t)c->sym_n_gran + 1);
        HIP_TRY(c, nbody::launch_forces_sym(L, c->stream));
        if (a >= b && folded_in_first_go && L.dup_table && L.eps2 == 0.0)
          HIP_TRY(c, clear_dup_table(c, L.dup_table));
        first = false;
      }
    }
  } else {
    HIP_TRY(c, nbody::launch_forces(make_launch(c), c->stream));
  }
  return NBODY_OK;
}

// ComputeCubeSize of the owned bodies' current positions, queued: its bit pattern arrives in h_scratch
int queue_bounds(nbody_ctx *c) {
  HIP_TRY(c, hipMemsetAsync(c->scratch, 0, 4, c->stream));
  HIP_TRY(c, nbody::launch_bounds(c->p.precision, c->posm, c->p.i_begin, c->p.i_count, (unsigned int *)c->scratch, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_scratch, c->scratch, 4, hipMemcpyDeviceToHost, c->stream));
  return NBODY_OK;
}

}  // namespace

// one force pass; theta > 0: the Barnes-Hut walk into bh_acc, waited for (bh_driver.h; diagnostic: nbody_compute_forces' pass, part of no frame)
// tracer_dt >= 0 (nbody_step, nbody_compute_forces): the pass also carries the tracers, if any (theta > 0: the frame does, bh_driver.hip)
int nbody::run_forces(nbody_ctx *c, bool diagnostic, int phase, float tracer_dt) {
  if (c->theta > 0.0f) return nbody::bh_run_forces(c, diagnostic);
  { int rc = ensure_floor(c); if (rc) return rc; }
  return timed_launch(c, NBODY_KERNEL_FORCES, [&] {
    if (c->tr_n > 0 && tracer_dt >= 0.0f) { if (int rc = queue_tracers(c, tracer_dt)) return rc; }
    return queue_forces(c, phase);
  }, phase != 1);   // two goes are ONE pass
}

int nbody::run_update(nbody_ctx *c, float dt) {
  if (c->theta > 0.0f) return nbody::bh_queue_update(c, dt);
  return timed_launch(c, NBODY_KERNEL_UPDATE, [&]() -> int {
    if (c->sym) {
      const nbody::SymLaunch L = make_sym_launch(c);
      HIP_TRY(c, nbody::launch_update_sym(L, c->posm, c->vel, c->acc, c->p.i_begin, c->p.i_count, dt, c->stream));
      if (L.fused) { c->sym_posg_valid = true; c->sym_dup_cur ^= 1; }   // the update wrote posg and the other table
    } else {
      HIP_TRY(c, nbody::launch_update(c->p.precision, c->posm, c->vel, c->acc, c->accp, c->p.i_begin, c->p.i_count,
                                      c->j_split, dt, c->stream));
    }
    return NBODY_OK;
  });
}

// The position buffer becomes visible to (or is replaced by) the caller: bodies may move behind the library's back from
// now on, so fused stepping and the buffer-swapping one-launch step end here, for the life of the context.  The detector
// table the two-kernel path uses may still hold what the last fused update left in it.
int nbody::posm_escapes(nbody_ctx *c) {
  if (c->posm_escaped) return NBODY_OK;
  if (c->sym_dup_table2)
    HIP_TRY(c, clear_dup_table(c, c->sym_dup_table));
  c->posm_escaped = true;
  c->sym_posg_valid = false;
  if (c->bh) nbody::bh_positions_external(c->bh);
  return NBODY_OK;
}

extern "C" {

// A sharded symmetric context has an exchange between the force pass and the update: the caller must drive
// nbody_step_begin -> all-to-all(nbody_exchange_info) -> nbody_step_end.
static int needs_phases(nbody_ctx *c, const char *who) {
  if (c->theta > 0.0f) return NBODY_OK;
  if (c->sym && c->sym_nsrc > 1)
    return fail(c, NBODY_ERR_STATE, "%s: this sharded context uses the symmetric algorithm; drive it with "
                "nbody_step_begin / all-to-all of nbody_exchange_info buffers / nbody_step_end", who);
  return NBODY_OK;
}

int nbody_step_begin(nbody_ctx *c) {
  if (c && c->multi) return multi_unsupported(c, "nbody_step_begin");
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->step_open || c->step_local) return fail(c, NBODY_ERR_STATE, "nbody_step_begin: previous step not ended");
  HIP_TRY(c, hipSetDevice(c->p.device));
  if ((rc = run_forces(c))) return rc;
  c->step_open = true;
  return NBODY_OK;
}

// Can the force pass run in two goes — the strips inside the own slice first, the rest once the other ranks' positions
// are in?  Sharded fp32 symmetric contexts (all-pairs): their preparation kernel and their plan know the cut.
static bool sym_two_goes(const nbody_ctx *c) {
  return c->theta == 0.0f && c->sym && c->sym_nsrc > 1 && c->p.precision != NBODY_PREC_F64;
}

int nbody_step_begin_local(nbody_ctx *c) {
  if (c && c->multi) return multi_unsupported(c, "nbody_step_begin_local");
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->step_open || c->step_local) return fail(c, NBODY_ERR_STATE, "nbody_step_begin_local: previous step not ended");
  if (sym_two_goes(c)) { if ((rc = run_forces(c, false, 1))) return rc; }   // otherwise everything happens in the second go
  c->step_local = true;
  return NBODY_OK;
}

int nbody_step_begin_remote(nbody_ctx *c) {
  if (c && c->multi) return multi_unsupported(c, "nbody_step_begin_remote");
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->step_local) return fail(c, NBODY_ERR_STATE, "nbody_step_begin_remote: nbody_step_begin_local first");
  c->step_local = false;
  if ((rc = run_forces(c, false, sym_two_goes(c) ? 2 : 0))) return rc;
  c->step_open = true;
  return NBODY_OK;
}

int nbody_step_end(nbody_ctx *c, float dt) {
  if (c && c->multi) return multi_unsupported(c, "nbody_step_end");
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->step_open) return fail(c, NBODY_ERR_STATE, "nbody_step_end: no step begun");
  HIP_TRY(c, hipSetDevice(c->p.device));
  c->step_open = false;
  if ((rc = run_update(c, dt > 0.0f ? dt : 0.0f))) return rc;
  if (dt > 0.0f) { c->steps_done += 1; nbody::hermite_invalidate(c); }
  return NBODY_OK;
}

int nbody_exchange_info(nbody_ctx *c, void **send, void **recv, size_t *bytes_per_rank, int32_t *n_ranks) {
  if (c && c->multi) { if (send) *send = nullptr; if (recv) *recv = nullptr; if (bytes_per_rank) *bytes_per_rank = 0; if (n_ranks) *n_ranks = 0; return NBODY_OK; }
  if (!c) return NBODY_ERR_INVALID;
  const bool ex = c->sym && c->sym_nsrc > 1;
  if (send) *send = ex ? c->sym_send : nullptr;
  if (recv) *recv = ex ? c->sym_recv : nullptr;
  if (bytes_per_rank) *bytes_per_rank = ex ? (size_t)c->p.i_count * c->elem : 0;
  if (n_ranks) *n_ranks = ex ? c->sym_nsrc : 0;
  return NBODY_OK;
}

int nbody_exchange_read_send(nbody_ctx *c, void *host) {
  if (c && c->multi) return multi_unsupported(c, "nbody_exchange_read_send");
  if (!c || !host) return NBODY_ERR_INVALID;
  if (!(c->sym && c->sym_nsrc > 1)) return fail(c, NBODY_ERR_STATE, "nbody_exchange_read_send: this context has no exchange step");
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(host, c->sym_send, (size_t)c->p.n_total * c->elem, hipMemcpyDeviceToHost));
  return NBODY_OK;
}

int nbody_exchange_write_recv(nbody_ctx *c, const void *host) {
  if (c && c->multi) return multi_unsupported(c, "nbody_exchange_write_recv");
  if (!c || !host) return NBODY_ERR_INVALID;
  if (!(c->sym && c->sym_nsrc > 1)) return fail(c, NBODY_ERR_STATE, "nbody_exchange_write_recv: this context has no exchange step");
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(c->sym_recv, host, (size_t)c->sym_nsrc * c->p.i_count * c->elem, hipMemcpyHostToDevice));
  return NBODY_OK;
}

int nbody_bind_exchange(nbody_ctx *c, void *send, void *recv) {
  if (c && c->multi) return multi_unsupported(c, "nbody_bind_exchange");
  if (!c) return NBODY_ERR_INVALID;
  if (!(c->sym && c->sym_nsrc > 1)) return fail(c, NBODY_ERR_STATE, "nbody_bind_exchange: this context has no exchange step");
  if (!send || !recv) return fail(c, NBODY_ERR_INVALID, "nbody_bind_exchange: null buffer");
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->own_send) (void)hipFree(c->sym_send);
  if (c->own_recv) (void)hipFree(c->sym_recv);
  c->sym_send = send; c->sym_recv = recv; c->own_send = c->own_recv = false;
  return NBODY_OK;
}

int nbody_compute_forces(nbody_ctx *c) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->multi) return multi_rc(c, nbody::multi_forces(c->multi, 0.0f));
  if ((rc = needs_phases(c, "nbody_compute_forces"))) return rc;
  HIP_TRY(c, hipSetDevice(c->p.device));
  if ((rc = run_forces(c, true, 0, 0.0f))) return rc;
  if ((rc = run_update(c, 0.0f))) return rc;
  return NBODY_OK;
}

// Small and mid-size single-context fp32 systems (forces_block_pk_kernel): forces + update in ONE launch per step, ping-ponging
// the position buffer — not once the caller holds a pointer to one of the two buffers, and the host must know the masses.
static bool one_launch_ok(const nbody_ctx *c) {
  return c->wave != 0 && c->theta == 0.0f && c->own_posm && !c->posm_escaped && c->p.i_count == c->p.n_total &&
         (c->p.precision != NBODY_PREC_F32 || make_launch(c).uni >= 0);
}

// one such step; stage / size_bits / size_zero: the frame's mirror and ComputeCubeSize from the same launch (nbody_tick)
static int step_one_launch(nbody_ctx *c, float dt, void *stage, void *size_bits, void *size_zero) {
  int rc;
  if (!c->posm_alt) HIP_TRY(c, hipMalloc(&c->posm_alt, (size_t)c->p.n_total * c->elem));
  if ((rc = ensure_floor(c))) return rc;
  rc = timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
    if (c->tr_n > 0) { if (int trc = queue_tracers(c, dt)) return trc; }   // (they read c->posm, which this launch only reads)
    HIP_TRY(c, nbody::launch_step_small(make_launch(c), c->posm_alt, c->vel, c->acc, dt, c->stream, stage, size_bits, size_zero));
    return NBODY_OK;
  });
  if (rc) return rc;
  std::swap(c->posm, c->posm_alt);
  return NBODY_OK;
}

int nbody_step(nbody_ctx *c, float dt, int32_t nsteps) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (nsteps < 0) return fail(c, NBODY_ERR_INVALID, "nbody_step: nsteps < 0");
  if (!(dt > 0.0f)) return NBODY_OK;   // OctreeSearch.cpp:25: PhDeltaTime <= 0 freezes the physics
  nbody::hermite_invalidate(c);
  if (c->multi) {
    if (c->theta > 0.0f) {                                        // whole frames on every device, one wait per batch (multi_bh_steps)
      int built = 0;
      rc = multi_rc(c, nbody::multi_bh_steps(c->multi, dt, nsteps, &built));
      c->steps_done += built;
      return rc;
    }
    for (int s = 0; s < nsteps; ++s) {
      if ((rc = multi_rc(c, nbody::multi_forces(c->multi, dt)))) return rc;
      c->steps_done += 1;
    }
    return NBODY_OK;
  }
  if ((rc = needs_phases(c, "nbody_step"))) return rc;
  if (nsteps > 1 && c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_STATE, "nbody_step: a sharded context advances one step per call (all-gather NBODY_BUF_POSM in between)");
  HIP_TRY(c, hipSetDevice(c->p.device));
  if (c->theta > 0.0f) {
    if ((rc = nbody::ensure_bh(c))) return rc;
    // every frame queued, one wait per call — the larger systems' in batches of 64: a frame their warm sort gives up takes the
    // frames queued behind it along (bh_drive queues them again), and that should not be hundreds
    const int batch = nbody::bh_is_small(c->bh) ? nsteps : 64;
    for (int done = 0; done < nsteps; done += batch)
      if ((rc = nbody::bh_run_frames(c, dt, std::min(batch, nsteps - done), nullptr))) return rc;
    return NBODY_OK;
  }
  const bool one_launch = one_launch_ok(c);
  for (int s = 0; s < nsteps; ++s) {
    if (one_launch) {
      if ((rc = step_one_launch(c, dt, nullptr, nullptr, nullptr))) return rc;
      continue;
    }
    if ((rc = run_forces(c, false, 0, dt))) return rc;
    if ((rc = run_update(c, dt))) return rc;
  }
  c->steps_done += nsteps;
  return NBODY_OK;
}

int nbody_get_bounds(nbody_ctx *c, float *size) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!size) return fail(c, NBODY_ERR_INVALID, "nbody_get_bounds: null output");
  if (c->multi) return multi_rc(c, nbody::multi_get_bounds(c->multi, size));
  if ((rc = queue_bounds(c))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(size, c->h_scratch, 4);
  return NBODY_OK;
}

int nbody_energy(nbody_ctx *c, double *ke, double *pe) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->multi) return multi_rc(c, nbody::multi_energy(c->multi, ke, pe));
  if (!c->energy_part)
    HIP_TRY(c, hipMalloc(&c->energy_part, nbody::energy_partials(c->p.n_total, c->p.i_count) * sizeof(double)));
  HIP_TRY(c, nbody::launch_energy(c->p.precision, c->posm, c->vel, c->p.n_total, c->p.i_begin, c->p.i_count, c->p.G,
                                  c->p.eps * c->p.eps, (double *)c->energy_part, (double *)c->scratch, c->stream));
  return read_energy(c, ke, pe);
}

// nbody_get_moments / nbody_mass_within: the slots and results on the device and the results' pinned mirror, on first use
static int ensure_moments(nbody_ctx *c) {
  if (!c->moments_part) HIP_TRY(c, hipMalloc(&c->moments_part, nbody::moments_scratch_bytes(c->p.i_count)));
  if (!c->moments_host) HIP_TRY(c, hipHostMalloc(&c->moments_host, 2 * nbody::kMassWithinMax * 8, hipHostMallocDefault));
  return NBODY_OK;
}

int nbody_get_moments(nbody_ctx *c, nbody_moments *out) {
  if (!c) return NBODY_ERR_INVALID;
  if (!out || out->struct_size != sizeof(nbody_moments))
    return fail(c, NBODY_ERR_INVALID, "nbody_get_moments: null output or struct_size != sizeof(nbody_moments)");
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->multi) return multi_rc(c, nbody::multi_moments(c->multi, out));
  if ((rc = ensure_moments(c))) return rc;
  // the buffers the getters read: c->posm is the live one of the one-launch step's two, c->acc holds every path's stored accelerations
  HIP_TRY(c, nbody::launch_moments(c->p.precision, c->posm, c->vel, c->acc, c->p.i_begin, c->p.i_count, c->moments_part, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->moments_host, c->moments_part, nbody::kMomentValues * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  static_assert(sizeof(nbody_moments) == 16 + nbody::kMomentValues * sizeof(double), "nbody_moments: 24 sums behind the header");
  out->reserved = 0;
  out->count = c->p.i_count;
  memcpy(&out->mass, c->moments_host, nbody::kMomentValues * sizeof(double));
  return NBODY_OK;
}

int nbody_mass_within(nbody_ctx *c, const double centre[3], const double *radii, int32_t k, double *mass, int64_t *count) {
  if (!c) return NBODY_ERR_INVALID;
  if (!centre || !radii || (!mass && !count)) return fail(c, NBODY_ERR_INVALID, "nbody_mass_within: null centre, radii or outputs");
  if (k < 1 || k > nbody::kMassWithinMax) return fail(c, NBODY_ERR_INVALID, "nbody_mass_within: k = %d outside 1 .. %d", k, nbody::kMassWithinMax);
  for (int q = 0; q < k; ++q)
    if (!(radii[q] >= 0.0) || !std::isfinite(radii[q]))
      return fail(c, NBODY_ERR_INVALID, "nbody_mass_within: radius %d is negative or not finite", q);
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->multi) return multi_rc(c, nbody::multi_mass_within(c->multi, centre, radii, k, mass, count));
  if ((rc = ensure_moments(c))) return rc;
  HIP_TRY(c, nbody::launch_mass_within(c->p.precision, c->posm, c->p.i_begin, c->p.i_count, centre, radii, k, c->moments_part, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->moments_host, c->moments_part, 2 * nbody::kMassWithinMax * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (mass) memcpy(mass, c->moments_host, (size_t)k * sizeof(double));
  if (count) memcpy(count, (const char *)c->moments_host + nbody::kMassWithinMax * 8, (size_t)k * sizeof(int64_t));
  return NBODY_OK;
}

// One whole frame of the actor with ONE host synchronisation: ComputeCubeSize of the current positions, the Tick body,
// the FParticle mirror.
int nbody_tick(nbody_ctx *c, float dt, float *size, void *aos, size_t stride) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (aos && stride < sizeof(nbody_particle)) return fail(c, NBODY_ERR_INVALID, "nbody_tick: stride < 40");
  if (c->multi) {                                                // the same frame as three calls: every device has its own stream to wait for
    if (dt > 0.0f && size && (rc = nbody_get_bounds(c, size))) return rc;
    if (dt > 0.0f && (rc = nbody_step(c, dt, 1))) return rc;
    return aos ? nbody_get_particles(c, aos, stride) : nbody_synchronize(c);
  }
  if ((rc = needs_phases(c, "nbody_tick"))) return rc;
  HIP_TRY(c, hipSetDevice(c->p.device));
  const bool live = dt > 0.0f;                                   // OctreeSearch.cpp:25
  if (live) nbody::hermite_invalidate(c);
  // the eps floor of NBODY_ZERO_FLOOR is computed through the same 64-byte scratch the bounds travel in: settle it
  // before the bounds are queued, or the first frame would return the largest mass as Size
  if (live && c->theta == 0.0f && (rc = ensure_floor(c))) return rc;
  // small systems at theta > 0: the tree's own launch computes Size (it is the root's half-width) — the frame is queued
  // here and its verdict collected by the frame's one wait
  bool bh_frame = false;
  if (live && c->theta > 0.0f) {
    if ((rc = nbody::ensure_bh(c))) return rc;
    bh_frame = true;
  }
  const size_t ic = (size_t)c->p.i_count;
  bool direct = false;                                           // the records go straight into the caller's pinned mirror
  // systems on the one-launch step (theta == 0, up to 16384 bodies): the same launch leaves Size (of the positions before
  // the update, as .cpp:26 has it) and the frame's FParticle records — one kernel, the copies, one wait
  if (live && c->theta == 0.0f && (size || aos) && c->p.precision == NBODY_PREC_F32 && one_launch_ok(c)) {
    void *stage = nullptr;
    if (aos && (rc = mirror_device_ptr(c, aos, stride, true, &direct, &stage))) return rc;
    unsigned int *words = (unsigned int *)c->scratch + 8;        // two words that take turns: this frame's (zero), the next one's
    unsigned int *cur = words + c->tick_word, *nxt = words + (c->tick_word ^ 1);
    if ((rc = step_one_launch(c, dt, stage, size ? cur : nullptr, size ? nxt : nullptr))) return rc;
    c->steps_done += 1;
    if (size) { c->tick_word ^= 1; HIP_TRY(c, hipMemcpyAsync(c->h_scratch, cur, 4, hipMemcpyDeviceToHost, c->stream)); }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (size) memcpy(size, c->h_scratch, 4);
    if (aos && !direct) scatter_records(aos, stride, c->h_stage, sizeof(nbody_particle), ic);
    return NBODY_OK;
  }
  void *bh_stage = nullptr;
  if (bh_frame) {                                                // the walk writes the frame's records itself, Size rides with the verdict
    if (aos && (rc = mirror_device_ptr(c, aos, stride, false, &direct, &bh_stage))) return rc;
    if ((rc = nbody::bh_queue_frame(c, dt, false, false, (float *)bh_stage))) return rc;
  } else if (live && size) {                                     // .cpp:26, 47-56: bounds of the positions BEFORE the step
    if ((rc = queue_bounds(c))) return rc;
  }
  if (live && !bh_frame && (rc = nbody_step(c, dt, 1))) return rc;   // .cpp:27-31
  if (aos && !bh_frame && (rc = queue_particle_mirror(c, aos, stride, &direct))) return rc;   // .cpp:33,41: what the frame draws
  int frame_rc = NBODY_OK;
  if (bh_frame) frame_rc = nbody::bh_run_frames(c, dt, 1, (float *)bh_stage, true);   // the frame's one wait (and, given up or handed back, once more)
  else HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (bh_frame && frame_rc != NBODY_OK && aos) {                 // a refused frame wrote no records: deliver the untouched state
    if ((rc = queue_particle_mirror(c, aos, stride, &direct))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (bh_frame) { if (size) *size = nbody::bh_last_size(c->bh); }
  else if (live && size) memcpy(size, c->h_scratch, 4);
  if (aos && !direct) scatter_records(aos, stride, c->h_stage, sizeof(nbody_particle), ic);
  return frame_rc;
}

}  // extern "C"
