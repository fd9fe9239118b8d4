// C-ABI of libnbody_amd.so (include/nbody.h): context, device state, launches (the Hermite calls: capi_hermite.hip; the fp64 queries: capi_query64.hip).  Host C++ over the
// HIP runtime; no torch types, no exceptions across the boundary (the entry points that allocate host memory catch
// std::bad_alloc), no CPU fallback.  Which kernel, geometry and plan a context gets — every size threshold — is decided in
// launch_policy.{h,cpp} (host only, CPU-tested); nbody_create asks the device its CU count and memory and carries the answer out.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>

#include "bh_driver.h"
#include "capi_common.h"
#include "ctx.h"
#include "launch_policy.h"

// ---- what capi_hermite.hip and capi_query64.hip call as well (capi_common.h) ----
namespace nbody {
int multi_unsupported(nbody_ctx *c, const char *who) {
  return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not available on a multi-device context (nbody_create_multi); use one context per device", who);
}

// the partial rows of a slab of `m` points (kernels_probe.hip), grown on demand; freed at nbody_destroy
int ensure_probe_part(nbody_ctx *c, int m, int width) {
  const size_t need = nbody::probe_part_elems(c->p.n_total, m, width);
  if (need <= c->probe_part_elems) return NBODY_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));                      // (a tracer pass may still be reading the old one)
  if (c->probe_part) (void)hipFree(c->probe_part);
  c->probe_part = nullptr; c->probe_part_elems = 0;
  HIP_TRY(c, hipMalloc(&c->probe_part, need * 16));
  c->probe_part_elems = need;
  return NBODY_OK;
}

// (Re)allocate the hand-off staging pair for `bytes`.
int ensure_stage(nbody_ctx *c, size_t bytes) {
  if (bytes <= c->stage_bytes) return NBODY_OK;
  if (c->d_stage) (void)hipFree(c->d_stage);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  c->d_stage = c->h_stage = nullptr; c->stage_bytes = 0;
  HIP_TRY(c, hipMalloc(&c->d_stage, bytes));
  HIP_TRY(c, hipHostMalloc(&c->h_stage, bytes, hipHostMallocDefault));
  c->stage_bytes = bytes;
  return NBODY_OK;
}

// `count` staged records of record_bytes each (src_stride apart: packed unless given) -> the caller's array, records `stride` bytes apart
void scatter_records(void *dst, size_t stride, const void *src, size_t record_bytes, size_t count, size_t src_stride) {
  if (src_stride == 0) src_stride = record_bytes;
  if (stride == record_bytes && src_stride == record_bytes) {
    memcpy(dst, src, count * record_bytes);
    return;
  }
  for (size_t i = 0; i < count; ++i) memcpy((char *)dst + i * stride, (const char *)src + i * src_stride, record_bytes);
}

// the two sums an energy reduction left in the scratch, waited for
int read_energy(nbody_ctx *c, double *ke, double *pe) {
  HIP_TRY(c, hipMemcpyAsync(c->h_scratch, c->scratch, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  double v[2];
  memcpy(v, c->h_scratch, 16);
  if (ke) *ke = v[0];
  if (pe) *pe = v[1];
  return NBODY_OK;
}

int check_ready(nbody_ctx *c) {
  if (!c) return NBODY_ERR_INVALID;
  if (!c->have_state) return fail(c, NBODY_ERR_STATE, "no particles set (call nbody_set_particles / nbody_set_state_soa first)");
  return use_device(c);
}
}  // namespace nbody

namespace {

using nbody::detector_table_bytes; using nbody::env_flag; using nbody::env_int; using nbody::EventPair; using nbody::fail; using nbody::g_create_error; using nbody::timed_launch; using nbody::use_device;
using nbody::check_ready; using nbody::ensure_jerk64; using nbody::ensure_probe_part; using nbody::ensure_stage; using nbody::multi_unsupported; using nbody::queue_body_jerk; using nbody::read_energy; using nbody::scatter_records;

// A call on a multi-device context is answered by its Multi; its message becomes the context's.
int multi_rc(nbody_ctx *c, int rc) {
  if (rc) c->err = nbody::multi_error(c->multi);
  return rc;
}

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

nbody::ForceLaunch make_launch(const nbody_ctx *c) {
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
int ensure_floor(nbody_ctx *c) {
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
int queue_probe(nbody_ctx *c, void *pts, void *vel, void *acc, int m, float dt) {
  nbody::ProbeLaunch L;
  L.posm = c->posm; L.probe = pts; L.part = c->probe_part; L.acc = acc; L.pos_out = pts; L.vel = vel;
  L.n_total = c->p.n_total; L.m = m;
  L.G = c->p.G; L.eps2 = pair_eps2(c);
  L.dt = dt;
  L.clk = c->clk;
  HIP_TRY(c, nbody::launch_probe(L, c->stream));
  return NBODY_OK;
}

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

// one force pass; theta > 0: the Barnes-Hut walk into bh_acc, waited for (bh_driver.h; diagnostic: nbody_compute_forces' pass, part of no frame)
// tracer_dt >= 0 (nbody_step, nbody_compute_forces): the pass also carries the tracers, if any (theta > 0: the frame does, bh_driver.hip)
int run_forces(nbody_ctx *c, bool diagnostic = false, int phase = 0, float tracer_dt = -1.0f) {
  if (c->theta > 0.0f) return nbody::bh_run_forces(c, diagnostic);
  { int rc = ensure_floor(c); if (rc) return rc; }
  return timed_launch(c, NBODY_KERNEL_FORCES, [&] {
    if (c->tr_n > 0 && tracer_dt >= 0.0f) { if (int rc = queue_tracers(c, tracer_dt)) return rc; }
    return queue_forces(c, phase);
  }, phase != 1);   // two goes are ONE pass
}

int run_update(nbody_ctx *c, float dt) {
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

template <typename SRC, typename DST>
void convert4(const SRC *src, DST *dst, size_t n_elems4, bool zero_w) {
  for (size_t i = 0; i < n_elems4; ++i) {
    dst[4 * i + 0] = (DST)src[4 * i + 0];
    dst[4 * i + 1] = (DST)src[4 * i + 1];
    dst[4 * i + 2] = (DST)src[4 * i + 2];
    dst[4 * i + 3] = zero_w ? (DST)0 : (DST)src[4 * i + 3];
  }
}

// A new state arrives from the host: are all masses (as the fp32 kernels will see them) equal?  The device word the
// equal-mass kernels are gated on is reset to that finding.
template <typename T>
int note_masses(nbody_ctx *c, const T *posm4) {
  if (!c->sym_general) return NBODY_OK;
  const bool ctx64 = c->p.precision == NBODY_PREC_F64;
  auto seen = [&](T v) { return ctx64 ? (double)v : (double)(float)v; };
  const double m0 = seen(posm4[3]);
  bool equal = true;
  for (size_t i = 1; i < (size_t)c->p.n_total && equal; ++i) equal = seen(posm4[4 * i + 3]) == m0;
  c->masses_equal = equal ? 1 : 0;
  HIP_TRY(c, hipMemsetAsync(c->sym_general, equal ? 0 : 0xFF, 4, c->stream));
  return NBODY_OK;
}

// Upload host SoA state given as T (float or double); converts to the context's precision.  Every copy goes through the context's
// stream, behind whatever steps are still in flight on it: a copy on the null stream would not wait for them (the stream is
// non-blocking), and their updates would land on top of the new state.
// keep_history: the records of a running simulation edited by the host (nbody_push_particles) — the step count and the
// Barnes-Hut root centre (the previous tree's CoM) stay what they are.
template <typename T>
int upload_soa(nbody_ctx *c, const T *posm4, const T *vel4, bool keep_history = false) {
  if (int rc = use_device(c)) return rc;
  const int n = c->p.n_total, ib = c->p.i_begin, ic = c->p.i_count;
  const bool ctx64 = c->p.precision == NBODY_PREC_F64;
  const bool same = ctx64 == (sizeof(T) == 8);
  // both copies, then ONE wait whatever they returned: a copy that may still be reading its source never outlives it
  auto send = [&](const void *p, size_t p_bytes, const void *v, size_t v_bytes) -> hipError_t {
    const hipError_t e1 = hipMemcpyAsync(c->posm, p, p_bytes, hipMemcpyHostToDevice, c->stream);
    const hipError_t e2 = e1 == hipSuccess ? hipMemcpyAsync(c->vel, v, v_bytes, hipMemcpyHostToDevice, c->stream) : e1;
    const hipError_t e3 = hipStreamSynchronize(c->stream);
    return e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
  };
  if (same) {
    HIP_TRY(c, send(posm4, (size_t)n * c->elem, vel4 + 4 * (size_t)ib, (size_t)ic * c->elem));
  } else if (ctx64) {
    std::vector<double> tp((size_t)n * 4), tv((size_t)ic * 4);
    convert4(posm4, tp.data(), (size_t)n, false);
    convert4(vel4 + 4 * (size_t)ib, tv.data(), (size_t)ic, true);
    HIP_TRY(c, send(tp.data(), tp.size() * 8, tv.data(), tv.size() * 8));
  } else {
    std::vector<float> tp((size_t)n * 4), tv((size_t)ic * 4);
    convert4(posm4, tp.data(), (size_t)n, false);
    convert4(vel4 + 4 * (size_t)ib, tv.data(), (size_t)ic, true);
    HIP_TRY(c, send(tp.data(), tp.size() * 4, tv.data(), tv.size() * 4));
  }
  HIP_TRY(c, hipMemsetAsync(c->acc, 0, (size_t)ic * c->elem, c->stream));
  { const int rc = note_masses(c, posm4); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->have_state = true;
  c->floor_eps2 = -1.0;
  c->sym_posg_valid = false;
  nbody::hermite_invalidate(c);
  if (c->bh) nbody::bh_positions_changed(c->bh);                   // the next Barnes-Hut frame looks at the positions for its Size
  if (keep_history) return NBODY_OK;
  c->steps_done = 0;
  if (c->bh) HIP_TRY(c, nbody::bh_reset_root(c->bh, c->stream));   // a new scene: root centre starts at zero again
  return NBODY_OK;
}

// Download `count` elements starting at element `first` of a device buffer as T x 4.
template <typename T>
int download4(nbody_ctx *c, const void *dev, size_t first, size_t count, T *out) {
  const bool ctx64 = c->p.precision == NBODY_PREC_F64;
  const char *src = (const char *)dev + first * c->elem;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (ctx64 == (sizeof(T) == 8)) {
    HIP_TRY(c, hipMemcpy(out, src, count * c->elem, hipMemcpyDeviceToHost));
  } else if (ctx64) {
    std::vector<double> tmp(count * 4);
    HIP_TRY(c, hipMemcpy(tmp.data(), src, count * 32, hipMemcpyDeviceToHost));
    convert4(tmp.data(), out, count, false);
  } else {
    std::vector<float> tmp(count * 4);
    HIP_TRY(c, hipMemcpy(tmp.data(), src, count * 16, hipMemcpyDeviceToHost));
    convert4(tmp.data(), out, count, false);
  }
  return NBODY_OK;
}

// Is [dst, dst + bytes) inside memory the caller pinned for this context?
bool in_pinned(const nbody_ctx *c, const void *dst, size_t bytes) {
  const char *d = (const char *)dst;
  for (const auto &r : c->pinned)
    if (d >= r.first && d + bytes <= r.first + r.second) return true;
  return false;
}

// Does the caller's FParticle array take the records by DMA — packed, and inside memory it pinned for this context?
bool mirror_is_direct(const nbody_ctx *c, const void *aos, size_t stride) {
  return stride == sizeof(nbody_particle) && in_pinned(c, aos, (size_t)c->p.i_count * sizeof(nbody_particle));
}

// The owned bodies' FParticle records, queued: packed on the device, then copied to the caller's pinned mirror (*direct) or to the
// staging buffer (scatter_records delivers from there once the stream has been waited for).
int queue_particle_mirror(nbody_ctx *c, void *aos, size_t stride, bool *direct) {
  const size_t bytes = (size_t)c->p.i_count * sizeof(nbody_particle);
  if (int rc = ensure_stage(c, bytes)) return rc;
  HIP_TRY(c, nbody::launch_pack_particles(c->p.precision, c->posm, c->vel, c->acc, (float *)c->d_stage, c->p.i_begin,
                                          c->p.i_count, c->stream));
  *direct = mirror_is_direct(c, aos, stride);
  HIP_TRY(c, hipMemcpyAsync(*direct ? aos : c->h_stage, c->d_stage, bytes, hipMemcpyDeviceToHost, c->stream));
  return NBODY_OK;
}

// For the launches that write the frame's records themselves, straight into page-locked host memory — the caller's own mirror if it
// pinned it (nbody_pin_host_buffer; align16: and only if it is 16-byte aligned), the context's staging buffer otherwise: no copy to
// wait for (profiles/r03_tick_parts_n2000.txt: the 80 KB copy of the shipped scene's mirror cost 12.7 us of a 32.7 us frame).
// *dev: that memory's device pointer.
int mirror_device_ptr(nbody_ctx *c, void *aos, size_t stride, bool align16, bool *direct, void **dev) {
  if (int rc = ensure_stage(c, (size_t)c->p.i_count * sizeof(nbody_particle))) return rc;
  *direct = mirror_is_direct(c, aos, stride) && (!align16 || ((uintptr_t)aos & 15u) == 0);
  HIP_TRY(c, hipHostGetDevicePointer(dev, *direct ? aos : c->h_stage, 0));
  return NBODY_OK;
}

// ComputeCubeSize of the owned bodies' current positions, queued: its bit pattern arrives in h_scratch
int queue_bounds(nbody_ctx *c) {
  HIP_TRY(c, hipMemsetAsync(c->scratch, 0, 4, c->stream));
  HIP_TRY(c, nbody::launch_bounds(c->p.precision, c->posm, c->p.i_begin, c->p.i_count, (unsigned int *)c->scratch, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_scratch, c->scratch, 4, hipMemcpyDeviceToHost, c->stream));
  return NBODY_OK;
}

// The position buffer becomes visible to (or is replaced by) the caller: bodies may move behind the library's back from
// now on, so fused stepping and the buffer-swapping one-launch step end here, for the life of the context.  The detector
// table the two-kernel path uses may still hold what the last fused update left in it.
int posm_escapes(nbody_ctx *c) {
  if (c->posm_escaped) return NBODY_OK;
  if (c->sym_dup_table2)
    HIP_TRY(c, clear_dup_table(c, c->sym_dup_table));
  c->posm_escaped = true;
  c->sym_posg_valid = false;
  if (c->bh) nbody::bh_positions_external(c->bh);
  return NBODY_OK;
}

// nbody_set_state_soa / nbody_set_state_soa_f64 (`who`): the whole state as T x 4
template <typename T>
int set_state_soa(nbody_ctx *c, const T *posm4, const T *vel4, int32_t n, const char *who) try {
  if (!c || !posm4 || !vel4) return c ? fail(c, NBODY_ERR_INVALID, "%s: null buffer", who) : NBODY_ERR_INVALID;
  if (n != c->p.n_total) return fail(c, NBODY_ERR_INVALID, "%s: n = %d but the context holds %d bodies", who, n, c->p.n_total);
  if (c->multi) {
    int rc;
    if constexpr (sizeof(T) == 8) rc = nbody::multi_set_state_soa_f64(c->multi, posm4, vel4, n);
    else rc = nbody::multi_set_state_soa(c->multi, posm4, vel4, n);
    if (!multi_rc(c, rc)) { c->have_state = true; c->steps_done = 0; }
    return rc;
  }
  return upload_soa<T>(c, posm4, vel4);
} catch (const std::bad_alloc &) {
  return fail(c, NBODY_ERR_NOMEM, "%s: out of host memory", who);
}

// nbody_get_state_soa / nbody_get_state_soa_f64 (`who`): the owned bodies' state as T x 4, each array optional
template <typename T>
int get_state_soa(nbody_ctx *c, T *posm4, T *vel4, T *acc4, const char *who) try {
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->multi) {
    if constexpr (sizeof(T) == 8) return multi_rc(c, nbody::multi_get_state_soa_f64(c->multi, posm4, vel4, acc4));
    else return multi_rc(c, nbody::multi_get_state_soa(c->multi, posm4, vel4, acc4));
  }
  if (posm4 && (rc = download4<T>(c, c->posm, (size_t)c->p.i_begin, (size_t)c->p.i_count, posm4))) return rc;
  if (vel4 && (rc = download4<T>(c, c->vel, 0, (size_t)c->p.i_count, vel4))) return rc;
  if (acc4 && (rc = download4<T>(c, c->acc, 0, (size_t)c->p.i_count, acc4))) return rc;
  return NBODY_OK;
} catch (const std::bad_alloc &) {
  return fail(c, NBODY_ERR_NOMEM, "%s: out of host memory", who);
}

}  // namespace

extern "C" {

int nbody_version(void) { return NBODY_VERSION_MAJOR * 100 + NBODY_VERSION_MINOR; }

int nbody_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int nbody_default_params(nbody_params *p) {
  if (!p) return NBODY_ERR_INVALID;
  memset(p, 0, sizeof *p);
  p->struct_size = (uint32_t)sizeof(nbody_params);
  p->precision = NBODY_PREC_F32;
  p->G = 1.0e4;      // OctreeSearch.h:104
  p->eps = 0.0;      // OctreeSearch.h:101-104: no softening
  return NBODY_OK;
}

const char *nbody_last_error(const nbody_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int nbody_create(const nbody_params *pin, nbody_ctx **out) try {
  if (!pin || !out) return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: null argument");
  *out = nullptr;
  std::string why;
  if (int rc = nbody::validate_params(*pin, &why)) return fail(nullptr, rc, "%s", why.c_str());
  nbody_params p = *pin;
  p.i_count = nbody::owned_count(p);

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, NBODY_ERR_NO_DEVICE, "nbody_create: no HIP device (%s); this engine has no CPU path",
                e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  if (p.device < 0 || p.device >= ndev)
    return fail(nullptr, NBODY_ERR_NO_DEVICE, "nbody_create: device %d not in [0,%d)", p.device, ndev);
  if ((e = hipSetDevice(p.device)) != hipSuccess)      // before anything that asks the device questions (free memory)
    return fail(nullptr, NBODY_ERR_HIP, "nbody_create: hipSetDevice(%d): %s", p.device, hipGetErrorString(e));

  // the two facts about the device the policy may depend on (launch_policy.h), asked once
  nbody::DeviceFacts dev{0, 0};
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, p.device) == hipSuccess) dev.cus = prop.multiProcessorCount; }
  { size_t free_b = 0, total_b = 0; if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) dev.total_bytes = total_b; }
  nbody::LaunchPolicy pol;
  if (int rc = nbody::choose_policy(p, dev, &pol, &why)) return fail(nullptr, rc, "%s", why.c_str());

  nbody_ctx *c = new (std::nothrow) nbody_ctx();
  if (!c) return fail(nullptr, NBODY_ERR_NOMEM, "nbody_create: out of host memory");
  c->p = p;
  c->theta = p.theta;
  c->elem = (p.precision == NBODY_PREC_F64) ? 32 : 16;
  c->tile = pol.tile; c->ipt = pol.ipt; c->j_split = pol.j_split; c->j_chunk = pol.j_chunk; c->wave = pol.wave;
  c->sym = pol.sym; c->sym_even = pol.sym_even; c->sym_slots = pol.sym_slots; c->sym_k = pol.sym_k; c->sym_min_sub = pol.sym_min_sub;
  c->sym_bi = pol.sym_bi; c->sym_np = pol.sym_np; c->sym_pad = pol.sym_pad; c->sym_items_n = pol.sym_items_n; c->sym_nsrc = pol.sym_nsrc;
  c->sym_pool_elems = (size_t)pol.sym_pool_elems; c->sym_n_local = pol.sym_n_local; c->sym_n_gran = pol.sym_n_gran;
  c->sym_phase_item0 = pol.plan.phase_item0;
  c->sym_dup_slots = pol.dup_slots;

  auto bail = [&](hipError_t he, const char *what, const char *what2 = "") {
    fail(nullptr, NBODY_ERR_HIP, "nbody_create: %s%s: %s", what, what2, hipGetErrorString(he));
    nbody_destroy(c);
    return NBODY_ERR_HIP;
  };
  // allocate and fill from the host: a list of the plan
  auto up = [&](void **dst, const void *src, size_t bytes, const char *what) -> hipError_t {
    hipError_t he = hipMalloc(dst, bytes ? bytes : 4);
    if (he != hipSuccess) { fail(nullptr, NBODY_ERR_HIP, "nbody_create: hipMalloc %s: %s", what, hipGetErrorString(he)); return he; }
    if (bytes) he = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    return he;
  };
  // allocate and zero (zalloc_op: which of the two calls failed).  The fill runs on the null stream: the wait at the end of this
  // function covers every one of them.
  const char *zalloc_op = "";
  auto zalloc = [&](void **dst, size_t bytes) -> hipError_t {
    zalloc_op = "hipMalloc ";
    const hipError_t he = hipMalloc(dst, bytes);
    return he != hipSuccess ? he : (zalloc_op = "hipMemset ", hipMemset(*dst, 0, bytes));
  };
  if ((e = hipSetDevice(p.device)) != hipSuccess) return bail(e, "hipSetDevice");
  if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
  c->stream = c->own_stream;
  if ((e = hipMalloc(&c->posm, (size_t)p.n_total * c->elem)) != hipSuccess) return bail(e, "hipMalloc posm");
  c->own_posm = true;
  if ((e = hipMalloc(&c->vel, (size_t)p.i_count * c->elem)) != hipSuccess) return bail(e, "hipMalloc vel");
  c->own_vel = true;
  if ((e = hipMalloc(&c->acc, (size_t)p.i_count * c->elem)) != hipSuccess) return bail(e, "hipMalloc acc");
  c->own_acc = true;
  const size_t table_bytes = detector_table_bytes(pol.dup_slots);
  if (c->sym) {
    const nbody::SymPlan &P = pol.plan;
    if ((e = hipMalloc(&c->sym_pool, c->sym_pool_elems * c->elem)) != hipSuccess) return bail(e, "hipMalloc partial-sum pool");
    if ((e = up(&c->sym_items, P.items.data(), P.items.size() * sizeof(nbody::SymItem), "work items")) != hipSuccess) return bail(e, "work items");
    if ((e = up(&c->sym_iptr, P.i_ptr.data(), P.i_ptr.size() * 4, "i-side list")) != hipSuccess) return bail(e, "i-side list");
    if ((e = up(&c->sym_ioff, P.i_off.data(), P.i_off.size() * 4, "i-side list")) != hipSuccess) return bail(e, "i-side list");
    if ((e = up(&c->sym_jptr, P.j_ptr.data(), P.j_ptr.size() * 4, "j-side list")) != hipSuccess) return bail(e, "j-side list");
    if ((e = up(&c->sym_joff, P.j_off.data(), P.j_off.size() * 4, "j-side list")) != hipSuccess) return bail(e, "j-side list");
    if (p.precision != NBODY_PREC_F64 &&
        (e = hipMalloc(&c->sym_posg, (size_t)c->sym_pad * 16)) != hipSuccess) return bail(e, "hipMalloc scaled positions");
    if (pol.dup_tables >= 1 && (e = zalloc(&c->sym_dup_table, table_bytes)) != hipSuccess) return bail(e, zalloc_op, "duplicate detector");
    if (pol.dup_tables == 2 && (e = zalloc(&c->sym_dup_table2, table_bytes)) != hipSuccess) return bail(e, zalloc_op, "duplicate detector");
    if (pol.equal_mass_word && (e = zalloc(&c->sym_general, 64)) != hipSuccess) return bail(e, zalloc_op, "equal-mass flag");
    if ((e = hipMalloc(&c->sym_send, (size_t)p.n_total * c->elem)) != hipSuccess) return bail(e, "hipMalloc send row");
    c->own_send = true;
    if (pol.recv_is_send) {
      c->sym_recv = c->sym_send;
    } else {
      if ((e = hipMalloc(&c->sym_recv, (size_t)c->sym_nsrc * p.i_count * c->elem)) != hipSuccess) return bail(e, "hipMalloc recv rows");
      c->own_recv = true;
    }
  } else {
    if ((e = hipMalloc(&c->accp, (size_t)c->j_split * p.i_count * c->elem)) != hipSuccess) return bail(e, "hipMalloc accp");
    // (the packed one-sided kernel's detector table is not cleared here: its launcher clears it before every pass)
    if (pol.dup_tables >= 1 && (e = hipMalloc(&c->sym_dup_table, table_bytes)) != hipSuccess) return bail(e, "hipMalloc duplicate detector");
    if (pol.equal_mass_word && (e = zalloc(&c->sym_general, 64)) != hipSuccess) return bail(e, zalloc_op, "equal-mass flag");
  }
  if ((e = zalloc(&c->scratch, 64)) != hipSuccess) return bail(e, zalloc_op, "scratch");
  if (p.time_kernels) {
    // NBODY_SYM_ITEM_CLOCKS=1 (tools/even_items.py): room for every work item's own two stamps, word 2 says so
    c->clk_items = (c->sym && env_int("NBODY_SYM_ITEM_CLOCKS", 0) == 1) ? c->sym_items_n : 0;
    const size_t clk_bytes = 64 + 16 * (size_t)c->clk_items;
    if ((e = zalloc((void **)&c->clk, clk_bytes)) != hipSuccess) return bail(e, zalloc_op, "clock words");
    if (c->clk_items) { const unsigned long long one = 1; if ((e = hipMemcpy(c->clk + 2, &one, 8, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy clock words"); }
    (void)hipDeviceGetAttribute(&c->wall_khz, hipDeviceAttributeWallClockRate, p.device);
    c->cus = dev.cus;
  }
  if ((e = hipHostMalloc(&c->h_scratch, 64, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc");
  // the hipMemset calls above run on the null stream and return early; the context's own stream is non-blocking and would not
  // wait for them (bh_frame.hip, bh_create)
  if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return bail(e, "hipStreamSynchronize after the creation memsets");
  g_create_error.clear();   // e.g. the reason AUTO passed over the symmetric plan: not an error of this call
  *out = c;
  return NBODY_OK;
} catch (const std::bad_alloc &) {
  return fail(nullptr, NBODY_ERR_NOMEM, "nbody_create: out of host memory");
}

int nbody_create_multi(const nbody_params *pin, const int32_t *devices, int32_t n_dev, nbody_ctx **out) try {
  if (!pin || !devices || !out) return fail(nullptr, NBODY_ERR_INVALID, "nbody_create_multi: null argument");
  *out = nullptr;
  nbody_ctx *c = new (std::nothrow) nbody_ctx();
  if (!c) return fail(nullptr, NBODY_ERR_NOMEM, "nbody_create_multi: out of host memory");
  std::string why;
  const int rc = nbody::multi_create(pin, devices, n_dev, &c->multi, &why);
  if (rc) { delete c; return fail(nullptr, rc, "%s", why.c_str()); }
  c->p = *pin;
  c->p.i_begin = 0; c->p.i_count = pin->n_total; c->p.device = devices[0];
  c->theta = pin->theta;
  c->elem = (pin->precision == NBODY_PREC_F64) ? 32 : 16;
  *out = c;
  return NBODY_OK;
} catch (const std::bad_alloc &) {
  return fail(nullptr, NBODY_ERR_NOMEM, "nbody_create_multi: out of host memory");
}

void nbody_destroy(nbody_ctx *c) {
  if (c && c->multi) { nbody::multi_destroy(c->multi); delete c; return; }
  if (!c) return;
  (void)hipSetDevice(c->p.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (nbody::KernelTimer &t : c->timers) {
    for (EventPair &e : t.pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (EventPair &e : t.pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  }
  if (c->own_posm && c->posm) (void)hipFree(c->posm);
  if (c->posm_alt) (void)hipFree(c->posm_alt);
  if (c->own_vel && c->vel) (void)hipFree(c->vel);
  if (c->own_acc && c->acc) (void)hipFree(c->acc);
  if (c->accp) (void)hipFree(c->accp);
  for (void *q : {c->sym_pool, c->sym_items, c->sym_iptr, c->sym_ioff, c->sym_jptr, c->sym_joff, c->sym_posg})
    if (q) (void)hipFree(q);
  delete c->plan;
  if (c->own_send && c->sym_send) (void)hipFree(c->sym_send);
  if (c->own_recv && c->sym_recv) (void)hipFree(c->sym_recv);
  if (c->sym_dup_table) (void)hipFree(c->sym_dup_table);
  if (c->sym_dup_table2) (void)hipFree(c->sym_dup_table2);
  if (c->sym_general) (void)hipFree(c->sym_general);
  if (c->bh) nbody::bh_destroy(c->bh);
  if (c->bh_acc) (void)hipFree(c->bh_acc);
  if (c->d_stage) (void)hipFree(c->d_stage);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  for (void *q : {c->tr_pos, c->tr_vel, c->tr_acc, c->probe_part, c->probe_dev, c->pot64, c->tidal64, c->jerk64, c->snap64, c->tr64})
    if (q) (void)hipFree(q);
  for (int o = 0; o < 2; ++o)
    for (void *q : {c->hm[o].buf, c->trh[o].buf, c->hb[o].buf, c->hb[o].tbuf})
      if (q) (void)hipFree(q);
  if (c->probe_host) (void)hipHostFree(c->probe_host);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->clk) (void)hipFree(c->clk);
  if (c->energy_part) (void)hipFree(c->energy_part);
  if (c->moments_part) (void)hipFree(c->moments_part);
  if (c->moments_host) (void)hipHostFree(c->moments_host);
  if (c->h_scratch) (void)hipHostFree(c->h_scratch);
  for (const auto &r : c->pinned) (void)hipHostUnregister(r.first);   // the memory itself stays the caller's
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int nbody_set_stream(nbody_ctx *c, void *hip_stream) {
  if (c && c->multi) return multi_unsupported(c, "nbody_set_stream");
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return NBODY_OK;
}

int nbody_device_ptr(nbody_ctx *c, int32_t which, void **ptr, size_t *bytes) {
  if (c && c->multi) return multi_unsupported(c, "nbody_device_ptr");
  if (!c || !ptr) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  c->hm_external = true;                                          // whichever buffer: the caller may write the state from now on
  nbody::hermite_invalidate(c);
  switch (which) {
    case NBODY_BUF_POSM:
      *ptr = c->posm; if (bytes) *bytes = (size_t)c->p.n_total * c->elem;
      if (int rc = posm_escapes(c)) return rc;                    // the caller may write positions from now on
      break;
    case NBODY_BUF_VEL:  *ptr = c->vel;  if (bytes) *bytes = (size_t)c->p.i_count * c->elem; break;
    case NBODY_BUF_ACC:  *ptr = c->acc;  if (bytes) *bytes = (size_t)c->p.i_count * c->elem; break;
    default: return fail(c, NBODY_ERR_INVALID, "nbody_device_ptr: unknown buffer %d", which);
  }
  return NBODY_OK;
}

int nbody_bind_device_state(nbody_ctx *c, void *posm, void *vel, void *acc) {
  if (c && c->multi) return multi_unsupported(c, "nbody_bind_device_state");
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->hm_external = true;
  nbody::hermite_invalidate(c);
  if (posm) {
    if (int rc = posm_escapes(c)) return rc;
    if (c->own_posm) (void)hipFree(c->posm);
    c->posm = posm; c->own_posm = false;
    c->masses_equal = -1;                       // masses nobody here has seen
    if (c->sym_general)                         // ... every pass's preparation kernel looks
      HIP_TRY(c, hipMemsetAsync(c->sym_general, 0, 4, c->stream));
  }
  if (vel)  { if (c->own_vel) (void)hipFree(c->vel);   c->vel = vel;   c->own_vel = false; }
  if (acc)  { if (c->own_acc) (void)hipFree(c->acc);   c->acc = acc;   c->own_acc = false; }
  // the caller vouches that bound buffers hold a valid state
  if (posm && vel) c->have_state = true;
  c->floor_eps2 = -1.0;
  return NBODY_OK;
}

int nbody_synchronize(nbody_ctx *c) {
  if (c && c->multi) return multi_rc(c, nbody::multi_synchronize(c->multi));
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

int nbody_set_state_soa(nbody_ctx *c, const float *posm4, const float *vel4, int32_t n) {
  return set_state_soa<float>(c, posm4, vel4, n, "nbody_set_state_soa");
}

int nbody_set_state_soa_f64(nbody_ctx *c, const double *posm4, const double *vel4, int32_t n) {
  return set_state_soa<double>(c, posm4, vel4, n, "nbody_set_state_soa_f64");
}

}  // extern "C"

namespace {
int set_particles(nbody_ctx *c, const void *aos, size_t stride, int32_t n, bool keep_history, const char *who) {
  if (!c || !aos) return c ? fail(c, NBODY_ERR_INVALID, "%s: null buffer", who) : NBODY_ERR_INVALID;
  if (n != c->p.n_total) return fail(c, NBODY_ERR_INVALID, "%s: n = %d but the context holds %d bodies", who, n, c->p.n_total);
  if (stride < sizeof(nbody_particle)) return fail(c, NBODY_ERR_INVALID, "%s: stride %zu < %zu", who, stride, sizeof(nbody_particle));
  if (keep_history && !c->have_state) return fail(c, NBODY_ERR_STATE, "%s: no state has been set yet (nbody_set_particles first)", who);
  if (c->multi) {
    const int rc = multi_rc(c, nbody::multi_set_particles(c->multi, aos, stride, n, keep_history));
    if (!rc) { c->have_state = true; if (!keep_history) c->steps_done = 0; }
    return rc;
  }
  std::vector<float> posm((size_t)n * 4), vel((size_t)n * 4);
  const char *base = (const char *)aos;
  for (int i = 0; i < n; ++i) {
    nbody_particle q;
    memcpy(&q, base + (size_t)i * stride, sizeof q);
    posm[4 * (size_t)i + 0] = q.Position[0]; posm[4 * (size_t)i + 1] = q.Position[1];
    posm[4 * (size_t)i + 2] = q.Position[2]; posm[4 * (size_t)i + 3] = q.Mass;
    vel[4 * (size_t)i + 0] = q.Velocity[0]; vel[4 * (size_t)i + 1] = q.Velocity[1];
    vel[4 * (size_t)i + 2] = q.Velocity[2]; vel[4 * (size_t)i + 3] = 0.f;
  }
  int rc = upload_soa<float>(c, posm.data(), vel.data(), keep_history);
  if (rc) return rc;
  // carry the records' Acceleration field over too (the reference keeps whatever was there until the next force pass)
  std::vector<float> acc((size_t)c->p.i_count * 4);
  for (int i = 0; i < c->p.i_count; ++i) {
    nbody_particle q;
    memcpy(&q, base + (size_t)(c->p.i_begin + i) * stride, sizeof q);
    acc[4 * (size_t)i + 0] = q.Acceleration[0]; acc[4 * (size_t)i + 1] = q.Acceleration[1];
    acc[4 * (size_t)i + 2] = q.Acceleration[2]; acc[4 * (size_t)i + 3] = 0.f;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));                     // (upload_soa's clearing of c->acc runs on the stream)
  if (c->p.precision == NBODY_PREC_F64) {
    std::vector<double> a64(acc.begin(), acc.end());
    HIP_TRY(c, hipMemcpy(c->acc, a64.data(), a64.size() * 8, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(c, hipMemcpy(c->acc, acc.data(), acc.size() * 4, hipMemcpyHostToDevice));
  }
  return NBODY_OK;
}
}  // namespace

extern "C" {

int nbody_set_particles(nbody_ctx *c, const void *aos, size_t stride, int32_t n) try {
  return set_particles(c, aos, stride, n, false, "nbody_set_particles");
} catch (const std::bad_alloc &) {
  return fail(c, NBODY_ERR_NOMEM, "nbody_set_particles: out of host memory");
}

int nbody_push_particles(nbody_ctx *c, const void *aos, size_t stride, int32_t n) try {
  return set_particles(c, aos, stride, n, true, "nbody_push_particles");
} catch (const std::bad_alloc &) {
  return fail(c, NBODY_ERR_NOMEM, "nbody_push_particles: out of host memory");
}

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

int nbody_get_positions(nbody_ctx *c, float *xyz, size_t stride, int32_t first, int32_t count) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!xyz || stride < 12) return fail(c, NBODY_ERR_INVALID, "nbody_get_positions: null buffer or stride < 12");
  if (first < 0 || count < 0 || first + count > c->p.n_total) return fail(c, NBODY_ERR_INVALID, "nbody_get_positions: range out of bounds");
  if (count == 0) return NBODY_OK;
  if (c->multi) return multi_rc(c, nbody::multi_get_positions(c->multi, xyz, stride, first, count));
  // one repack kernel + one pinned D2H copy (OctreeSearch.cpp:41 reads Position of every body each frame)
  const size_t bytes = (size_t)count * 12;
  if ((rc = ensure_stage(c, bytes))) return rc;
  HIP_TRY(c, nbody::launch_pack_positions(c->p.precision, c->posm, (float *)c->d_stage, first, count, c->stream));
  const bool direct = stride == 12 && in_pinned(c, xyz, bytes);     // caller's pinned buffer: DMA straight into it
  HIP_TRY(c, hipMemcpyAsync(direct ? (void *)xyz : c->h_stage, c->d_stage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!direct) scatter_records(xyz, stride, c->h_stage, 12, (size_t)count);
  return NBODY_OK;
}

int nbody_get_state_soa(nbody_ctx *c, float *posm4, float *vel4, float *acc4) {
  return get_state_soa<float>(c, posm4, vel4, acc4, "nbody_get_state_soa");
}

int nbody_get_state_soa_f64(nbody_ctx *c, double *posm4, double *vel4, double *acc4) {
  return get_state_soa<double>(c, posm4, vel4, acc4, "nbody_get_state_soa_f64");
}

int nbody_get_particles(nbody_ctx *c, void *aos, size_t stride) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!aos || stride < sizeof(nbody_particle)) return fail(c, NBODY_ERR_INVALID, "nbody_get_particles: null buffer or stride < 40");
  if (c->multi) return multi_rc(c, nbody::multi_get_particles(c->multi, aos, stride));
  bool direct = false;
  if ((rc = queue_particle_mirror(c, aos, stride, &direct))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!direct) scatter_records(aos, stride, c->h_stage, sizeof(nbody_particle), (size_t)c->p.i_count);
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

int nbody_pin_host_buffer(nbody_ctx *c, void *host, size_t bytes) {
  if (!c) return NBODY_ERR_INVALID;
  if (!host || bytes == 0) return fail(c, NBODY_ERR_INVALID, "nbody_pin_host_buffer: null buffer or zero size");
  if (c->multi) return NBODY_OK;   // an optimisation only: a multi-device context delivers through each device's staging buffer
  for (const auto &r : c->pinned)
    if ((char *)host < r.first + r.second && r.first < (char *)host + bytes)
      return fail(c, NBODY_ERR_INVALID, "nbody_pin_host_buffer: overlaps a range that is already pinned");
  HIP_TRY(c, hipSetDevice(c->p.device));
  HIP_TRY(c, hipHostRegister(host, bytes, hipHostRegisterDefault));
  c->pinned.emplace_back((char *)host, bytes);
  return NBODY_OK;
}

int nbody_unpin_host_buffer(nbody_ctx *c, void *host) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return NBODY_OK;
  for (size_t k = 0; k < c->pinned.size(); ++k)
    if (c->pinned[k].first == (char *)host) {
      if (int rc = use_device(c)) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      c->pinned.erase(c->pinned.begin() + (long)k);
      HIP_TRY(c, hipHostUnregister(host));
      return NBODY_OK;
    }
  return fail(c, NBODY_ERR_INVALID, "nbody_unpin_host_buffer: not a buffer pinned through this context");
}

// ---- checkpoint / resume (nothing in the reference to mirror: its state is not even a UPROPERTY) ----
namespace {
struct CkptHeader {
  char magic[8];          // "NBDYCKP2"
  uint32_t header_bytes;
  int32_t n_total, i_begin, i_count;
  int32_t elem_bytes;     // 4 (fp32 state) or 8 (fp64 state)
  int32_t has_root;       // Barnes-Hut cross-frame state present: root_com is the next tree's root centre
  int64_t steps_done;
  double G, eps;
  float theta;            // opening angle in force when the file was written (the reference ships 1.0, OctreeSearch.cpp:85)
  float root_com[3];      // previous tree's centre of mass (OctreeSearch.cpp:77-79)
};
}  // namespace

int nbody_save_checkpoint(nbody_ctx *c, const char *path) try {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!path) return fail(c, NBODY_ERR_INVALID, "nbody_save_checkpoint: null path");
  const bool f64 = c->p.precision == NBODY_PREC_F64;
  const size_t eb = f64 ? 8 : 4, n = (size_t)c->p.n_total, ic = (size_t)c->p.i_count;
  std::vector<char> posm(n * 4 * eb), vel(ic * 4 * eb), acc(ic * 4 * eb);
  CkptHeader h;
  memset(&h, 0, sizeof h);
  if (c->multi) {
    // a multi-device context writes the file a single context of the whole system would write
    rc = f64 ? nbody_get_state_soa_f64(c, (double *)posm.data(), (double *)vel.data(), (double *)acc.data())
             : nbody_get_state_soa(c, (float *)posm.data(), (float *)vel.data(), (float *)acc.data());
    if (rc) return rc;
    int has_root = 0;
    if ((rc = multi_rc(c, nbody::multi_bh_root(c->multi, h.root_com, &has_root)))) return rc;
    h.has_root = has_root;
  } else {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(posm.data(), c->posm, posm.size(), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(vel.data(), c->vel, vel.size(), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(acc.data(), c->acc, acc.size(), hipMemcpyDeviceToHost));
    if (c->bh) {                                                   // the next frame's tree is rooted at this frame's CoM
      HIP_TRY(c, nbody::bh_get_root_com(c->bh, h.root_com, c->stream));
      h.has_root = 1;
    }
  }
  memcpy(h.magic, "NBDYCKP2", 8);
  h.header_bytes = (uint32_t)sizeof h;
  h.n_total = c->p.n_total; h.i_begin = c->p.i_begin; h.i_count = c->p.i_count;
  h.elem_bytes = (int32_t)eb; h.steps_done = c->steps_done; h.G = c->p.G; h.eps = c->p.eps; h.theta = c->theta;
  FILE *f = fopen(path, "wb");
  if (!f) return fail(c, NBODY_ERR_INVALID, "nbody_save_checkpoint: cannot open %s for writing", path);
  const bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(posm.data(), 1, posm.size(), f) == posm.size() &&
                  fwrite(vel.data(), 1, vel.size(), f) == vel.size() && fwrite(acc.data(), 1, acc.size(), f) == acc.size();
  if (fclose(f) != 0 || !ok) return fail(c, NBODY_ERR_INVALID, "nbody_save_checkpoint: short write to %s", path);
  return NBODY_OK;
} catch (const std::bad_alloc &) {
  return fail(c, NBODY_ERR_NOMEM, "nbody_save_checkpoint: out of host memory");
}

int nbody_load_checkpoint(nbody_ctx *c, const char *path, int64_t *steps_done) try {
  if (!c || !path) return c ? fail(c, NBODY_ERR_INVALID, "nbody_load_checkpoint: null path") : NBODY_ERR_INVALID;
  if (c->multi) {                                                  // every device reads its slice of the same file
    int64_t n = 0;
    const int rc = multi_rc(c, nbody::multi_load_checkpoint(c->multi, path, &n));
    if (rc) return rc;
    c->have_state = true; c->steps_done = n;
    (void)nbody_get_theta(nbody::multi_part(c->multi, 0), &c->theta);   // the file's opening angle: every device took it over
    if (steps_done) *steps_done = n;
    return NBODY_OK;
  }
  CkptHeader h;
  const bool f64 = c->p.precision == NBODY_PREC_F64;
  const size_t eb = f64 ? 8 : 4, n = (size_t)c->p.n_total, ic = (size_t)c->p.i_count;
  int rc = NBODY_OK;
  std::vector<char> posm(n * 4 * eb), vel(ic * 4 * eb), acc(ic * 4 * eb);
  FILE *f = fopen(path, "rb");
  if (!f) return fail(c, NBODY_ERR_INVALID, "nbody_load_checkpoint: cannot open %s", path);
  // format 1 (no Barnes-Hut state: the header ends after eps) still loads, as a theta = 0 file without a tree root
  constexpr size_t v1_bytes = offsetof(CkptHeader, theta);
  memset(&h, 0, sizeof h);
  bool head_ok = fread(&h, v1_bytes, 1, f) == 1;
  if (head_ok && memcmp(h.magic, "NBDYCKP2", 8) == 0)
    head_ok = h.header_bytes == sizeof h && fread((char *)&h + v1_bytes, sizeof h - v1_bytes, 1, f) == 1;
  else if (head_ok && memcmp(h.magic, "NBDYCKP1", 8) == 0) {
    head_ok = h.header_bytes == v1_bytes;
    h.has_root = 0; h.theta = 0.0f;
  } else head_ok = false;
  if (!head_ok)
    rc = fail(c, NBODY_ERR_INVALID, "nbody_load_checkpoint: %s is not a checkpoint of this engine (formats NBDYCKP1/2)", path);
  // the file's owned range must contain the context's: a whole-system file also feeds the slices of a sharded job
  else if (h.n_total != c->p.n_total || h.elem_bytes != (int32_t)eb || h.i_begin > c->p.i_begin ||
           h.i_begin + h.i_count < c->p.i_begin + c->p.i_count)
    rc = fail(c, NBODY_ERR_INVALID, "nbody_load_checkpoint: layout mismatch (file n=%d [%d,+%d) %d-byte, context n=%d [%d,+%d) %zu-byte)",
              h.n_total, h.i_begin, h.i_count, h.elem_bytes, c->p.n_total, c->p.i_begin, c->p.i_count, eb);
  else if (h.G != c->p.G || h.eps != c->p.eps)
    rc = fail(c, NBODY_ERR_INVALID, "nbody_load_checkpoint: the file was written with G = %.17g, eps = %.17g but the context has G = %.17g, "
              "eps = %.17g: resuming would not continue the same trajectory", h.G, h.eps, c->p.G, c->p.eps);
  else {
    const long skip = (long)((size_t)(c->p.i_begin - h.i_begin) * 4 * eb), rest = (long)(((size_t)h.i_count - ic) * 4 * eb) - skip;
    if (fread(posm.data(), 1, posm.size(), f) != posm.size() || fseek(f, skip, SEEK_CUR) != 0 ||
        fread(vel.data(), 1, vel.size(), f) != vel.size() || fseek(f, rest + skip, SEEK_CUR) != 0 ||
        fread(acc.data(), 1, acc.size(), f) != acc.size())
      rc = fail(c, NBODY_ERR_INVALID, "nbody_load_checkpoint: %s is truncated", path);
  }
  fclose(f);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->p.device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(c->posm, posm.data(), posm.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->vel, vel.data(), vel.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->acc, acc.data(), acc.size(), hipMemcpyHostToDevice));
  { const int rc2 = f64 ? note_masses(c, (const double *)posm.data()) : note_masses(c, (const float *)posm.data()); if (rc2) return rc2; }
  c->have_state = true; c->floor_eps2 = -1.0; c->step_open = false; c->step_local = false; c->sym_posg_valid = false;
  nbody::hermite_invalidate(c);                                    // (the file holds no derivatives: a resumed run starts from the corrected state)
  if (c->bh) nbody::bh_positions_changed(c->bh);
  c->steps_done = h.steps_done;
  // Barnes-Hut: the opening angle and the root of the next tree (the previous tree's CoM, OctreeSearch.cpp:77-79) are
  // part of the trajectory.  Only contexts that can run the walk take them over (a slice of a sharded job as well: it builds
  // the whole tree).
  if (c->p.precision == NBODY_PREC_F32) {
    c->theta = h.theta;
    if (h.has_root || c->bh) {
      { const int rc2 = nbody::ensure_bh(c); if (rc2) return rc2; }
      const float zero[3] = {0.f, 0.f, 0.f};
      HIP_TRY(c, nbody::bh_set_root_com(c->bh, h.has_root ? h.root_com : zero, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
  }
  if (steps_done) *steps_done = h.steps_done;
  return NBODY_OK;
} catch (const std::bad_alloc &) {
  return fail(c, NBODY_ERR_NOMEM, "nbody_load_checkpoint: out of host memory");
}

int nbody_set_theta(nbody_ctx *c, float theta) {
  if (!c) return NBODY_ERR_INVALID;
  if (!(theta >= 0.0f)) return fail(c, NBODY_ERR_INVALID, "nbody_set_theta: theta must be >= 0");
  if (c->multi) {
    const int rc = multi_rc(c, nbody::multi_set_theta(c->multi, theta));
    if (!rc) c->theta = theta;
    return rc;
  }
  if (theta > 0.0f && c->p.precision != NBODY_PREC_F32)
    return fail(c, NBODY_ERR_UNSUPPORTED, "nbody_set_theta: Barnes-Hut needs an fp32 context");
  if (theta != c->theta) c->sym_posg_valid = false;   // the other force pass moves bodies without preparing the next all-pairs pass
  if (theta != c->theta && c->bh) nbody::bh_positions_changed(c->bh);   // ... nor leaving the next Barnes-Hut frame's Size
  if (theta != c->theta) c->bh_tree_valid = false;    // the last tree's thresholds are the old angle's (nbody_field_at)
  c->theta = theta;
  return NBODY_OK;
}

int nbody_set_bh_max_depth(nbody_ctx *c, int32_t levels) {
  if (!c) return NBODY_ERR_INVALID;
  if (levels < 42 || levels > 200) return fail(c, NBODY_ERR_INVALID, "nbody_set_bh_max_depth: levels must be in [42, 200]");
  if (c->multi) {
    const int rc = multi_rc(c, nbody::multi_set_bh_max_depth(c->multi, levels));
    if (!rc) c->bh_max_depth = levels;
    return rc;
  }
  if (c->p.precision != NBODY_PREC_F32)
    return fail(c, NBODY_ERR_UNSUPPORTED, "nbody_set_bh_max_depth: Barnes-Hut needs an fp32 context");
  if (levels > 42 && c->tr_n > 0)
    return fail(c, NBODY_ERR_UNSUPPORTED, "nbody_set_bh_max_depth: trees deeper than 42 levels do not carry tracers (remove them with "
                "nbody_set_tracers(ctx, NULL, NULL, 0) first)");
  if (int rc = use_device(c)) return rc;
  if (c->bh) {
    const hipError_t e = nbody::bh_set_max_depth(c->bh, levels);
    if (e != hipSuccess) return fail(c, NBODY_ERR_HIP, "nbody_set_bh_max_depth: %s", hipGetErrorString(e));
  }
  c->bh_max_depth = levels;    // (a context without a tree yet takes it when its first theta > 0 frame creates one: bh_driver.hip ensure_bh)
  return NBODY_OK;
}

int nbody_get_bh_max_depth(nbody_ctx *c, int32_t *levels) {
  if (!c || !levels) return NBODY_ERR_INVALID;
  *levels = c->bh_max_depth;
  return NBODY_OK;
}

int nbody_get_theta(nbody_ctx *c, float *theta) {
  if (!c || !theta) return NBODY_ERR_INVALID;
  *theta = c->theta;
  return NBODY_OK;
}

int nbody_bh_stats(nbody_ctx *c, int32_t *nodes, int32_t *levels, float root_com[3]) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return multi_rc(c, nbody::multi_bh_stats(c->multi, nodes, levels, root_com));   // every device holds the whole tree
  if (!c->bh) return fail(c, NBODY_ERR_STATE, "nbody_bh_stats: no tree has been built on this context");
  if (int rc = use_device(c)) return rc;
  int n = 0, l = 0;
  HIP_TRY(c, nbody::bh_stats(c->bh, c->stream, &n, &l));
  if (nodes) *nodes = n;
  if (levels) *levels = l;
  if (root_com) HIP_TRY(c, nbody::bh_get_tree_com(c->bh, root_com, c->stream));
  return NBODY_OK;
}

int nbody_bh_leaf_boxes(nbody_ctx *c, float *boxes, size_t stride) {
  if (!c || !boxes || stride < 16) return c ? fail(c, NBODY_ERR_INVALID, "nbody_bh_leaf_boxes: null buffer or stride < 16") : NBODY_ERR_INVALID;
  if (c->multi) return multi_rc(c, nbody::multi_bh_leaf_boxes(c->multi, boxes, stride));
  if (!c->bh) return fail(c, NBODY_ERR_STATE, "nbody_bh_leaf_boxes: no tree has been built on this context (theta == 0?)");
  if (int rc0 = use_device(c)) return rc0;
  const size_t bytes = (size_t)c->p.n_total * 16;
  int rc = ensure_stage(c, bytes);
  if (rc) return rc;
  HIP_TRY(c, nbody::bh_leaf_boxes(c->bh, c->d_stage, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->d_stage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  scatter_records(boxes, stride, c->h_stage, 16, (size_t)c->p.n_total);
  return NBODY_OK;
}

int nbody_bh_leaf_order(nbody_ctx *c, int32_t *order) {
  if (!c || !order) return c ? fail(c, NBODY_ERR_INVALID, "nbody_bh_leaf_order: null buffer") : NBODY_ERR_INVALID;
  if (c->multi) return multi_rc(c, nbody::multi_bh_leaf_order(c->multi, order));
  if (!c->bh) return fail(c, NBODY_ERR_STATE, "nbody_bh_leaf_order: no tree has been built on this context (theta == 0?)");
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, nbody::bh_leaf_order(c->bh, order, c->stream));
  return NBODY_OK;
}

}  // extern "C"

// ---- the field at points that are not bodies: queries (nbody_field_at) and engine-stepped tracers ----
namespace {
// where they exist: plain fp32 contexts on one device that own all bodies
int probes_supported(nbody_ctx *c, const char *who) {
  if (c->p.precision != NBODY_PREC_F32)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: plain fp32 contexts only (NBODY_PREC_F32)", who);
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  return NBODY_OK;
}

// the queries' staging: n points as float4 and `out_floats` floats each behind them, on the device and its pinned mirror, grown on demand
// (probe_cap: in units of 32 bytes)
int ensure_probe_staging(nbody_ctx *c, int n_points, size_t out_floats) {
  const size_t n = ((size_t)n_points * (16 + 4 * out_floats) + 31) / 32;
  if (n <= c->probe_cap) return NBODY_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->probe_dev) (void)hipFree(c->probe_dev);
  if (c->probe_host) (void)hipHostFree(c->probe_host);
  c->probe_dev = c->probe_host = nullptr; c->probe_cap = 0;
  HIP_TRY(c, hipMalloc(&c->probe_dev, n * 32));
  HIP_TRY(c, hipHostMalloc(&c->probe_host, n * 32, hipHostMallocDefault));
  c->probe_cap = n;
  return NBODY_OK;
}

// theta > 0: is there a tree a query may walk?  (`what`: "field", "potential", "tidal tensor")
int probe_tree_ready(nbody_ctx *c, const char *who, const char *what) {
  if (!c->bh || !c->bh_tree_valid || c->bh_tree_theta != c->theta)
    return fail(c, NBODY_ERR_STATE, "%s: theta > 0 walks the last tree built, and there is none for this opening angle "
                "(none built yet, the last frame refused, or theta changed since): call nbody_compute_forces, nbody_step or nbody_tick first", who);
  if (nbody::bh_last_deep(c->bh))
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: the last tree was built deeper than 42 levels (nbody_set_bh_max_depth); "
                "such trees answer no %s queries", who, what);
  return NBODY_OK;
}

// theta == 0: the potential of the bodies at their CURRENT positions at m points, queued (G and eps the context's; eps == 0: the exact
// d == 0 rule whatever its zero_mode is).  probe == nullptr: at the bodies themselves (m == n_total).
int queue_pot(nbody_ctx *c, const void *probe, int m, double *phi64, float *phif) {
  nbody::PotLaunch L;
  L.posm = c->posm; L.probe = probe; L.part = c->probe_part; L.phi64 = phi64; L.phif = phif;
  L.n_total = c->p.n_total; L.m = m; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps; L.clk = c->clk;
  HIP_TRY(c, nbody::launch_pot(L, c->stream));
  return NBODY_OK;
}

// The bodies' potentials at their CURRENT positions, queued on the stream as one pass under NBODY_KERNEL_FORCES: phi64 ([n_total] double,
// device) and / or phif ([n_total] float, device).  theta > 0: first exactly what nbody_compute_forces runs (the tree of the current
// positions, the stored accelerations, the tracers'), then the walk of that tree from every body.
int queue_body_potentials(nbody_ctx *c, const char *who, double *phi64, float *phif) {
  int rc;
  const int n = c->p.n_total;
  if (c->theta > 0.0f) {
    if ((rc = run_forces(c, true, 0, 0.0f))) return rc;            // (a refused frame: its error, no potentials)
    if ((rc = run_update(c, 0.0f))) return rc;
    if ((rc = probe_tree_ready(c, who, "potential"))) return rc;
    return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
      HIP_TRY(c, nbody::bh_pot_walk(c->bh, c->posm, nullptr, phi64, phif, n, c->p.G, (float)(c->p.eps * c->p.eps), c->stream));
      return NBODY_OK;
    });
  }
  if ((rc = ensure_probe_part(c, n))) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return queue_pot(c, nullptr, n, phi64, phif); });
}

// theta == 0: the tidal tensor of the bodies at their CURRENT positions at m points, queued (G and eps the context's; eps == 0: the
// potential's d == 0 rule, whatever the zero_mode).  probe == nullptr: at the bodies themselves (m == n_total).
int queue_tidal(nbody_ctx *c, const void *probe, int m, double *t64, float *tf) {
  nbody::TidalLaunch L;
  L.posm = c->posm; L.probe = probe; L.part = c->probe_part; L.t64 = t64; L.tf = tf;
  L.n_total = c->p.n_total; L.m = m; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps; L.clk = c->clk;
  HIP_TRY(c, nbody::launch_tidal(L, c->stream));
  return NBODY_OK;
}

// The bodies' tidal tensors at their CURRENT positions, queued as one pass under NBODY_KERNEL_FORCES: t64 ([n_total][6] double, device)
// and / or tf ([n_total][6] float, device).  theta > 0: first exactly what nbody_compute_forces runs, as queue_body_potentials.
int queue_body_tidal(nbody_ctx *c, const char *who, double *t64, float *tf) {
  int rc;
  const int n = c->p.n_total;
  if (c->theta > 0.0f) {
    if ((rc = run_forces(c, true, 0, 0.0f))) return rc;            // (a refused frame: its error, no tensors)
    if ((rc = run_update(c, 0.0f))) return rc;
    if ((rc = probe_tree_ready(c, who, "tidal tensor"))) return rc;
    return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int {
      HIP_TRY(c, nbody::bh_tidal_walk(c->bh, c->posm, nullptr, t64, tf, n, c->p.G, (float)(c->p.eps * c->p.eps), c->stream));
      return NBODY_OK;
    });
  }
  if ((rc = ensure_probe_part(c, n, 2))) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return queue_tidal(c, nullptr, n, t64, tf); });
}

// One query at points that are not bodies: n points from (xyz, stride) in, `width` floats each out to (out, out_stride) — the
// arguments' checks (`bad_args`: the message of a bad one), the tree or the partial rows the launch needs, the points as float4
// through the pinned staging, launch(d_pts, d_out) timed as a pass under NBODY_KERNEL_FORCES, the values back (d_out: a float4 per
// point for width 3, `width` floats otherwise).  floor: the query follows the context's NBODY_ZERO_FLOOR.  part_width: the float4 of a
// point in a chunk's partial row (theta == 0).
// `pair` (the jerk): a second input array — 3 floats per point, staged as float4 behind the points (d_pts + 4 n); NULL: zeros — and a
// second output of `width` floats behind the first in the point's device record (2 * width floats, packed); either output may be NULL,
// not both.  Such a query is a pair sum at every theta (no tree is asked for) and is served where jerk_supported says.
struct PointPair { const float *in; size_t in_stride; float *out; size_t out_stride; };
int jerk_supported(nbody_ctx *c, const char *who, bool points);
template <class Launch>
int query_points(nbody_ctx *c, const char *who, const char *what, const char *bad_args, bool floor, const float *xyz, size_t stride,
                 int32_t n, float *out, size_t out_stride, int width, int part_width, Launch launch, const PointPair *pair = nullptr) {
  if (c && c->multi) return multi_unsupported(c, who);
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = pair ? jerk_supported(c, who, true) : probes_supported(c, who))) return rc;
  const size_t out_min = 4 * (size_t)width;
  bool bad = n < 0 || !xyz || stride < 12;
  if (pair) bad = bad || (pair->in && pair->in_stride < 12) || (!out && !pair->out) || (out && out_stride < out_min) ||
                  (pair->out && pair->out_stride < out_min);
  else      bad = bad || !out || out_stride < out_min;
  if (bad) return fail(c, NBODY_ERR_INVALID, "%s: %s", who, bad_args);
  if (n == 0) return NBODY_OK;
  if (c->theta > 0.0f && !pair) {
    if ((rc = probe_tree_ready(c, who, what))) return rc;
  } else {
    if (floor && (rc = ensure_floor(c))) return rc;
    if ((rc = ensure_probe_part(c, n, part_width))) return rc;
  }
  const size_t out_floats = pair ? 2 * (size_t)width : (width == 3 ? 4 : (size_t)width);
  const size_t in_floats = pair ? 8 : 4;
  if ((rc = ensure_probe_staging(c, n, in_floats - 4 + out_floats))) return rc;
  float *h_pts = (float *)c->probe_host, *h_out = h_pts + in_floats * (size_t)n;
  float *d_pts = (float *)c->probe_dev, *d_out = d_pts + in_floats * (size_t)n;
  for (size_t k = 0; k < (size_t)n; ++k) {
    memcpy(h_pts + 4 * k, (const char *)xyz + k * stride, 12);
    h_pts[4 * k + 3] = 0.0f;
  }
  if (pair) {
    float *h_in2 = h_pts + 4 * (size_t)n;
    for (size_t k = 0; k < (size_t)n; ++k) {
      if (pair->in) memcpy(h_in2 + 4 * k, (const char *)pair->in + k * pair->in_stride, 12);
      else          h_in2[4 * k] = h_in2[4 * k + 1] = h_in2[4 * k + 2] = 0.0f;
      h_in2[4 * k + 3] = 0.0f;
    }
  }
  HIP_TRY(c, hipMemcpyAsync(d_pts, h_pts, (size_t)n * in_floats * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return launch(d_pts, d_out); }))) return rc;
  HIP_TRY(c, hipMemcpyAsync(h_out, d_out, (size_t)n * out_floats * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out) scatter_records(out, out_stride, h_out, out_min, (size_t)n, 4 * out_floats);
  if (pair && pair->out) scatter_records(pair->out, pair->out_stride, h_out + width, out_min, (size_t)n, 4 * out_floats);
  return NBODY_OK;
}
}  // namespace

extern "C" {

int nbody_field_at(nbody_ctx *c, const float *xyz, size_t stride, int32_t n, float *acc, size_t acc_stride) {
  return query_points(c, "nbody_field_at", "field", "null buffer, n < 0 or a stride < 12", true, xyz, stride, n, acc, acc_stride, 3,
                      1, [&](float *d_pts, float *d_acc) -> int {
    if (!(c->theta > 0.0f)) return queue_probe(c, d_pts, nullptr, d_acc, n, 0.0f);
    HIP_TRY(c, nbody::bh_probe_walk(c->bh, d_pts, nullptr, d_acc, n, c->p.G, (float)(c->p.eps * c->p.eps), 0.0f, c->stream));
    return NBODY_OK;
  });
}

// (no ensure_floor: the potential's d == 0 rule is the same under every zero_mode)
int nbody_potential_at(nbody_ctx *c, const float *xyz, size_t stride, int32_t n, float *phi, size_t phi_stride) {
  return query_points(c, "nbody_potential_at", "potential", "null buffer, n < 0, a point stride < 12 or a potential stride < 4", false, xyz,
                      stride, n, phi, phi_stride, 1, 1, [&](float *d_pts, float *d_phi) -> int {
    if (!(c->theta > 0.0f)) return queue_pot(c, d_pts, n, nullptr, d_phi);
    HIP_TRY(c, nbody::bh_pot_walk(c->bh, c->posm, d_pts, nullptr, d_phi, n, c->p.G, (float)(c->p.eps * c->p.eps), c->stream));
    return NBODY_OK;
  });
}

int nbody_get_potentials(nbody_ctx *c, float *phi, size_t stride) {
  if (c && c->multi) return multi_unsupported(c, "nbody_get_potentials");
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = probes_supported(c, "nbody_get_potentials"))) return rc;
  if (!phi || stride < 4) return fail(c, NBODY_ERR_INVALID, "nbody_get_potentials: null buffer or stride < 4");
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * 4))) return rc;
  if ((rc = queue_body_potentials(c, "nbody_get_potentials", nullptr, (float *)c->d_stage))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->d_stage, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  scatter_records(phi, stride, c->h_stage, 4, n);
  return NBODY_OK;
}

int nbody_energy_fast(nbody_ctx *c, double *ke, double *pe) {
  if (c && c->multi) return multi_unsupported(c, "nbody_energy_fast");
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = probes_supported(c, "nbody_energy_fast"))) return rc;
  const int n = c->p.n_total;
  if (!c->pot64) HIP_TRY(c, hipMalloc(&c->pot64, ((size_t)n + 2 * (size_t)nbody::energy_fast_slots(n)) * sizeof(double)));
  double *phi64 = (double *)c->pot64, *partials = phi64 + n;
  if ((rc = queue_body_potentials(c, "nbody_energy_fast", phi64, nullptr))) return rc;
  HIP_TRY(c, nbody::launch_energy_fast(c->posm, c->vel, phi64, n, partials, (double *)c->scratch, c->stream));
  return read_energy(c, ke, pe);
}

int nbody_tidal_at(nbody_ctx *c, const float *xyz, size_t stride, int32_t n, float *t, size_t t_stride) {
  return query_points(c, "nbody_tidal_at", "tidal tensor", "null buffer, n < 0, a point stride < 12 or a tensor stride < 24", false, xyz,
                      stride, n, t, t_stride, 6, 2, [&](float *d_pts, float *d_t) -> int {
    if (!(c->theta > 0.0f)) return queue_tidal(c, d_pts, n, nullptr, d_t);
    HIP_TRY(c, nbody::bh_tidal_walk(c->bh, c->posm, d_pts, nullptr, d_t, n, c->p.G, (float)(c->p.eps * c->p.eps), c->stream));
    return NBODY_OK;
  });
}

int nbody_get_tidal(nbody_ctx *c, float *t, size_t stride) {
  if (c && c->multi) return multi_unsupported(c, "nbody_get_tidal");
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = probes_supported(c, "nbody_get_tidal"))) return rc;
  if (!t || stride < 24) return fail(c, NBODY_ERR_INVALID, "nbody_get_tidal: null buffer or stride < 24");
  const size_t n = (size_t)c->p.n_total;
  if ((rc = ensure_stage(c, n * 24))) return rc;
  if ((rc = queue_body_tidal(c, "nbody_get_tidal", nullptr, (float *)c->d_stage))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->d_stage, n * 24, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  scatter_records(t, stride, c->h_stage, 24, n);
  return NBODY_OK;
}

int nbody_tidal_time(nbody_ctx *c, double *t_min, int32_t *body) {
  if (c && c->multi) return multi_unsupported(c, "nbody_tidal_time");
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = probes_supported(c, "nbody_tidal_time"))) return rc;
  if (!t_min && !body) return fail(c, NBODY_ERR_INVALID, "nbody_tidal_time: both outputs are null");
  const int n = c->p.n_total;
  if (!c->tidal64) HIP_TRY(c, hipMalloc(&c->tidal64, (6 * (size_t)n + 2 * (size_t)nbody::energy_fast_slots(n)) * sizeof(double)));
  double *t64 = (double *)c->tidal64, *partials = t64 + 6 * (size_t)n;
  if ((rc = queue_body_tidal(c, "nbody_tidal_time", t64, nullptr))) return rc;
  HIP_TRY(c, nbody::launch_tidal_time(t64, n, partials, (double *)c->scratch, c->stream));
  double n2 = 0.0, at = 0.0;
  if ((rc = read_energy(c, &n2, &at))) return rc;              // (the scratch's two doubles: the largest n2, its body)
  // t = ||T||_F^(-1/2) = n2^(-1/4)
  if (t_min) *t_min = n2 == 0.0 ? HUGE_VAL : (std::isfinite(n2) ? 1.0 / std::sqrt(std::sqrt(n2)) : 0.0);
  if (body) *body = (int32_t)at;
  return NBODY_OK;
}

}  // extern "C"

// ---- the jerk: a pair sum over all bodies at every theta, on every precision (kernels_jerk.hip) ----
namespace {
// where it exists: contexts on one device that own all bodies; at caller-given points (float arrays) those whose state is fp32 as well
int jerk_supported(nbody_ctx *c, const char *who, bool points) {
  if (c->p.i_count != c->p.n_total)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on a context that owns a slice of the bodies (i_count < n_total)", who);
  if (points && c->p.precision == NBODY_PREC_F64)
    return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not on an fp64 context (its points would have to be doubles); nbody_get_jerk_f64 answers at the bodies", who);
  return NBODY_OK;
}

// (a, j) of the bodies' LIVE buffers — c->posm is the current one of the one-launch step's two, c->vel every path's velocities, as
// nbody_get_moments reads them — at m points, queued (the partial rows are the caller's to provide).  probe == nullptr: at the bodies themselves.
// eps == 0: the potential's d == 0 rule, whatever the zero_mode.  No tree is read or built.
int launch_jerk_on(nbody_ctx *c, const void *probe, const void *pvel, int m, double *aj64, float *ajf) {
  nbody::JerkLaunch L;
  L.posm = c->posm; L.vel = c->vel; L.probe = probe; L.pvel = pvel; L.part = c->probe_part; L.aj64 = aj64; L.ajf = ajf;
  L.n_total = c->p.n_total; L.m = m; L.precision = c->p.precision; L.G = c->p.G; L.eps2 = c->p.eps * c->p.eps;
  HIP_TRY(c, nbody::launch_jerk(L, c->stream));
  return NBODY_OK;
}
}  // namespace

// The bodies' own (a, j), as one pass under NBODY_KERNEL_FORCES; the partial rows in the staging area the point queries use: two
// float4 per body and chunk, six doubles on fp64 state.
int nbody::queue_body_jerk(nbody_ctx *c, double *aj64, float *ajf) {
  const int n = c->p.n_total;
  if (int rc = ensure_probe_part(c, n, c->p.precision == NBODY_PREC_F64 ? 3 : 2)) return rc;
  return timed_launch(c, NBODY_KERNEL_FORCES, [&]() -> int { return launch_jerk_on(c, nullptr, nullptr, n, aj64, ajf); });
}

// the bodies' unrounded (a, j), [n_total][6] double, and the reduction's workgroup pairs behind them: allocated at first use
int nbody::ensure_jerk64(nbody_ctx *c) {
  const size_t n = (size_t)c->p.n_total;
  if (!c->jerk64) HIP_TRY(c, hipMalloc(&c->jerk64, (6 * n + 2 * (size_t)nbody::energy_fast_slots((int)n)) * sizeof(double)));
  return NBODY_OK;
}
namespace {

// nbody_get_jerk / nbody_get_jerk_f64: T = float / double
template <typename T>
int get_jerk(nbody_ctx *c, const char *who, T *acc, size_t acc_stride, T *jerk, size_t jerk_stride) {
  if (c && c->multi) return multi_unsupported(c, who);
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = jerk_supported(c, who, false))) return rc;
  if ((!acc && !jerk) || (acc && acc_stride < 3 * sizeof(T)) || (jerk && jerk_stride < 3 * sizeof(T)))
    return fail(c, NBODY_ERR_INVALID, "%s: both outputs are null, or a stride < %d", who, (int)(3 * sizeof(T)));
  const size_t n = (size_t)c->p.n_total, rec = 6 * sizeof(T);
  if ((rc = ensure_stage(c, n * rec))) return rc;
  if constexpr (sizeof(T) == 8) {
    if ((rc = ensure_jerk64(c))) return rc;
    if ((rc = queue_body_jerk(c, (double *)c->jerk64, nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->jerk64, n * rec, hipMemcpyDeviceToHost, c->stream));
  } else {
    if ((rc = queue_body_jerk(c, nullptr, (float *)c->d_stage))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_stage, c->d_stage, n * rec, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (acc) scatter_records(acc, acc_stride, c->h_stage, rec / 2, n, rec);
  if (jerk) scatter_records(jerk, jerk_stride, (const char *)c->h_stage + rec / 2, rec / 2, n, rec);
  return NBODY_OK;
}
}  // namespace

extern "C" {

int nbody_jerk_at(nbody_ctx *c, const float *xyz, size_t stride, const float *vel, size_t vel_stride, int32_t n, float *acc,
                  size_t acc_stride, float *jerk, size_t jerk_stride) {
  const PointPair pair{vel, vel_stride, jerk, jerk_stride};
  return query_points(c, "nbody_jerk_at", "jerk", "null points, n < 0, both outputs null, or a stride < 12", false, xyz, stride, n, acc,
                      acc_stride, 3, 2, [&](float *d_pts, float *d_aj) -> int {
    return launch_jerk_on(c, d_pts, d_pts + 4 * (size_t)n, n, nullptr, d_aj);
  }, &pair);
}

int nbody_get_jerk(nbody_ctx *c, float *acc, size_t acc_stride, float *jerk, size_t jerk_stride) {
  return get_jerk<float>(c, "nbody_get_jerk", acc, acc_stride, jerk, jerk_stride);
}

int nbody_get_jerk_f64(nbody_ctx *c, double *acc, size_t acc_stride, double *jerk, size_t jerk_stride) {
  return get_jerk<double>(c, "nbody_get_jerk_f64", acc, acc_stride, jerk, jerk_stride);
}

int nbody_jerk_time(nbody_ctx *c, double *t_min, int32_t *body) {
  if (c && c->multi) return multi_unsupported(c, "nbody_jerk_time");
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = jerk_supported(c, "nbody_jerk_time", false))) return rc;
  if (!t_min && !body) return fail(c, NBODY_ERR_INVALID, "nbody_jerk_time: both outputs are null");
  const int n = c->p.n_total;
  if ((rc = ensure_jerk64(c))) return rc;
  double *aj64 = (double *)c->jerk64, *partials = aj64 + 6 * (size_t)n;
  if ((rc = queue_body_jerk(c, aj64, nullptr))) return rc;
  HIP_TRY(c, nbody::launch_jerk_time(aj64, n, partials, (double *)c->scratch, c->stream));
  double k = 0.0, at = 0.0;
  if ((rc = read_energy(c, &k, &at))) return rc;               // (the scratch's two doubles: the largest |j|^2 / |a|^2, its body)
  if (t_min) *t_min = k == 0.0 ? HUGE_VAL : (std::isfinite(k) ? 1.0 / std::sqrt(k) : 0.0);
  if (body) *body = (int32_t)at;
  return NBODY_OK;
}

int nbody_set_tracers(nbody_ctx *c, const float *pos4, const float *vel4, int32_t n) {
  if (c && c->multi) return multi_unsupported(c, "nbody_set_tracers");
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = probes_supported(c, "nbody_set_tracers")) return rc;
  if (n < 0 || (n > 0 && !pos4)) return fail(c, NBODY_ERR_INVALID, "nbody_set_tracers: n < 0 or null positions");
  if (n > 0 && c->bh_max_depth > 42)
    return fail(c, NBODY_ERR_UNSUPPORTED, "nbody_set_tracers: this context builds trees deeper than 42 levels (nbody_set_bh_max_depth), "
                "which do not carry tracers");
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (void **q : {&c->tr_pos, &c->tr_vel, &c->tr_acc}) { if (*q) (void)hipFree(*q); *q = nullptr; }
  c->tr_n = 0;
  if (n == 0) return NBODY_OK;
  const size_t bytes = (size_t)n * 16;
  HIP_TRY(c, hipMalloc(&c->tr_pos, bytes));
  HIP_TRY(c, hipMalloc(&c->tr_vel, bytes));
  HIP_TRY(c, hipMalloc(&c->tr_acc, bytes));
  HIP_TRY(c, hipMemcpyAsync(c->tr_pos, pos4, bytes, hipMemcpyHostToDevice, c->stream));
  if (vel4) HIP_TRY(c, hipMemcpyAsync(c->tr_vel, vel4, bytes, hipMemcpyHostToDevice, c->stream));
  else      HIP_TRY(c, hipMemsetAsync(c->tr_vel, 0, bytes, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->tr_acc, 0, bytes, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));                     // the caller's arrays are its own again
  c->tr_n = n;
  return NBODY_OK;
}

int nbody_get_tracers(nbody_ctx *c, float *pos4, float *vel4, float *acc4) {
  if (c && c->multi) return multi_unsupported(c, "nbody_get_tracers");
  if (!c) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t bytes = (size_t)c->tr_n * 16;
  if (bytes == 0) return NBODY_OK;
  if (pos4) HIP_TRY(c, hipMemcpy(pos4, c->tr_pos, bytes, hipMemcpyDeviceToHost));
  if (vel4) HIP_TRY(c, hipMemcpy(vel4, c->tr_vel, bytes, hipMemcpyDeviceToHost));
  if (acc4) HIP_TRY(c, hipMemcpy(acc4, c->tr_acc, bytes, hipMemcpyDeviceToHost));
  return NBODY_OK;
}

int nbody_tracer_count(nbody_ctx *c, int32_t *n) {
  if (c && c->multi) return multi_unsupported(c, "nbody_tracer_count");
  if (!c || !n) return NBODY_ERR_INVALID;
  *n = c->tr_n;
  return NBODY_OK;
}

// Not in include/nbody.h: tuning aid of tools/even_items.py — the reference-clock stamps (start, end) every work item of the
// last symmetric force launch left (contexts created with time_kernels under NBODY_SYM_ITEM_CLOCKS=1), and the clock's rate.
__attribute__((visibility("default"))) int nbody_debug_sym_item_clocks(nbody_ctx *c, unsigned long long *out, int32_t cap, int32_t *n_items,
                                                                       int32_t *khz) {
  if (!c || c->multi || !c->clk || c->clk_items <= 0) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  if (n_items) *n_items = c->clk_items;
  if (khz) *khz = c->wall_khz;
  if (!out) return NBODY_OK;
  if (cap < 2 * c->clk_items) return NBODY_ERR_INVALID;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->clk + 8, 16 * (size_t)c->clk_items, hipMemcpyDeviceToHost));
  return NBODY_OK;
}

// Not in include/nbody.h: tuning aid of tools/bh_phases.py (meaningful in -DNBODY_BH_PHASE_CLOCKS builds only).
__attribute__((visibility("default"))) int nbody_debug_bh_clocks(nbody_ctx *c, long long out[16 + 3 * 512]) {
  if (!c || c->multi || !c->bh || !out) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, nbody::bh_debug_clocks(c->bh, out, c->stream));
  return NBODY_OK;
}

// Not in include/nbody.h either: how many frames of the larger systems were sorted starting from the previous frame's order, and how
// often a frame given up by that sort (a bucket ran over) was queued again with the cold sorts (tests/test_bh_gpu.py).
__attribute__((visibility("default"))) int nbody_debug_bh_sort_counts(nbody_ctx *c, long long *warm_frames, long long *retries) {
  if (!c || c->multi || !c->bh || !warm_frames || !retries) return NBODY_ERR_INVALID;
  nbody::bh_debug_sort_counts(c->bh, warm_frames, retries);
  return NBODY_OK;
}

// Not in include/nbody.h: fault injection for tests/test_bh_gpu.py — the words the creation memsets clear, set to something else between
// two frames (what a fill that ran late, or never, would leave): kind 1 = the warm sort's bucket counts := 3 each.
__attribute__((visibility("default"))) int nbody_debug_bh_poison(nbody_ctx *c, int kind) {
  if (!c || c->multi || !c->bh) return NBODY_ERR_INVALID;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, nbody::bh_debug_poison(c->bh, kind, c->stream));
  return NBODY_OK;
}

int nbody_steps_done(nbody_ctx *c, int64_t *steps) {
  if (!c || !steps) return NBODY_ERR_INVALID;
  *steps = c->steps_done;
  return NBODY_OK;
}

int nbody_kernel_time(nbody_ctx *c, int32_t which, double *total_ms, int64_t *launches) {
  if (!c || which < 0 || which > 1) return NBODY_ERR_INVALID;
  if (c->multi) return multi_rc(c, nbody::multi_kernel_time(c->multi, which, total_ms, launches));
  if (int rc0 = use_device(c)) return rc0;
  int rc = nbody::timer_drain(c, which);
  if (rc) return rc;
  if (total_ms) *total_ms = c->timers[which].total_ms;
  if (launches) *launches = c->timers[which].launches;
  return NBODY_OK;
}

int nbody_kernel_time_reset(nbody_ctx *c) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return multi_rc(c, nbody::multi_kernel_time_reset(c->multi));
  if (int rc0 = use_device(c)) return rc0;
  for (int w = 0; w < 2; ++w) {
    int rc = nbody::timer_drain(c, w);
    if (rc) return rc;
    c->timers[w].total_ms = 0.0;
    c->timers[w].launches = 0;
  }
  if (c->clk) { HIP_TRY(c, hipMemsetAsync(c->clk, 0, 16, c->stream)); HIP_TRY(c, hipStreamSynchronize(c->stream)); }
  return NBODY_OK;
}

int nbody_kernel_clock(nbody_ctx *c, double *shader_mhz, int32_t *compute_units) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return multi_rc(c, nbody::multi_kernel_clock(c->multi, shader_mhz, compute_units));
  if (int rc0 = use_device(c)) return rc0;
  if (shader_mhz) *shader_mhz = 0.0;
  if (compute_units) *compute_units = c->cus;
  if (!c->clk) return fail(c, NBODY_ERR_STATE, "nbody_kernel_clock: the context was created without time_kernels");
  unsigned long long w[2] = {0, 0};
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(w, c->clk, sizeof w, hipMemcpyDeviceToHost));
  if (shader_mhz && w[1] != 0ull) *shader_mhz = (double)w[0] / (double)w[1] * (double)c->wall_khz * 1e-3;
  return NBODY_OK;
}

const char *nbody_force_kernel_name(const nbody_ctx *c) {
  if (!c) return "";
  if (c->multi) return nbody_force_kernel_name(nbody::multi_part(c->multi, 0));
  return nbody::force_kernel_name(c->sym, c->wave, c->ipt, c->p, c->theta);
}

int nbody_get_algorithm(nbody_ctx *c, int32_t *algorithm, int32_t *super_tile) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return nbody_get_algorithm(nbody::multi_part(c->multi, 0), algorithm, super_tile);
  if (algorithm) *algorithm = c->sym ? NBODY_ALGO_SYMMETRIC : NBODY_ALGO_TILED;
  if (super_tile) *super_tile = c->sym ? c->sym_bi : 0;
  return NBODY_OK;
}

int32_t nbody_sym_plan_is_even(const nbody_ctx *c) {
  if (!c) return 0;
  if (c->multi) return nbody_sym_plan_is_even(nbody::multi_part(c->multi, 0));
  return c->sym && c->sym_even ? 1 : 0;
}

int nbody_sym_pool_info(nbody_ctx *c, uint64_t *pool_bytes, int32_t *phases) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return nbody_sym_pool_info(nbody::multi_part(c->multi, 0), pool_bytes, phases);
  if (pool_bytes) *pool_bytes = c->sym ? (uint64_t)c->sym_pool_elems * c->elem : 0;
  if (phases) *phases = c->sym ? (int32_t)c->sym_phase_item0.size() - 1 : 0;
  return NBODY_OK;
}

int nbody_equal_mass_form(nbody_ctx *c, int32_t *in_use) {
  if (!c || !in_use) return NBODY_ERR_INVALID;
  if (c->multi) return nbody_equal_mass_form(nbody::multi_part(c->multi, 0), in_use);
  *in_use = 0;
  if (!c->sym_general || c->theta > 0.0f) return NBODY_OK;
  HIP_TRY(c, hipSetDevice(c->p.device));
  HIP_TRY(c, hipMemcpyAsync(c->h_scratch, c->sym_general, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int32_t word;
  memcpy(&word, c->h_scratch, 4);
  *in_use = word == 0 ? 1 : 0;
  return NBODY_OK;
}

int nbody_get_launch_config(nbody_ctx *c, int32_t *tile, int32_t *i_per_thread, int32_t *j_split, int32_t *blocks,
                            int32_t *threads) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return nbody_get_launch_config(nbody::multi_part(c->multi, 0), tile, i_per_thread, j_split, blocks, threads);   // per device
  int b = 0, t = 0;
  nbody::forces_geometry(make_launch(c), &b, &t);
  if (c->sym) { b = c->sym_items_n; t = 256; }
  if (tile) *tile = c->tile;
  if (i_per_thread) *i_per_thread = c->sym ? c->sym_bi / 256 : c->ipt;
  if (j_split) *j_split = c->j_split;
  if (blocks) *blocks = b;
  if (threads) *threads = t;
  return NBODY_OK;
}

}  // extern "C"
