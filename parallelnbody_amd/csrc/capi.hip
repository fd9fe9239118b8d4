// C-ABI of libnbody_amd.so (include/nbody.h): the context's life, its stream and device buffers, the Barnes-Hut settings, the info getters,
// timers and debug calls, and the helpers every host unit calls (capi_common.h).  State in and out: capi_state.hip; the passes, the steps
// and nbody_tick: capi_step.hip; the fp32 queries and tracers: capi_query.hip; the fp64 queries: capi_query64.hip; the Hermite calls:
// capi_hermite.hip.  Host C++ over the HIP runtime; no torch types, no exceptions across the boundary (the entry points that allocate
// host memory catch std::bad_alloc), no CPU fallback.  Which kernel, geometry and plan a context gets — every size threshold — is decided
// in launch_policy.{h,cpp} (host only, CPU-tested); nbody_create asks the device its CU count and memory and carries the answer out.
#include <cstddef>
#include <cstring>
#include <new>

#include "bh_driver.h"
#include "capi_common.h"
#include "ctx.h"
#include "launch_policy.h"

// ---- what the other host units call as well (capi_common.h) ----
namespace nbody {
int multi_unsupported(nbody_ctx *c, const char *who) {
  return fail(c, NBODY_ERR_UNSUPPORTED, "%s: not available on a multi-device context (nbody_create_multi); use one context per device", who);
}

// A call on a multi-device context is answered by its Multi; its message becomes the context's.
int multi_rc(nbody_ctx *c, int rc) {
  if (rc) c->err = nbody::multi_error(c->multi);
  return rc;
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

// (Re)allocate the hand-off staging pair for `bytes`.  Every call that uses the pair waits for its own work before it returns, so nothing
// in flight reads or writes the old one; the wait in front of the frees says so instead of leaving it to hipFree's (growth only).
int ensure_stage(nbody_ctx *c, size_t bytes) {
  if (bytes <= c->stage_bytes) return NBODY_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->d_stage) (void)hipFree(c->d_stage);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  c->d_stage = c->h_stage = nullptr; c->stage_bytes = 0;
  HIP_TRY(c, hipMalloc(&c->d_stage, bytes));
  HIP_TRY(c, hipHostMalloc(&c->h_stage, bytes, hipHostMallocDefault));
  c->stage_bytes = bytes;
  return NBODY_OK;
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

using nbody::detector_table_bytes; using nbody::env_int; using nbody::EventPair; using nbody::fail; using nbody::g_create_error; using nbody::use_device;
using nbody::ensure_stage; using nbody::make_launch; using nbody::multi_rc; using nbody::multi_unsupported; using nbody::posm_escapes; using nbody::scatter_records;

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
  for (void *q : {c->tr_pos, c->tr_vel, c->tr_acc, c->probe_part, c->pot64, c->tidal64, c->jerk64, c->snap64, c->tr64})
    if (q) (void)hipFree(q);
  for (int o = 0; o < 2; ++o)
    for (void *q : {c->hm[o].buf, c->trh[o].buf, c->hb[o].buf, c->hb[o].tbuf})
      if (q) (void)hipFree(q);
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
