// State in and out of a context (include/nbody.h): uploads and downloads in the three record formats (SoA float, SoA double, FParticle
// records), the frame's FParticle mirror, pinning of caller memory, checkpoints.  Host C++ like capi.hip; what it shares with the other
// host units: capi_common.h.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>

#include "bh_driver.h"
#include "capi_common.h"
#include "ctx.h"

namespace {
using nbody::check_ready; using nbody::ensure_stage; using nbody::fail; using nbody::multi_rc; using nbody::queue_particle_mirror; using nbody::scatter_records; using nbody::use_device;

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

}  // namespace

// The owned bodies' FParticle records, queued: packed on the device, then copied to the caller's pinned mirror (*direct) or to the
// staging buffer (scatter_records delivers from there once the stream has been waited for).
int nbody::queue_particle_mirror(nbody_ctx *c, void *aos, size_t stride, bool *direct) {
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
int nbody::mirror_device_ptr(nbody_ctx *c, void *aos, size_t stride, bool align16, bool *direct, void **dev) {
  if (int rc = ensure_stage(c, (size_t)c->p.i_count * sizeof(nbody_particle))) return rc;
  *direct = mirror_is_direct(c, aos, stride) && (!align16 || ((uintptr_t)aos & 15u) == 0);
  HIP_TRY(c, hipHostGetDevicePointer(dev, *direct ? aos : c->h_stage, 0));
  return NBODY_OK;
}

namespace {
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

// ---- checkpoint / resume (nothing in the reference to mirror: its state is not even a UPROPERTY) ----
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

extern "C" {

int nbody_set_state_soa(nbody_ctx *c, const float *posm4, const float *vel4, int32_t n) {
  return set_state_soa<float>(c, posm4, vel4, n, "nbody_set_state_soa");
}

int nbody_set_state_soa_f64(nbody_ctx *c, const double *posm4, const double *vel4, int32_t n) {
  return set_state_soa<double>(c, posm4, vel4, n, "nbody_set_state_soa_f64");
}

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

}  // extern "C"
