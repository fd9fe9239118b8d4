// The per-context half of the Barnes-Hut frame driver (bh_driver.h): what is queued, what the one wait finds, and the books kept in
// between — the event pairs of nbody_kernel_time, the steps done.  Host C++ over bh_frame.hip's launchers.
#include "bh_driver.h"

#include "ctx.h"

namespace nbody {

int ensure_bh(nbody_ctx *c) {
  if (c->p.precision != NBODY_PREC_F32)
    return fail(c, NBODY_ERR_UNSUPPORTED, "theta > 0 (Barnes-Hut) needs an fp32 context");
  if (c->bh) return NBODY_OK;
  // a context that owns a slice builds the whole tree from the replicated positions and walks its own bodies (bh_common.h, WalkSlice)
  hipError_t e = bh_create(&c->bh, c->p.n_total, c->p.i_begin, c->p.i_count);
  if (e == hipSuccess) e = hipMalloc(&c->bh_acc, (size_t)c->p.i_count * 16);
  if (e != hipSuccess) {
    bh_destroy(c->bh); c->bh = nullptr;
    if (c->bh_acc) { (void)hipFree(c->bh_acc); c->bh_acc = nullptr; }
    return fail(c, NBODY_ERR_HIP, "bh_create: %s", hipGetErrorString(e));
  }
  bh_set_div_mode(c->bh, c->p.bh_div_mode);
  if (c->bh_max_depth != 42 && (e = bh_set_max_depth(c->bh, c->bh_max_depth)) != hipSuccess)
    return fail(c, NBODY_ERR_HIP, "bh_set_max_depth: %s", hipGetErrorString(e));
  if (c->posm_escaped) bh_positions_external(c->bh);
  return NBODY_OK;
}

static int bh_status_error(nbody_ctx *c, int status) {
  switch (status) {
    case kBhStatusTooDeep: return fail(c, NBODY_ERR_UNSUPPORTED, "Barnes-Hut tree deeper than %d levels: two bodies closer than Size/2^%d (the reference's Add would recurse without bound on coincident bodies)", c->bh_max_depth, c->bh_max_depth);
    case kBhStatusDeepRun: return fail(c, NBODY_ERR_UNSUPPORTED, "Barnes-Hut: more than 64 bodies share one cell of level 42 (a deep context orders at most 64 bodies below level 42)");
    case kBhStatusNodePool: return fail(c, NBODY_ERR_NOMEM, "Barnes-Hut node pool exhausted");
    case kBhStatusUnsorted: return fail(c, NBODY_ERR_STATE, "Barnes-Hut: the sorted path keys are out of order (an internal error of this library; the frame was not built and the state is what it was)");
    default: return NBODY_OK;
  }
}

// the Plummer softening of every theta > 0 walk: eps * eps in double, rounded once to fp32; 0 — eps == 0, or an eps whose square
// rounds to 0 — walks with the reference's own term
static float bh_eps2(const nbody_ctx *c) { return (float)(c->p.eps * c->p.eps); }

int bh_queue_frame(nbody_ctx *c, float dt, bool diagnostic, bool deep, float *stage) {
  if (int rc = ensure_bh(c)) return rc;
  const bool whole = dt > 0.0f;
  auto launch = [&]() -> int {
    HIP_TRY(c, (deep ? bh_deep_frame : bh_frame)(c->bh, c->posm, whole ? c->vel : nullptr, whole ? c->acc : c->bh_acc, c->theta, c->p.G,
                                                 bh_eps2(c), whole ? dt : 0.0f, diagnostic ? 1 : 0, whole ? stage : nullptr, c->stream));
    // the tracers' walk of this frame's tree, behind the frame's own walk and part of the frame: timed with it, queued again with it,
    // and — looking at the frame's verdict itself — idle behind a frame that did nothing
    // (whole frames and nbody_compute_forces' pass; not the force-only pass of nbody_step_begin, which leaves tracers alone at every angle)
    if (c->tr_n > 0 && (whole || diagnostic))
      HIP_TRY(c, bh_probe_walk(c->bh, c->tr_pos, c->tr_vel, c->tr_acc, c->tr_n, c->p.G, bh_eps2(c), whole ? dt : 0.0f, c->stream));
    return NBODY_OK;
  };
  // (small systems queue a whole call's frames at once and give none up: bound the number of live events; the larger systems'
  // batches of 64 never get here, so the pairs of a given-up batch are still there to be taken back)
  if (int rc = timed_launch(c, NBODY_KERNEL_FORCES, launch, true, whole && bh_is_small(c->bh))) return rc;
  c->bh_batch.queued += 1;
  c->bh_batch.whole = whole;
  if (whole) c->sym_posg_valid = false;   // bodies move without the fused all-pairs update's preparation of the next pass
  return NBODY_OK;
}

// (given up: kernels_bh_sort.hip — a bucket ran over: the records were replaced, the root box jumped; handed back: a deep context's
// frame with bodies below level 42.  bh_drive queues them again, inside event pairs of their own.)
int bh_collect_frames(nbody_ctx *c, int *status, int *built) {
  *status = kBhStatusOk; *built = 0;
  HIP_TRY(c, bh_collect(c->bh, c->stream, status, built));
  if (c->bh_batch.whole) c->steps_done += *built;
  const int undone = c->bh_batch.queued - *built;
  // what nbody_field_at may walk: the arrays hold the tree of the last frame queued, if that frame was built
  if (c->bh_batch.queued > 0) { c->bh_tree_valid = *status == kBhStatusOk && undone == 0; c->bh_tree_theta = c->theta; }
  c->bh_batch.queued = 0;
  if (*status == kBhStatusRetry || *status == kBhStatusDeep) {
    if (c->p.time_kernels) timer_take_back(c, NBODY_KERNEL_FORCES, undone);
    return NBODY_OK;
  }
  if (c->p.time_kernels) { if (int rc = timer_drain_at_cap(c, NBODY_KERNEL_FORCES)) return rc; }   // the batch has gone through
  return bh_status_error(c, *status);
}

int bh_queue_update(nbody_ctx *c, float dt) {
  auto launch = [&]() -> int {
    HIP_TRY(c, launch_update(c->p.precision, c->posm, c->vel, c->acc, c->bh_acc, c->p.i_begin, c->p.i_count, 1, dt, c->stream));
    return NBODY_OK;
  };
  if (int rc = timed_launch(c, NBODY_KERNEL_UPDATE, launch)) return rc;
  // bodies moved without the fused update's preparation of the next all-pairs pass: posg and the detector table are
  // those of older positions (the next theta == 0 pass runs the preparation kernel again)
  if (dt > 0.0f) c->sym_posg_valid = false;
  if (dt > 0.0f && c->bh) bh_positions_changed(c->bh);   // ... and the next Barnes-Hut frame looks at the positions for its Size
  return NBODY_OK;
}

int bh_run_frames(nbody_ctx *c, float dt, int frames, float *stage, bool queued) {
  return bh_drive(frames, [&](bool deep, bool last) { return bh_queue_frame(c, dt, false, deep, last ? stage : nullptr); },
                  [&](int *status, int *built) { return bh_collect_frames(c, status, built); }, nullptr, queued);
}

int bh_run_forces(nbody_ctx *c, bool diagnostic) {
  return bh_drive(1, [&](bool deep, bool) { return bh_queue_frame(c, 0.0f, diagnostic, deep, nullptr); },
                  [&](int *status, int *built) { return bh_collect_frames(c, status, built); });
}

int part_bh_root(nbody_ctx *c, float out[3], int *has_root) {
  *has_root = 0;
  if (!c->bh) return NBODY_OK;
  if (int rc = use_device(c)) return rc;
  HIP_TRY(c, bh_get_root_com(c->bh, out, c->stream));
  *has_root = 1;
  return NBODY_OK;
}

}  // namespace nbody
