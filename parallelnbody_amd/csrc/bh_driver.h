// The host-side driver of the theta > 0 (Barnes-Hut) path: frames are queued, waited for once, and what the verdict says was not
// built is queued again.  One per-context pair — bh_queue_frame, bh_collect_frames — and one loop over it, bh_drive, shared by a
// single context's whole frames (nbody_step, nbody_tick), its force-only pass (nbody_compute_forces, nbody_step_begin) and the
// multi-device engine (multi.hip: every device's frames and the all-gathers between them, then one wait).  Not part of the C-ABI.
#pragma once
#include "../../include/nbody.h"
#include "kernels.h"

namespace nbody {

int ensure_bh(nbody_ctx *c);                       // the Barnes-Hut state of a context, on first use

// Queue one frame on the context's stream (its device is the current one); nothing waits.  dt > 0: a whole frame — tree, walk of the
// own slice, kick-drift —, `stage` (optional) takes its FParticle records.  Otherwise a force-only pass: the walk's accelerations
// into bh_acc (bh_queue_update adds them up); diagnostic: it belongs to no frame and leaves the next tree's root centre alone.
// deep: the frame is the one bh_collect_frames handed back (kBhStatusDeep), built with its deep clusters resolved (one wait inside).
int bh_queue_frame(nbody_ctx *c, float dt, bool diagnostic, bool deep, float *stage);
// The one wait.  *built of the frames queued since the last collect were built, and count as steps if they were whole frames.
// *status kBhStatusRetry / kBhStatusDeep: the others did nothing (on this device nor, the build being the same everywhere, on any
// other) and are the caller's to queue again; their event pairs have been taken back.  A refusal (bh_refused) is the return
// value, its text the context's, and the state that of the frames built.
int bh_collect_frames(nbody_ctx *c, int *status, int *built);
// bh_acc -> acc and, with dt > 0, the kick-drift of the own slice: the update behind a force-only pass
int bh_queue_update(nbody_ctx *c, float dt);

// `frames` frames through queue / collect until all are built or one is refused.
//   queue(deep, last)        queue one frame: `deep` the rebuild of a frame handed back, `last` the last one of this round
//   collect(&status, &built) wait and report; a non-zero return ends the call
// queued: the caller has queued the first round itself (nbody_tick queues its frame ahead of its other work).
template <typename Queue, typename Collect>
int bh_drive(int frames, Queue &&queue, Collect &&collect, int *built_total = nullptr, bool queued = false) {
  bool deep_next = false;                          // the first frame of the next round is one a deep context handed back
  for (int left = frames; left > 0; queued = false) {
    for (int f = 0; f < left && !queued; ++f)
      if (int rc = queue(f == 0 && deep_next, f == left - 1)) return rc;
    int status = kBhStatusOk, built = 0;
    const int rc = collect(&status, &built);
    left -= built;
    if (built_total) *built_total += built;
    if (rc) return rc;
    deep_next = status == kBhStatusDeep;
    if (!deep_next && status != kBhStatusRetry) break;
  }
  return NBODY_OK;
}

// the two single-context instantiations: whole frames (stage: the last frame's records), and the force-only pass
int bh_run_frames(nbody_ctx *c, float dt, int frames, float *stage, bool queued = false);
int bh_run_forces(nbody_ctx *c, bool diagnostic);

// the next tree's root centre (the previous tree's CoM, OctreeSearch.cpp:77-79) of a context that has built a tree: what a checkpoint keeps
int part_bh_root(nbody_ctx *c, float out[3], int *has_root);

}  // namespace nbody
