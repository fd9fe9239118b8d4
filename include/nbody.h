/*
 * nbody.h — C-ABI of the MI355X-native N-body engine (libnbody_amd.so).
 *
 * The reference (Milias/ParallelNbody) has no FFI; its boundary for this path is the public
 * surface of the UE4 actor AOctreeSearch (Source/NBody/OctreeSearch.h:111-149).  Each entry point
 * below replaces one responsibility of that class and cites it.  Paths are relative to
 * /root/reference/Source/NBody/.
 *
 * Conventions: plain C types only; every call returns 0 (NBODY_OK) or a negative NBODY_ERR_*;
 * nothing throws across the boundary; the context is an opaque caller-owned pointer; all host
 * buffers are caller-allocated; calls on one context are not thread-safe (the reference runs on
 * the UE4 game thread only).  There is NO CPU fallback: without a HIP device nbody_create fails
 * with NBODY_ERR_NO_DEVICE.
 */
#ifndef NBODY_AMD_H
#define NBODY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (Not NBODY_API: UnrealBuildTool defines <MODULE>_API for every module, and the reference's module is called NBody — its actor is
 * declared `class NBODY_API AOctreeSearch`, OctreeSearch.h:112.  A header of this library must not redefine the host's macro.) */
#define NBODY_AMD_API __attribute__((visibility("default")))

#define NBODY_VERSION_MAJOR 0
#define NBODY_VERSION_MINOR 1

typedef struct nbody_ctx nbody_ctx;

enum {
  NBODY_OK = 0,
  NBODY_ERR_INVALID = -1,     /* bad argument */
  NBODY_ERR_NO_DEVICE = -2,   /* no HIP device / device ordinal out of range */
  NBODY_ERR_HIP = -3,         /* a HIP runtime call failed; see nbody_last_error */
  NBODY_ERR_STATE = -4,       /* call made in the wrong state (e.g. no particles set) */
  NBODY_ERR_NOMEM = -5,
  NBODY_ERR_UNSUPPORTED = -6,
  NBODY_ERR_INTERNAL = -7     /* a bound the library proves was passed (nbody_get_groups_f64: more rounds than bodies) */
};

/* Arithmetic of the force accumulation. */
enum {
  NBODY_PREC_F32 = 0,         /* reference-compatible: fp32 pair law, fp32 accumulate */
  NBODY_PREC_F32_KAHAN = 1,   /* fp32 pair law, Kahan-compensated fp32 accumulate */
  NBODY_PREC_F64 = 2          /* fp64 state, pair law and accumulate */
};

/*
 * Handling of pairs at distance exactly 0 when eps == 0 (OctreeSearch.h:102, `if (d == 0) return;`).
 * EXACT and SELECT reproduce it for every representable distance; FLOOR adds the smallest eps^2 that
 * keeps G*m_max/d^3 finite in fp32 (about 1e-20: d == 0 pairs still contribute exactly 0, but pairs
 * closer than ~4e-7 length units are softened) and saves two vector instructions per pair.
 */
enum {
  NBODY_ZERO_EXACT = 0,       /* default: r2 += clamp01(1 - r2*2^126), 2 full-rate VALU ops */
  NBODY_ZERO_SELECT = 1,      /* compare + select (half-rate ops on gfx950); for A/B measurements */
  NBODY_ZERO_FLOOR = 2        /* eps^2 floor, not bit-faithful below d ~ 4e-7 */
};

/*
 * Force algorithm.  Both evaluate the same pair law over all pairs; they differ in summation order only.
 * TILED: every ordered pair (i, j), one-sided (kernels.hip).  SYMMETRIC: every unordered pair once, feeding
 * both bodies (kernels_sym.hip, kernels_sym64.hip; work plan csrc/sym_plan.h): fp32, Kahan fp32 and fp64 contexts;
 * when the bodies are sharded the slices must be equal multiples of 256 * i_per_thread bodies and the host drives
 * nbody_step_begin / all-to-all / nbody_step_end.  The per-body summation order then depends on the number of ranks
 * (TILED's does not).  AUTO picks SYMMETRIC where it applies and n_total >= 9216 (where its whole step gets faster
 * than the one-sided kernel's), else TILED.
 */
enum { NBODY_ALGO_AUTO = 0, NBODY_ALGO_TILED = 1, NBODY_ALGO_SYMMETRIC = 2 };

/* Device buffers reachable through nbody_device_ptr / nbody_bind_device_state. */
enum {
  NBODY_BUF_POSM = 0,         /* [n_total] x,y,z,mass  (float4, or double4 for NBODY_PREC_F64) */
  NBODY_BUF_VEL = 1,          /* [i_count] vx,vy,vz,0 */
  NBODY_BUF_ACC = 2           /* [i_count] ax,ay,az,0 */
};

/* Kernels whose device time nbody_kernel_time reports. */
enum { NBODY_KERNEL_FORCES = 0, NBODY_KERNEL_UPDATE = 1 };

/* FParticle — OctreeSearch.h:8-18.  Same field order and offsets (40 bytes). */
typedef struct nbody_particle {
  float Mass;
  float Position[3];
  float Velocity[3];
  float Acceleration[3];
} nbody_particle;

/*
 * Engine parameters.  The reference hard-codes G = 1e4 (OctreeSearch.h:104), no softening
 * (.h:101-104) and fp32; nbody_default_params fills in exactly those.
 */
typedef struct nbody_params {
  uint32_t struct_size;   /* sizeof(nbody_params), for ABI versioning */
  int32_t n_total;        /* bodies in the whole system (Particles.Num(), OctreeSearch.h:118) */
  int32_t i_begin;        /* first body this context owns (range partition over GPUs); default 0 */
  int32_t i_count;        /* bodies this context owns; 0 = n_total - i_begin */
  int32_t device;         /* HIP device ordinal */
  int32_t precision;      /* NBODY_PREC_* */
  double G;               /* gravitational constant; reference 1e4 */
  double eps;             /* Plummer softening length; reference 0 (d == 0 pairs are skipped).  Applied at any theta: at theta > 0
                             to the term of every node the walk accepts (see the Barnes-Hut paragraph below) */
  int32_t tile;           /* bodies per LDS tile: 64, 128, 256 (default), 512 */
  int32_t i_per_thread;   /* i-bodies per lane: 1, 2, 4 (8: fp32 symmetric kernels, 16: the plain one only); 0 = auto */
  int32_t j_split;        /* j-range chunks summed separately then combined in order; 0 = auto (a function of n_total only) */
  int32_t time_kernels;   /* nonzero: bracket kernels with HIP events for nbody_kernel_time */
  int32_t zero_mode;      /* how d == 0 pairs are dropped when eps == 0 (NBODY_ZERO_*); 0 = default.  No effect at theta > 0 */
  int32_t algorithm;      /* NBODY_ALGO_*; 0 = auto */
  float theta;            /* Barnes-Hut opening angle.  0 (default) = exact all-pairs, the hot path of this engine.  > 0 =
                             the reference's own tree walk (OctreeSearch.h:99-108; it ships 1.0, OctreeSearch.cpp:85) */
  int32_t bh_div_mode;    /* theta > 0 only: reading of `CenterOfMass /= TotalMass` in ComputeMass (OctreeSearch.h:95).  0 (default):
                             FVector::operator/=(float) multiplies by the fp32 reciprocal (UE4 4.9 as remembered — the engine
                             is not vendored); 1: three divisions.  The oracle has the same switch (div_mode). */
} nbody_params;

/* ---- lifecycle ---------------------------------------------------------------------------- */

/* Fill `p` with the reference-compatible defaults (G=1e4, eps=0, fp32, device 0). */
NBODY_AMD_API int nbody_default_params(nbody_params *p);

/* AOctreeSearch ctor + CreateSpacePoints' allocation (OctreeSearch.cpp:8,62).
 *
 * Reproducibility.  Every force pass is deterministic (no atomics in any sum): the same context, state and call sequence
 * give the same bits, run after run.  WHICH sums are formed — the launch geometry — is chosen here, once, from the
 * parameters and from two facts about the device: its compute-unit count (workgroup slots of the symmetric pass's work
 * plan) and, beyond N = 2^22, its total memory (whether the partial-sum pool is shared by phases); the strip-length
 * divisor K of that plan also follows an estimate of the pass's duration from rates measured on MI355X (6.6e12 / 6.0e12 /
 * 2.7e12 interactions/s: fp32 / compensated / fp64); between 16385 and 139264 bodies (compensated: 12288 ... 40960) a context
 * that owns all bodies runs the even-share plan instead — one work item per slot, a function of the body count, the bodies
 * per lane and the CU count (nbody_sym_plan_is_even).  Results are therefore reproducible on every MI355X, and across
 * library versions only where the release notes say so; on a part with another CU count they agree to rounding, not in
 * every bit.  (Plain fp32 systems of up to 16384 bodies run forces_block_pk_kernel: there the CU count only decides how
 * many bodies share a workgroup, which no sum depends on — the same bits on any part.)  nbody_get_launch_config,
 * nbody_get_algorithm and nbody_sym_pool_info say what was chosen;
 * NBODY_ALGO_TILED with explicit tile / i_per_thread / j_split depends on the parameters alone.
 *
 * Masses.  A context that owns all bodies re-reads every mass before every pass: a mass changed through a bound or handed-out
 * device buffer is seen at once.  SHARDED contexts (i_count < n_total) treat masses as immutable between uploads
 * (nbody_set_* / nbody_push_particles / nbody_load_checkpoint): the first go of a pass looks only at the own slice — the other
 * ranks' records may still be arriving — so a mass another rank changes in its buffer selects the general form of the kernels one
 * pass late. */
NBODY_AMD_API int nbody_create(const nbody_params *p, nbody_ctx **out);

/*
 * The same context over several GPUs of one node, driven by ONE caller thread — the reference's only caller is the game
 * thread (OctreeSearch.cpp:21-34).  Bodies are range-partitioned in equal slices over `devices` (n_total a multiple of
 * n_dev); every device keeps all positions.  Per step each device runs the force pass of its slice, [symmetric
 * algorithm] the j-side sums change hands by grouped ncclSend/ncclRecv, the slices are integrated, and ONE in-place
 * ncclAllGather of the positions (RCCL over xGMI; communicators from ncclCommInitAll, librccl loaded at this call)
 * brings every device up to date.  p->i_begin / i_count / device are ignored (the context owns all bodies).
 * theta > 0 (fp32): the reference's tree is ONE tree (OctreeSearch.cpp:79-81) and a body's walk (.cpp:83-86) reads it and writes
 * that body alone — every device builds the whole tree from its copy of the positions (the build is the reference's arithmetic in
 * a fixed order: the same bits everywhere), walks and integrates its own slice, and the same all-gather follows: frames equal the
 * one-device context's in EVERY byte, whatever n_dev is.
 * Every entry point of this header works on the result except the device-plumbing ones (nbody_set_stream, nbody_device_ptr,
 * nbody_bind_*, nbody_step_begin/_end, nbody_exchange_*), which report NBODY_ERR_UNSUPPORTED.  With n_dev = 1 results equal
 * nbody_create's bit for bit.
 */
NBODY_AMD_API int nbody_create_multi(const nbody_params *p, const int32_t *devices, int32_t n_dev, nbody_ctx **out);

/* CleanParticles (OctreeSearch.cpp:91-97).  NULL is allowed, like `delete NULL` there. */
NBODY_AMD_API void nbody_destroy(nbody_ctx *ctx);

/* Message of the last error on `ctx` (or of the last failed nbody_create when ctx is NULL). */
NBODY_AMD_API const char *nbody_last_error(const nbody_ctx *ctx);

NBODY_AMD_API int nbody_version(void);

/* Number of HIP devices visible (0 when there is none; never fails). */
NBODY_AMD_API int nbody_device_count(void);

/* ---- state in ----------------------------------------------------------------------------- */

/* Every call of this section is ordered behind whatever the context still has in flight on its stream (nbody_step returns before its
 * steps have run): the upload lands after the last queued update, whichever type the caller's arrays have, and the call returns once
 * the new state is on the device — the caller's arrays are its own again. */

/* TArray<FParticle> contents (OctreeSearch.h:8-18,118): all n_total records, `stride` bytes apart (>= 40). */
NBODY_AMD_API int nbody_set_particles(nbody_ctx *ctx, const void *aos, size_t stride, int32_t n);

/* The host has EDITED records of a running simulation.  In the reference `Particles` is the state itself (OctreeSearch.h:118;
 * the Tick reads and writes it in place, OctreeSearch.cpp:28-31): code that changes Particles[i] between two Ticks changes the
 * simulation, and nothing else restarts — the next tree is still rooted at the previous tree's CoM (OctreeSearch.cpp:77-79).
 * Same upload as nbody_set_particles (Mass, Position, Velocity, Acceleration of all n_total records), but the history stays:
 * nbody_steps_done goes on counting and the Barnes-Hut root centre is kept. */
NBODY_AMD_API int nbody_push_particles(nbody_ctx *ctx, const void *aos, size_t stride, int32_t n);

/* Native layout: posm4 = n_total x {x,y,z,m}, vel4 = n_total x {vx,vy,vz,unused}, fp32. */
NBODY_AMD_API int nbody_set_state_soa(nbody_ctx *ctx, const float *posm4, const float *vel4, int32_t n);

/* Same in fp64 (converted down for fp32 contexts). */
NBODY_AMD_API int nbody_set_state_soa_f64(nbody_ctx *ctx, const double *posm4, const double *vel4, int32_t n);

/* ---- the hot path ------------------------------------------------------------------------- */

/*
 * The force loop of CreateOctree (OctreeSearch.cpp:83-86) at theta = 0: Acceleration_i =
 * sum over j of the pair law (OctreeSearch.h:101-104) for the owned bodies against all n_total.
 */
NBODY_AMD_API int nbody_compute_forces(nbody_ctx *ctx);

/*
 * The body of Tick (OctreeSearch.cpp:25-32), `nsteps` times: forces(x_n); v += dt*a; x += dt*v.
 * dt <= 0 is a no-op, as PhDeltaTime <= 0 freezes the reference (.cpp:25).  Asynchronous on the
 * context's stream; the getters synchronise.  On a sharded context (i_count < n_total) nsteps
 * must be 1: the caller all-gathers NBODY_BUF_POSM across ranks between steps.
 */
NBODY_AMD_API int nbody_step(nbody_ctx *ctx, float dt, int32_t nsteps);

/*
 * The same step in two phases, for hosts that share the bodies over several GPUs:
 *   nbody_step_begin : force pass (OctreeSearch.cpp:83-86 at theta = 0) for the owned bodies
 *   nbody_step_end   : v += dt*a; x += dt*v for the owned bodies (OctreeSearch.cpp:28-31); dt <= 0 only stores a
 * Between them a sharded context running NBODY_ALGO_SYMMETRIC needs ONE all-to-all: it has evaluated each body pair
 * once and holds, in `send`, what its pairs contribute to every other rank's bodies (n_ranks segments of
 * bytes_per_rank, segment q for rank q); `recv` must receive segment r of every rank's `send`.  nbody_exchange_info
 * reports n_ranks = 0 when no exchange is needed.  After nbody_step_end the owned slice of NBODY_BUF_POSM is
 * all-gathered as with nbody_step.
 */
NBODY_AMD_API int nbody_step_begin(nbody_ctx *ctx);
NBODY_AMD_API int nbody_step_end(nbody_ctx *ctx, float dt);
/*
 * nbody_step_begin in two goes, so that the all-gather of the previous step's positions can still be in flight when the
 * next force pass starts ("compute own-range j-tiles while the gather is in flight"):
 *   nbody_step_begin_local  : the part of the force pass that needs the OWNED slice of NBODY_BUF_POSM only — on a sharded
 *                             fp32 NBODY_ALGO_SYMMETRIC context the strips whose j range lies inside the own slice (about
 *                             1/n_ranks of the rank's work); on any other context nothing
 *   nbody_step_begin_remote : the rest (everything, where the first go did nothing).  Queue it behind the gather:
 *                             an event wait on the context's stream is enough, the host need not block.
 * Same plan, same partial-sum segments, same order of additions as nbody_step_begin: the results are identical in every
 * bit.  The first go reads the masses of ALL bodies (they are what the last upload left; the gather rewrites them with
 * the same bits): a host that changes masses in the bound buffer must let the gather finish first.
 */
NBODY_AMD_API int nbody_step_begin_local(nbody_ctx *ctx);
NBODY_AMD_API int nbody_step_begin_remote(nbody_ctx *ctx);
NBODY_AMD_API int nbody_exchange_info(nbody_ctx *ctx, void **send, void **recv, size_t *bytes_per_rank, int32_t *n_ranks);
/* Use caller-owned device buffers (e.g. torch tensors) for the exchange: send = n_total x float4, recv = n_ranks x i_count x float4
 * (double4 on an fp64 context). */
NBODY_AMD_API int nbody_bind_exchange(nbody_ctx *ctx, void *send, void *recv);
/* Host-staged exchange for callers without a device-side collective: copy `send` out (n_total x 4 floats) /
 * copy `recv` in (n_ranks x i_count x 4 floats); doubles on an fp64 context. */
NBODY_AMD_API int nbody_exchange_read_send(nbody_ctx *ctx, void *host);
NBODY_AMD_API int nbody_exchange_write_recv(nbody_ctx *ctx, const void *host);

/*
 * Barnes-Hut mode: with theta > 0 the force pass is the reference's CreateOctree (OctreeSearch.cpp:
 * 74-89) on the device — same region octree (root centre = previous tree's CoM, half-width = ComputeCubeSize), same
 * mass upsweep, same depth-first walk with `Size/d < Theta`, same arithmetic — instead of the all-pairs kernels.
 * fp32 contexts only.  A context that owns a SLICE of the bodies (i_count < n_total: one rank of a sharded job, one device of
 * nbody_create_multi) builds the whole tree from the replicated positions and walks its own bodies; the caller all-gathers
 * NBODY_BUF_POSM between steps as at theta = 0.  nbody_set_particles / nbody_set_state_* reset the "previous CoM" to zero.
 * Systems of more than 4096 bodies sort a frame's path keys starting from the previous frame's order and take its Size out of the
 * previous frame's walk: a frame whose sort gives up (the records were replaced, the root box jumped) is queued again
 * by the library at the call's one wait; nothing of it shows but the time.
 * Softening (eps > 0): the walk goes where the reference's goes, on the unsoftened d (Size/d < Theta, the leaf rule, d == 0 ends the
 * subtree), and an accepted node adds float(G * M / ds^3) * (CoM - Pos) with ds = sqrtf(d^2 + eps2), eps2 = (float)(eps * eps), the
 * one fp32 add not fused; an eps whose square rounds to 0 in fp32 gives the reference's frame, bit for bit.  zero_mode has no effect.
 */
NBODY_AMD_API int nbody_set_theta(nbody_ctx *ctx, float theta);
/* The opening angle in force (nbody_params.theta, nbody_set_theta, or what nbody_load_checkpoint took over from a file). */
NBODY_AMD_API int nbody_get_theta(nbody_ctx *ctx, float *theta);
/*
 * The deepest tree a theta > 0 frame may build, 42 <= levels <= 200 (root = level 0); default 42.  A frame is answered iff the
 * reference's Octree::Add of that frame reaches depth <= levels; a frame that goes deeper is refused as before (NBODY_ERR_UNSUPPORTED,
 * "Barnes-Hut tree deeper than N levels"): the state is left alone and the frames queued behind it do nothing.  Above 42, clusters of
 * bodies that share a cell of level 42 are resolved on the device (at most 64 bodies per such cell; more are refused with a message
 * of their own) in a frame that costs more than an ordinary one; frames without such a cluster run as at 42.  fp32 contexts only
 * (NBODY_ERR_UNSUPPORTED otherwise); allowed at theta == 0, in force once theta > 0.  Every device of nbody_create_multi and every
 * slice context takes it.  A setting, not state: checkpoints do not keep it.  Other values: NBODY_ERR_INVALID.
 */
NBODY_AMD_API int nbody_set_bh_max_depth(nbody_ctx *ctx, int32_t levels);
NBODY_AMD_API int nbody_get_bh_max_depth(nbody_ctx *ctx, int32_t *levels);
/* Nodes and levels of the last tree built, and its root CoM (= the next frame's root centre). */
NBODY_AMD_API int nbody_bh_stats(nbody_ctx *ctx, int32_t *nodes, int32_t *levels, float root_com[3]);
/* What DrawOctreeBoxes passes to DrawDebugBox when ShowOctree is set (OctreeSearch.cpp:39-40): for every body the box
 * (Origin.x, Origin.y, Origin.z, Size) of the leaf that held it in the last tree; 4 floats per body, `stride` bytes apart. */
NBODY_AMD_API int nbody_bh_leaf_boxes(nbody_ctx *ctx, float *boxes, size_t stride);
/* The order in which DrawOctreeBoxes (OctreeSearch.cpp:36-45) meets the bodies on the last tree built: depth first,
 * children 0..7; order[k] = index of the body in the k-th occupied leaf.  n_total ints. */
NBODY_AMD_API int nbody_bh_leaf_order(nbody_ctx *ctx, int32_t *order);

/*
 * The field at points that are not bodies (build-defined: the reference computes gravity at the bodies only).  Plain fp32 contexts
 * (NBODY_PREC_F32) on one device that own all bodies; Kahan, fp64 and slice contexts (i_count < n_total) and nbody_create_multi
 * contexts report NBODY_ERR_UNSUPPORTED.
 *
 * nbody_field_at: the acceleration the bodies exert on a massless point, for n caller-given points — xyz: 3 floats each, `stride`
 * bytes apart (>= 12: &Particles[0].Position with stride 40 works); acc: 3 floats each, `acc_stride` bytes apart (>= 12).
 *   theta == 0: acc[k] = sum over all n_total bodies, at their current positions, of the context's own pair law (G, eps, zero_mode;
 *     NBODY_ZERO_SELECT contexts get the clamp form, which drops the same pairs); a point exactly on a body skips that pair when
 *     eps == 0, as d == 0 does (OctreeSearch.h:102).  Every point's sum runs in a fixed order — the bodies in chunks that follow from
 *     n_total alone, the chunks in order — so a point's result depends neither on the other points of the call, nor on n, nor on the
 *     strides, nor on the device.
 *   theta > 0: the walk of Octree::ComputeForces (OctreeSearch.h:99-108) from the point over THE LAST TREE BUILT — the tree nbody_bh_stats,
 *     nbody_bh_leaf_boxes and nbody_bh_leaf_order describe —: the same opening rule on the unsoftened d, the same leaf rule, d == 0 ends the
 *     subtree, the same term, softening included; at a body's own position it gives that body's own sum in every bit.  After nbody_step or
 *     nbody_tick the last tree is that of the positions BEFORE that frame's update — the field the bodies just felt; for the field at the
 *     current positions call nbody_compute_forces first.  Without a valid last tree — none built yet, the last frame refused, theta changed
 *     since it was built — NBODY_ERR_STATE; a last tree built deeper than 42 levels (nbody_set_bh_max_depth) NBODY_ERR_UNSUPPORTED.
 * n == 0 is a no-op; NULL pointers, n < 0 and strides < 12 are NBODY_ERR_INVALID.  The call synchronises and changes nothing a getter
 * of the state shows: bodies, accelerations, steps done, root centre and tree stay what they were.  The one exception are the kernel
 * timers of a time_kernels context: a query's device time is added to NBODY_KERNEL_FORCES and counts as one pass there
 * (nbody_kernel_time), and at theta == 0 its workgroups enter nbody_kernel_clock's average.
 *
 * Tracers: massless bodies the engine advances along with the bodies.  nbody_set_tracers replaces any earlier set — pos4 / vel4: n x 4
 * floats (the 4th ignored); vel4 NULL = at rest; n = 0 removes them.  In every step of nbody_step and nbody_tick with dt > 0 a tracer at
 * y_n gets a = the field of the bodies at x_n — the positions that step's force pass uses (theta > 0: the walk of that frame's tree) —,
 * then v += dt*a; y += dt*v, the bodies' own fp32 kick-drift (OctreeSearch.cpp:29-30).  nbody_compute_forces stores the tracers'
 * accelerations as well and moves nothing; dt <= 0 leaves them alone, and nbody_step_begin / nbody_step_end touch neither their
 * state nor their stored accelerations, at any theta.  Tracers never act on bodies or on each other: a context with tracers advances its bodies exactly as the same context without them, byte for byte.  A theta > 0
 * frame that is refused leaves the tracers untouched like the bodies.  Their device time counts under NBODY_KERNEL_FORCES.
 * Uploads (nbody_set_*, nbody_push_particles, nbody_load_checkpoint) keep the tracers.  Checkpoints do not store them (NBDYCKP2 is what
 * it was): a host saves and restores them with nbody_get_tracers / nbody_set_tracers, which is bit-exact.
 * Tracers and trees deeper than 42 levels exclude each other: whichever of nbody_set_tracers and nbody_set_bh_max_depth(> 42) comes second
 * reports NBODY_ERR_UNSUPPORTED.
 */
NBODY_AMD_API int nbody_field_at(nbody_ctx *ctx, const float *xyz, size_t stride, int32_t n, float *acc, size_t acc_stride);
NBODY_AMD_API int nbody_set_tracers(nbody_ctx *ctx, const float *pos4, const float *vel4, int32_t n);
/* pos4 / vel4 / acc4: nbody_tracer_count x 4 floats each, any may be NULL.  Synchronises. */
NBODY_AMD_API int nbody_get_tracers(nbody_ctx *ctx, float *pos4, float *vel4, float *acc4);
NBODY_AMD_API int nbody_tracer_count(nbody_ctx *ctx, int32_t *n);

/*
 * The gravitational potential (build-defined: the reference computes none), on the contexts that answer nbody_field_at: plain fp32, one
 * device, owning all bodies; Kahan, fp64, slice and nbody_create_multi contexts report NBODY_ERR_UNSUPPORTED.
 *
 * nbody_potential_at: phi at n caller-given points — xyz: 3 floats each, `stride` bytes apart (>= 12); phi: one float each, `phi_stride`
 * bytes apart (>= 4).
 *   theta == 0: phi(x) = -sum_j G m_j / sqrt(|x - x_j|^2 + eps^2) over all n_total bodies at their current positions.  With eps == 0 a pair
 *     at distance exactly 0 contributes nothing, whatever zero_mode the context has (NBODY_ZERO_FLOOR's eps floor is NOT applied: it would
 *     add G m / 1e-10); with eps > 0 a point exactly on a body does feel that body's -G m / eps, the Plummer potential at its centre.  The
 *     pair term is fp32 (a 1-ulp reciprocal square root); a chunk's sum is one chain of fused multiply-adds in body order, the chunks —
 *     those of nbody_field_at, a function of n_total alone — are added in chunk order in fp64, and the sum is negated and rounded once.  A
 *     point's bits depend neither on the other points of the call, nor on n, nor on the strides, nor on the device.
 *   theta > 0: the walk of Octree::ComputeForces (OctreeSearch.h:99-108) over THE LAST TREE BUILT, with nbody_field_at's rules: the same
 *     opening test on the unsoftened d, the same leaf rule, d == 0 ends the subtree.  An accepted node adds, in fp64,
 *     G * (double)M / (double)ds, ds = sqrtf(d^2 + eps^2) correctly rounded in fp32 (the eps^2 add one fp32 add, not fused), the division
 *     correctly rounded; the fp64 sum runs in walk order and the result is (float)(-sum) — reproducible in plain C with contraction off.
 *     Consequences of the reference's rule: a point exactly on the root's CoM gets 0, a point far outside the single root term.  Without a
 *     valid last tree NBODY_ERR_STATE, after a tree deeper than 42 levels NBODY_ERR_UNSUPPORTED, as nbody_field_at reports them.
 *   n == 0 is a no-op; NULL pointers, n < 0, stride < 12 and phi_stride < 4 are NBODY_ERR_INVALID.  The call synchronises and changes
 *   nothing a getter of the state shows; its device time counts as one pass under NBODY_KERNEL_FORCES, as a field query's does.
 *
 * nbody_get_potentials: every body's potential from all OTHER bodies at the CURRENT positions — n_total floats, `stride` bytes apart (>= 4).
 *   theta == 0: the sum above with the body itself left out BY INDEX (not by subtracting G m_i / eps afterwards); other bodies on the same
 *     point are skipped when eps == 0, as nbody_energy skips them.  Changes nothing a getter shows.
 *   theta > 0: the call first runs exactly what nbody_compute_forces runs — the tree of the current positions is built, the next frame's
 *     root centre stays, the stored accelerations (the tracers' too) become those of the current positions — and then walks that tree
 *     from every body, which meets its own leaf at d == 0.  Side effects: as after nbody_compute_forces.  A refused frame returns that
 *     frame's error and no potentials.
 *
 * nbody_energy_fast: ke = 1/2 sum m_i v_i^2 in fp64, as nbody_energy computes it; pe = 1/2 sum m_i phi_i with phi_i the UNROUNDED fp64
 *   per-body potentials of nbody_get_potentials (the fp64 fold at theta == 0, the fp64 walk sum at theta > 0), reduced in fp64 in a fixed
 *   order without atomics: the same bits every run.  At theta > 0 it costs about one force pass where nbody_energy evaluates all pairs; its
 *   potential is that of the opening rule's monopoles.  Synchronises; side effects as nbody_get_potentials.  Either output may be NULL.
 */
NBODY_AMD_API int nbody_potential_at(nbody_ctx *ctx, const float *xyz, size_t stride, int32_t n, float *phi, size_t phi_stride);
NBODY_AMD_API int nbody_get_potentials(nbody_ctx *ctx, float *phi, size_t stride);
NBODY_AMD_API int nbody_energy_fast(nbody_ctx *ctx, double *ke, double *pe);

/*
 * The tidal tensor T_ab = d a_a / d x_b, the second derivative of the potential (build-defined, like the potential), on the contexts that
 * answer nbody_potential_at: plain fp32, one device, owning all bodies; Kahan, fp64, slice and nbody_create_multi contexts report
 * NBODY_ERR_UNSUPPORTED.  Sign and softening are the pair law's own: with d = x_j - x and s^2 = |d|^2 + eps^2,
 *     T_ab(x) = sum_j G m_j [ 3 d_a d_b / s^5 - delta_ab / s^3 ].
 * Six components, in the order of nbody_moments.second: xx, yy, zz, xy, xz, yz.  At eps == 0 the trace is 0; at eps > 0 it is
 * -3 sum G m eps^2 / s^5 (the Plummer density).
 *
 * nbody_tidal_at: T at n caller-given points — xyz: 3 floats each, `stride` bytes apart (>= 12); t: 6 floats each, `t_stride` bytes apart
 * (>= 24).
 *   theta == 0: the sum over all n_total bodies at their current positions.  With eps == 0 a pair at distance exactly 0 contributes
 *     nothing, whatever zero_mode the context has (the potential's rule: no NBODY_ZERO_FLOOR eps floor, and for the same reason); with
 *     eps > 0 a point exactly on a body feels that body's -G m / eps^3 on the diagonal.  The pair term is fp32 on the potential's distance
 *     term (a 1-ulp reciprocal square root t = 1 / s): S_ab += (3 G m t^3)(d_a t)(d_b t) and Q += G m t^3 — no s^-5 is formed, so a pair
 *     is finite wherever 3 G m / s^3 is.  A chunk's seven sums are each one chain of fused multiply-adds in body order; the chunks —
 *     those of nbody_field_at, a function of n_total alone — are added in chunk order in fp64, T_aa = S_aa - Q is formed there, and each
 *     component is rounded once.  A point's bits depend neither on the other points of the call, nor on n, nor on the strides, nor on
 *     the device.
 *   theta > 0: the walk of Octree::ComputeForces (OctreeSearch.h:99-108) over THE LAST TREE BUILT, with nbody_potential_at's rules.  An
 *     accepted node (CoM c, mass M) adds, every operation one correctly rounded operation (plain C with contraction off reproduces it):
 *         e_a = p_a - c_a (fp32, the differences d^2 was made of);  ds = sqrtf(d^2 [+ eps^2]) (fp32; the add one fp32 add)
 *         u = 1.0 / (double)ds;  u2 = u * u;  gm = G * (double)M;  q3 = (gm * u) * u2;  h = (3.0 * q3) * u2
 *         hx = h * ex;  hy = h * ey;  hz = h * ez                       (the doubles of the fp32 e)
 *         Sxx += hx * ex;  Sxy += hx * ey;  Sxz += hx * ez;  Syy += hy * ey;  Syz += hy * ez;  Szz += hz * ez;  Q += q3
 *     to seven fp64 sums in walk order; the result is (float)(Sxx - Q), (float)(Syy - Q), (float)(Szz - Q), (float)Sxy, (float)Sxz,
 *     (float)Syz.  Consequences of the reference's rule, as for the potential: a point exactly on the root's CoM gets zeros, and from a
 *     body's own position its own leaf adds nothing.  Without a valid last tree NBODY_ERR_STATE, after a tree deeper than 42 levels
 *     NBODY_ERR_UNSUPPORTED, as nbody_field_at reports them.
 *   n == 0 is a no-op; NULL pointers, n < 0, stride < 12 and t_stride < 24 are NBODY_ERR_INVALID.  The call synchronises and changes
 *   nothing a getter of the state shows; its device time counts as one pass under NBODY_KERNEL_FORCES.
 *
 * nbody_get_tidal: every body's tensor from all OTHER bodies at the CURRENT positions — n_total x 6 floats, `stride` bytes apart (>= 24).
 *   theta == 0: the sum above with the body itself left out BY INDEX; other bodies on the same point are skipped when eps == 0.  Changes
 *     nothing a getter shows.
 *   theta > 0: first exactly what nbody_compute_forces runs, then the walk of that tree from every body, as nbody_get_potentials: the same
 *     side effects, and a refused frame returns that frame's error and no tensors.
 *
 * nbody_tidal_time: the tidal time scale t = ||T||_F^(-1/2) — a time that depends neither on velocities, nor on the frame, nor on a
 *   softening length — minimised over the bodies: what a host needs to choose a dt the current state can bear.  Per body
 *   n2 = ||T_i||_F^2 = (Txx^2 + Tyy^2) + Tzz^2 + 2 ((Txy^2 + Txz^2) + Tyz^2) in fp64 with contraction off, from the UNROUNDED fp64 tensors
 *   of nbody_get_tidal (the fp64 fold at theta == 0, the fp64 walk sums at theta > 0); the largest n2 and the lowest body index that
 *   attains it come from a fixed-order reduction without atomics: the same bits and the same body every run.  *t_min =
 *   1 / sqrt(sqrt(max n2)); +inf when the maximum is 0 (a single body), 0 when it is not finite.  Synchronises; side effects as
 *   nbody_get_tidal.  Either output may be NULL, not both (NBODY_ERR_INVALID).
 */
NBODY_AMD_API int nbody_tidal_at(nbody_ctx *ctx, const float *xyz, size_t stride, int32_t n, float *t, size_t t_stride);
NBODY_AMD_API int nbody_get_tidal(nbody_ctx *ctx, float *t, size_t stride);
NBODY_AMD_API int nbody_tidal_time(nbody_ctx *ctx, double *t_min, int32_t *body);

/*
 * The jerk j = da/dt of the pair law beside the acceleration a (build-defined, like the potential) — the one per-body quantity that
 * depends on the VELOCITIES.  With d = x_j - x, w = v_j - v and s^2 = |d|^2 + eps^2,
 *     a(x) = sum_j G m_j d / s^3        j(x, v) = sum_j G m_j [ w / s^3 - 3 (d . w) d / s^5 ]
 * with the context's G and eps.  Positions, masses and velocities are those nbody_get_particles / nbody_get_state_soa would deliver at
 * that moment — the live buffers, whichever the stepping path has left current, bound buffers included (as nbody_get_moments reads them).
 * After nbody_step the stored velocity is the STAGGERED one (v_(n+1/2) beside x_(n+1), OctreeSearch.cpp:29-30): a host that wants the
 * synchronised jerk synchronises the velocities itself.
 *
 * At EVERY theta both sums are the pair sum over all n_total bodies: the tree holds no node velocities (nbody_energy sets the precedent:
 * all pairs at theta > 0 too).  So these calls need no tree, build none, work whether or not a last tree exists, and change nothing a
 * getter shows at any theta — state, stored accelerations, tracers, steps done, root centre, last tree.  The acceleration they return
 * is the pair sum's: at theta > 0 that is NOT the monopole walk's that nbody_compute_forces stores.
 *
 * Contexts: one device, owning all bodies — slice contexts (i_count < n_total) and nbody_create_multi contexts report
 * NBODY_ERR_UNSUPPORTED from all four calls.  nbody_get_jerk, nbody_get_jerk_f64 and nbody_jerk_time answer on all three precisions;
 * nbody_jerk_at on those whose state is fp32 (NBODY_PREC_F32, NBODY_PREC_F32_KAHAN) — an fp64 context reports NBODY_ERR_UNSUPPORTED
 * there, as its points would have to be doubles.  No particles set: NBODY_ERR_STATE.  All four synchronise; their device time counts as
 * one pass under NBODY_KERNEL_FORCES (the kernels do not enter nbody_kernel_clock's average).
 *
 * The d == 0 rule is the potential's: with eps == 0 a pair at distance exactly 0 is dropped from BOTH sums, whatever zero_mode the context
 * has (no NBODY_ZERO_FLOOR eps floor); with eps > 0 a point exactly on a body feels G m w / eps^3 from it in the jerk and nothing in
 * the acceleration.
 *
 * Arithmetic, fp32 state (a Kahan context runs the same kernel on its fp32 state: bit-equal to a plain fp32 context holding that state):
 *   the potential's distance term (a 1-ulp reciprocal square root t = 1 / s, or 0 for a pair that adds nothing), then in fp32
 *       g = G m t;  g2 = g t;  q = g2 t;  n_a = d_a t (|n| <= 1);  k = n . w (a product and two fused multiply-adds in z, y, x order)
 *       u_a = fma(-3 k, n_a, w_a);  A_a = fma(q, d_a, A_a);  J_a = fma(q, u_a, J_a)
 *   — no s^-5 is formed: a pair is finite wherever 4 G m |w| / s^3 is.  A chunk's six sums are each one chain of fused multiply-adds in
 *   body order; the chunks — those of nbody_field_at, a function of n_total alone — are added in chunk order in fp64, and each component
 *   is rounded once.  A point's bits depend neither on the other points of the call, nor on n, nor on the strides, nor on the device.
 * Arithmetic, fp64 state: t = 1 / s as the fp64 force kernels form it (0 where s^2 == 0 and for j == i), then q = G m t^3,
 *   k = (d . w) t^2, A += q d, J += q (w - 3 k d): chains of fused multiply-adds in body order per chunk, the chunks added in chunk order.
 *
 * nbody_jerk_at: a and j at n massless points — xyz and vel: 3 floats each, `stride` / `vel_stride` bytes apart (>= 12); vel == NULL
 *   means at rest and gives the bits an array of zeros gives.  acc and jerk: 3 floats each, >= 12 bytes apart; either may be NULL, not
 *   both.  n == 0 is a no-op; NULL points, n < 0, both outputs NULL or a stride too small are NBODY_ERR_INVALID.
 * nbody_get_jerk / nbody_get_jerk_f64: every body's a and j from all OTHER bodies — the body itself left out BY INDEX; other bodies on
 *   the same point are skipped when eps == 0 and felt when eps > 0.  n_total x 3 floats (strides >= 12) or doubles (strides >= 24);
 *   either output may be NULL, not both (NBODY_ERR_INVALID).  _f64 delivers the UNROUNDED fp64 results — the fp64 fold on fp32-state
 *   contexts, the fp64 sums on fp64 contexts —, the float form the same rounded once per component.
 * nbody_jerk_time: the step-size criterion |a| / |j|, minimised over the bodies.  Per body k_i = |j_i|^2 / |a_i|^2 from those unrounded
 *   fp64 vectors, each squared norm (x x + y y) + z z in fp64 with contraction off; 0 / 0 counts as 0, x / 0 with x > 0 as +inf, and a
 *   value that is not finite as +inf.  The largest k and the lowest body index that attains it come from nbody_tidal_time's fixed-order
 *   reduction: the same bits and the same body every run.  *t_min = 1 / sqrt(max k); +inf when the maximum is 0 (a single body), 0 when
 *   it is not finite.  Either output may be NULL, not both (NBODY_ERR_INVALID).
 */
NBODY_AMD_API int nbody_jerk_at(nbody_ctx *ctx, const float *xyz, size_t stride, const float *vel, size_t vel_stride, int32_t n,
                                float *acc, size_t acc_stride, float *jerk, size_t jerk_stride);
NBODY_AMD_API int nbody_get_jerk(nbody_ctx *ctx, float *acc, size_t acc_stride, float *jerk, size_t jerk_stride);
NBODY_AMD_API int nbody_get_jerk_f64(nbody_ctx *ctx, double *acc, size_t acc_stride, double *jerk, size_t jerk_stride);
NBODY_AMD_API int nbody_jerk_time(nbody_ctx *ctx, double *t_min, int32_t *body);

/*
 * Fourth-order Hermite stepping (build-defined: the reference has one integrator, the kick-drift of nbody_step, first order in the
 * position) — Makino & Aarseth's shared-step predict-evaluate-correct scheme P(EC) on the fp64 jerk pass of nbody_get_jerk_f64.  On the
 * two-body orbit of DESIGN 4.11 one period in 256 steps ends 2.9e-7 of the separation away from its start where nbody_step ends 2.0e-3
 * away, and halving dt divides the error by 16.
 *
 * Contexts: NBODY_PREC_F64, one device, owning all bodies (such contexts are at theta == 0).  NBODY_PREC_F32 and NBODY_PREC_F32_KAHAN
 * contexts, slice contexts (i_count < n_total) and nbody_create_multi contexts report NBODY_ERR_UNSUPPORTED from all five calls, with a
 * message that says why.  No particles set, or a nbody_step_begin whose nbody_step_end is pending: NBODY_ERR_STATE.
 *
 * The stored (x, v) are taken as SYNCHRONISED: v is the velocity at the positions' time.  nbody_step leaves the velocity staggered
 * (v_(n+1/2) beside x_(n+1)); a host that mixes the two integrators on one context must know what it is doing.  G, eps and the d == 0
 * rule are the jerk's.
 *
 * One step of length dt, per component, every bracket ONE correctly rounded fp64 operation in the order written (the kernels are
 * compiled with contraction off; plain C or numpy reproduces a step in every bit from nbody_get_jerk_f64's vectors) — the constants
 * c2 = (dt dt) 0.5, c3 = ((dt dt) dt) / 6, ch = dt 0.5, c12 = (dt dt) / 12, d2 = dt dt, d3 = (dt dt) dt are the host's doubles:
 *   predict    xp = ((x + dt v) + c2 a0) + c3 j0;   vp = (v + dt a0) + c2 j0            (xp carries the mass, vp.w = 0)
 *   evaluate   (a1, j1) = what nbody_get_jerk_f64 returns on a context holding (xp, vp): the same kernel, fold and geometry
 *   correct    v1 = v + (ch (a0 + a1) + c12 (j0 - j1));   x1 = x + (ch (v + v1) + c12 (a0 - a1));   da = a0 - a1
 *              a2_0 = ((-6 da) - dt ((4 j0) + (2 j1))) / d2;   a3 = ((12 da) + (6 dt) (j0 + j1)) / d3;   a2_1 = a2_0 + dt a3
 *   store      x := x1, v := v1 (masses and the velocities' fourth component stay), NBODY_BUF_ACC := (a1, 0)
 *   cache      (a0, j0) := (a1, j1), a2 := a2_1, a3 := a3 — the derivatives at the new time
 *
 * The cache — a0, j0, a2, a3 and whether they belong to the stored state — lives on the device, is allocated at first use and is NOT part
 * of a checkpoint.  While it is valid a step costs ONE jerk pass (one pass under NBODY_KERNEL_FORCES; predictor and corrector together
 * count as one pass under NBODY_KERNEL_UPDATE); the first step after an invalidation first evaluates (a0, j0) at the stored (x, v): one
 * more pass.  These calls invalidate it: every upload (nbody_set_particles, nbody_push_particles, nbody_set_state_soa[_f64],
 * nbody_load_checkpoint), nbody_step / nbody_tick / nbody_step_end with dt > 0, nbody_bind_device_state, nbody_device_ptr and
 * nbody_hermite_restart.  After a bind or a handed-out pointer the context cannot know who writes the state: from then on every
 * nbody_hermite_step / _timescale / _advance CALL evaluates anew at entry (once per call, not once per step).  nbody_compute_forces
 * leaves the cache alone.  Checkpoints stay NBDYCKP2 byte for byte: a resumed run restarts from the corrected state, and the same
 * trajectory on the context that wrote the file is "nbody_save_checkpoint, nbody_hermite_restart, go on" — equal in every byte.
 *
 * nbody_hermite_step: nsteps steps of length dt; steps_done grows by nsteps.  Asynchronous like nbody_step.  dt <= 0 is a no-op that
 *   returns NBODY_OK, like nbody_step's; a dt that is not finite or nsteps < 0 is NBODY_ERR_INVALID.
 * nbody_hermite_timescale: the shared step's time scale from the cache, in one pass over it and nbody_jerk_time's fixed-order reduction
 *   (no atomics: the same bits and the same body every run).  Norms are sqrt((x x + y y) + z z): A = |a0|, J = |j0|, S = |a2|, C = |a3|.
 *   With derivatives (a step has been taken since the last invalidation) *kind = 1, Aarseth's criterion: k_i = (J C + S S) / (A S + J J),
 *   0 / 0 counting as 0, x / 0 as +inf and a value that is not finite as +inf; *t_min = 1 / sqrt(max k), *body the lowest index that
 *   attains the maximum.  Without, *kind = 0: nbody_jerk_time's own value and body from the cached (a0, j0), which the call evaluates
 *   first if they are invalid.  In both kinds a maximum of 0 gives +inf and one that is not finite 0.  Synchronises; changes nothing a
 *   getter shows.  Any output may be NULL, not all three (NBODY_ERR_INVALID).
 * nbody_hermite_advance: shared adaptive steps until t_span has passed or max_steps have been taken.  Per step, with (t, kind) that
 *   step's nbody_hermite_timescale: dt = min(dt_max, kind == 1 ? sqrt(eta) t : eta_start t); a dt >= t_span - t_acc becomes
 *   t_span - t_acc, and *t_done then t_span exactly.  The host reads 16 bytes per step.  *t_done = the time covered, *steps = the steps
 *   taken (either may be NULL).  eta, eta_start and dt_max must be > 0 (dt_max may be +inf), t_span >= 0 and finite, max_steps >= 0:
 *   anything else is NBODY_ERR_INVALID.  A chosen dt that is 0 or not finite stops the call with NBODY_ERR_STATE and a message that names
 *   the body; the state, *t_done and *steps are those of the last good step.
 * nbody_hermite_get: the cache, 12 doubles per body — a0, j0, a2, a3 —, `stride` bytes apart (>= 96, else NBODY_ERR_INVALID).
 *   NBODY_ERR_STATE while (a0, j0) are invalid; a2 and a3 read as zeros while there are no derivatives.  Synchronises.
 * nbody_hermite_restart: forgets the cache; the next call starts from the stored (x, v) alone, as a context that loaded them would.
 */
NBODY_AMD_API int nbody_hermite_step(nbody_ctx *ctx, double dt, int32_t nsteps);
NBODY_AMD_API int nbody_hermite_timescale(nbody_ctx *ctx, double *t_min, int32_t *body, int32_t *kind);
NBODY_AMD_API int nbody_hermite_advance(nbody_ctx *ctx, double t_span, double eta, double eta_start, double dt_max, int64_t max_steps,
                                        double *t_done, int64_t *steps);
NBODY_AMD_API int nbody_hermite_get(nbody_ctx *ctx, double *d12, size_t stride);
NBODY_AMD_API int nbody_hermite_restart(nbody_ctx *ctx);

/* Hermite BLOCK time steps (build-defined: the reference has one step for all bodies) — the same predictor, evaluation and corrector
 * with a step per body: a hard binary steps often, the rest of the system seldom, and an evaluation costs (bodies due) x N pairs instead
 * of N^2.  Where: the contexts that answer nbody_hermite_step (NBODY_PREC_F64, one device, all bodies); fp32 and Kahan contexts, slice
 * contexts and nbody_create_multi contexts report NBODY_ERR_UNSUPPORTED with that call's reasons.  No particles set: NBODY_ERR_STATE.
 *
 * Time is counted in integer ticks: tick = ldexp(dt_max, -levels), 0 <= levels <= 40.  Body i holds a time T_i (int64 ticks), a level
 * k_i in 0 .. levels whose step is 2^(levels - k_i) ticks = dt_max 2^-k_i, (x_i, v_i) AT T_i in the context's state buffers and
 * (a0, j0, a2, a3)_i at T_i in the Hermite cache.  T_i is always a multiple of the body's step, so every body lands on every multiple
 * of 2^levels ticks: a FRAME end, where the stored state is synchronised.  In between it is RAGGED: x_i is at T_i.
 *
 * One block step — every bracket ONE correctly rounded fp64 operation, contraction off, as in the paragraph above:
 *   schedule   T_next = min_i (T_i + step_i); the active set = the bodies that attain it, as a list in ascending body index (built by a
 *              scan: no atomics).  No body's result depends on its place in the list or on the other members.
 *   predict    EVERY body to T_next: dt_i = (double)(T_next - T_i) * tick (for an active body exactly dt_max 2^-k_i); on the device
 *              c2 = (dt_i dt_i) 0.5, c3 = ((dt_i dt_i) dt_i) / 6;  xp = ((x + dt_i v) + c2 a0) + c3 j0;  vp = (v + dt_i a0) + c2 j0
 *   evaluate   (a1, j1) of the ACTIVE bodies against all N predicted bodies: for every active body, in every bit, what
 *              nbody_get_jerk_f64 returns for that body on a context holding (xp, vp) — the same chunks, pair operations and order
 *   correct    the active bodies, by the corrector above with the body's own dt_i (ch, c12, d2, d3 formed on the device in that order):
 *              x, v, NBODY_BUF_ACC := (a1, 0), (a0, j0) := (a1, j1), a2 := a2_1, a3, T_i := T_next.  Inactive bodies keep every byte.
 *   levels     of the active bodies: k = (J C + S S) / (A S + J J) of nbody_hermite_timescale from the NEW vectors; t = +inf for k == 0,
 *              0 for a k that is not finite, else 1.0 / sqrt(k); dt_c = sqrt(eta) * t (sqrt(eta) the host's double); the wanted level
 *              kw = nbody_hermite_block_level(dt_c, dt_max, levels, &hit).  kw > k_i: k_i := kw (a smaller step, by any amount).
 *              kw < k_i and T_next a multiple of 2^(levels - k_i + 1): k_i := k_i - 1 (one level up at most, and only when aligned).
 *              Otherwise k_i stays.
 * nbody_steps_done grows by one per block step; a block step is one pass under NBODY_KERNEL_FORCES and — schedule, predictor and
 * corrector together — one under NBODY_KERNEL_UPDATE.  The host reads 16 bytes per block step (T_next and the number of active bodies)
 * to size the evaluation.
 *
 * nbody_hermite_block_level (host only, no context): the smallest k in 0 .. levels with ldexp(dt_max, -k) <= dt_c.  If there is none
 *   (dt_c below the smallest step, 0, or not a number) it returns `levels` and *floor_hit = 1 — the body is CLAMPED to the deepest level,
 *   not refused, and counted —; otherwise *floor_hit = 0 (floor_hit may be NULL).  levels outside 0 .. 40: -1.
 * nbody_hermite_block_begin: starts a session at tick 0 from the stored (x, v), taken as synchronised.  (a0, j0) come from the shared
 *   cache where it is valid (its a2, a3 too, if a step left them) and otherwise from one evaluation at the stored state (one pass; a2 and
 *   a3 then read as zeros until a body has stepped).  level_in, if not NULL: n_total levels, each 0 .. levels (else NBODY_ERR_INVALID) —
 *   how a host resumes, checkpoints hold no levels.  NULL: every body gets the level of dt_c = eta_start * t, t from nbody_jerk_time's
 *   per-body k = |j|^2 / |a|^2 with the same 0 / not-finite rules (a body no level fits is a floor hit here too).  dt_max, eta and
 *   eta_start must be finite and > 0, levels 0 .. 40 and the tick a normal double: anything else is NBODY_ERR_INVALID.  On a session in
 *   mid-frame: NBODY_ERR_STATE; at a frame end the old session ends and the new one begins.  Synchronises.  On a context whose
 *   buffers are bound or whose pointers are out, begin evaluates anew like every Hermite call; the session then trusts the state
 *   until it ends (a new nbody_device_ptr or bind ends it).
 * nbody_hermite_block_advance: block steps until T_sys reaches (floor(T_sys / 2^levels) + frames) 2^levels or max_block_steps have been
 *   taken; frames == 0 takes none.  After a stop in mid-frame the state is ragged; a later call with frames = 1 finishes the frame.
 *   *out (may be NULL; set out->struct_size = sizeof(nbody_hermite_block_stats) first, another size is NBODY_ERR_INVALID) gets the totals
 *   since begin.  frames or max_block_steps < 0, or frames whose end passes 2^62 ticks: NBODY_ERR_INVALID.  No session: NBODY_ERR_STATE.
 * nbody_hermite_block_get: T_i and k_i, n_total values each; either may be NULL.  No session: NBODY_ERR_STATE.  Synchronises.
 *
 * What ends a session: everything that invalidates the shared cache (the list above: uploads, nbody_step / nbody_tick / nbody_step_end
 * with dt > 0, nbody_bind_device_state, nbody_device_ptr) and nbody_hermite_restart — in mid-frame the state then stays ragged, which is
 * the caller's to know.  nbody_hermite_step / _timescale / _advance report NBODY_ERR_STATE on a session in mid-frame, with a message that
 * says why; at a frame end they work from the cache and end the session.  nbody_hermite_get works during a session: a body's row belongs
 * to its own T_i.  Checkpoints stay NBDYCKP2 byte for byte and hold neither cache nor levels: the trajectory a resumed run takes —
 * load, begin with the saved levels, go on — is "nbody_save_checkpoint, nbody_hermite_restart, nbody_hermite_block_begin with the levels
 * of nbody_hermite_block_get, go on" on the context that wrote the file, equal in every byte.
 */
typedef struct nbody_hermite_block_stats {
  uint32_t struct_size;   /* caller sets sizeof(nbody_hermite_block_stats) before the call */
  int32_t synchronised;   /* 1: T_sys is a frame end, every body is at T_sys */
  int64_t ticks;          /* T_sys */
  int64_t frames_done;    /* floor(T_sys / 2^levels) */
  int64_t block_steps;
  int64_t body_steps;     /* sum of the active sets' sizes m */
  int64_t pairs;          /* sum of m * n_total */
  int64_t floor_hits;     /* bodies clamped to the deepest level, begin's included */
  int32_t level_min, level_max;   /* over the bodies, now */
} nbody_hermite_block_stats;      /* 64 bytes */
NBODY_AMD_API int nbody_hermite_block_level(double dt_c, double dt_max, int32_t levels, int32_t *floor_hit);
NBODY_AMD_API int nbody_hermite_block_begin(nbody_ctx *ctx, double dt_max, int32_t levels, double eta, double eta_start,
                                            const int32_t *level_in);
NBODY_AMD_API int nbody_hermite_block_advance(nbody_ctx *ctx, int64_t frames, int64_t max_block_steps, nbody_hermite_block_stats *out);
NBODY_AMD_API int nbody_hermite_block_get(nbody_ctx *ctx, int64_t *ticks, int32_t *level);

/*
 * The snap s = d^2 a / dt^2 and sixth-order Hermite stepping (build-defined: the reference computes neither) — Nitadori & Makino's
 * shared-step P(EC) scheme.  It still costs ONE O(N^2) pass per step, and buys a given accuracy with fewer of them: on the two-body
 * orbits of DESIGN 4.13 halving dt divides the error by 64, and the e = 0.9 orbit closes to 2.8e-4 of the semi-major axis in 70 adaptive
 * steps where nbody_hermite_advance needs 242.
 *
 * The snap pass.  With d = x_j - x_i, w = v_j - v_i, b = acc_j - acc_i — acc a per-body INPUT acceleration array —, s^2 = |d|^2 + eps^2,
 * t = 1 / s, al = (d . w) t^2, be = (w . w + d . b) t^2 + al^2, summed over the other bodies j:
 *     A_ij = G m_j d t^3      J_ij = G m_j w t^3 - 3 al A_ij      S_ij = G m_j b t^3 - 6 al J_ij - 3 be A_ij
 * The chunks, the fp64 root and the zero rule are nbody_get_jerk_f64's — t = 0 where s^2 == 0 and for j == i BY INDEX, so a dropped pair
 * adds exactly 0 to all nine sums; with eps > 0 another body on the same point adds G m t^3 w to the jerk and G m t^3 b to the snap — and so
 * are the per-pair operations up to A and J.  The a and j of a snap pass therefore equal nbody_get_jerk_f64's IN EVERY BIT, whatever the
 * input accelerations.  Then, per pair, g_a = fma(-3 be, d_a, fma(2 k3, u_a, b_a)) with the jerk's k3 = -3 al and u_a = fma(k3, d_a, w_a),
 * and S_a = fma(q, g_a, S_a): one fused chain per sum and chunk in body order, the chunks added from 0.0 in chunk order.
 *
 * nbody_get_snap_f64: every body's a, j and s.  Contexts: NBODY_PREC_F64, one device, owning all bodies; NBODY_PREC_F32,
 *   NBODY_PREC_F32_KAHAN, slice and nbody_create_multi contexts report NBODY_ERR_UNSUPPORTED with a message that says why; no particles
 *   set: NBODY_ERR_STATE.  acc_in: n_total x 3 doubles, acc_in_stride >= 24 bytes apart.  acc_in == NULL: the library first runs the fp64
 *   jerk pass on the live state and feeds its UNROUNDED accelerations (two passes under NBODY_KERNEL_FORCES) — the result is then the
 *   physical snap of the current state.  acc, jerk, snap: n_total x 3 doubles each, strides >= 24; any may be NULL, not all three; that,
 *   and a stride too small, is NBODY_ERR_INVALID.  Synchronises; changes nothing a getter shows and leaves both Hermite caches alone.
 *
 * Sixth-order stepping.  Contexts, the "stored (x, v) are SYNCHRONISED" rule and NBODY_ERR_STATE for a pending nbody_step_begin are
 * nbody_hermite_step's.  One step of length dt, per component, every bracket ONE correctly rounded fp64 operation in the order written
 * (contraction off); the constants are the host's doubles — d2 = dt dt, c2 = d2 0.5, c3 = (d2 dt) / 6, c4 = (d2 d2) / 24,
 * c5 = ((d2 d2) dt) / 120, ch = dt 0.5, c10 = d2 / 10, c120 = (d2 dt) / 120, d3 = d2 dt, d4 = d2 d2, d5 = d4 dt:
 *   predict    xp = ((((x + dt v) + c2 a0) + c3 j0) + c4 s0) + c5 a3                  (xp carries the mass)
 *              vp = (((v + dt a0) + c2 j0) + c3 s0) + c4 a3                           (vp.w = 0)
 *              ap = ((a0 + dt j0) + c2 s0) + c3 a3
 *   evaluate   (a1, j1, s1) = what nbody_get_snap_f64 returns on a context holding (xp, vp) given acc_in = ap: the same kernel, fold
 *              and geometry
 *   correct    v1 = v + ((ch (a0 + a1) + c10 (j0 - j1)) + c120 (s0 + s1))
 *              x1 = x + ((ch (v + v1) + c10 (a0 - a1)) + c120 (j0 + j1))
 *              R1 = ((a1 - a0) - dt j0) - c2 s0;   R2 = dt ((j1 - j0) - dt s0);   R3 = d2 (s1 - s0)
 *              X = ((60 R1) - (24 R2)) + (3 R3);   Y = ((168 R2) - (360 R1)) - (24 R3);   Z = ((720 R1) - (360 R2)) + (60 R3)
 *              a3' = ((X + Y) + 0.5 Z) / d3;   a4' = (Y + Z) / d4;   a5' = Z / d5
 *   store      x := x1, v := v1 (masses and the velocities' fourth component stay), NBODY_BUF_ACC := (a1, 0)
 *   cache      (a0, j0, s0) := (a1, j1, s1), a3 := a3', a4 := a4', a5 := a5'
 * X, Y, Z are dt^3, dt^4, dt^5 times the third to fifth derivative of a at the step's start, from the quintic through both ends; a3', a4',
 * a5' are the derivatives at its end.
 *
 * The cache — a0, j0, s0, a3, a4, a5 and whether they belong to the stored state — is a cache of its OWN beside the fourth-order one, on
 * the device, allocated at first use, NOT part of a checkpoint.  At a start (the cache invalid) one jerk pass gives a and one snap pass
 * with that a as its input gives (a0, j0, s0): two passes under NBODY_KERNEL_FORCES; a3, a4, a5 read as zeros until a step has been
 * taken.  A step thereafter costs ONE snap pass; predictor and corrector together count as one pass under NBODY_KERNEL_UPDATE.
 * Everything that invalidates the fourth-order cache (the list above) invalidates this one, nbody_hermite_restart forgets both, and the
 * bound-buffer / handed-out-pointer rule is the same: every CALL evaluates anew at entry.  The two schemes forget each other's cache: a
 * sixth-order step invalidates the fourth-order cache and ends a block session at a frame end — on a session in mid-frame
 * nbody_hermite6_step / _timescale / _advance report NBODY_ERR_STATE with a message that says why —, and nbody_hermite_step,
 * nbody_hermite_advance and nbody_hermite_block_begin invalidate the sixth-order cache.  Checkpoints stay NBDYCKP2 byte for byte:
 * "nbody_save_checkpoint, nbody_hermite_restart, go on" equals "load, go on" in every byte.
 *
 * nbody_hermite6_step: nsteps steps of length dt; steps_done grows by nsteps.  Asynchronous like nbody_step.  dt <= 0 is a no-op that
 *   returns NBODY_OK; a dt that is not finite or nsteps < 0 is NBODY_ERR_INVALID.
 * nbody_hermite6_timescale: norms are sqrt((x x + y y) + z z), contraction off.  With derivatives *kind = 1, Nitadori & Makino's
 *   generalisation of Aarseth's criterion: k_i = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2), 0 / 0 counting as 0, x / 0 as +inf and a
 *   value that is not finite as +inf; the largest k and the lowest index that attains it come from nbody_jerk_time's fixed-order
 *   reduction (no atomics); *t_min = 1.0 / cbrt(sqrt(max k)) on the host.  Without, *kind = 0: nbody_jerk_time's value and body from the
 *   cached (a0, j0).  In both kinds a maximum of 0 gives +inf and one that is not finite 0.  Synchronises; changes nothing a getter
 *   shows.  Any output may be NULL, not all three (NBODY_ERR_INVALID).
 * nbody_hermite6_advance: nbody_hermite_advance's loop and rules with dt = min(dt_max, kind == 1 ? eta t : eta_start t).  NOTE: eta
 *   multiplies t DIRECTLY here — there is no square root, following Nitadori & Makino's convention (t already carries the sixth root) —,
 *   so sensible values are 0.1 .. 1 where nbody_hermite_advance takes 0.01 .. 0.04.  The host reads 16 bytes per step.  *t_done == t_span
 *   exactly at the end; a chosen dt that is 0 or not finite stops the call with NBODY_ERR_STATE and a message that names the body.
 * nbody_hermite6_get: the cache, 18 doubles per body — a0, j0, s0, a3, a4, a5 —, `stride` bytes apart (>= 144, else NBODY_ERR_INVALID).
 *   NBODY_ERR_STATE while (a0, j0, s0) are invalid; a3, a4, a5 read as zeros while there are no derivatives.  Synchronises.
 */
NBODY_AMD_API int nbody_get_snap_f64(nbody_ctx *ctx, const double *acc_in, size_t acc_in_stride, double *acc, size_t acc_stride,
                                     double *jerk, size_t jerk_stride, double *snap, size_t snap_stride);
NBODY_AMD_API int nbody_hermite6_step(nbody_ctx *ctx, double dt, int32_t nsteps);
NBODY_AMD_API int nbody_hermite6_timescale(nbody_ctx *ctx, double *t_min, int32_t *body, int32_t *kind);
NBODY_AMD_API int nbody_hermite6_advance(nbody_ctx *ctx, double t_span, double eta, double eta_start, double dt_max, int64_t max_steps,
                                         double *t_done, int64_t *steps);
NBODY_AMD_API int nbody_hermite6_get(nbody_ctx *ctx, double *d18, size_t stride);

/* Sixth-order Hermite BLOCK time steps (build-defined) — Nitadori & Makino's scheme with a step per body: the sixth-order predictor,
 * snap evaluation and corrector above inside the ticks, levels, frames and sessions of nbody_hermite_block_*.  Where: the contexts that
 * answer nbody_hermite6_step (NBODY_PREC_F64, one device, all bodies); fp32 and Kahan contexts, slice contexts and nbody_create_multi
 * contexts report NBODY_ERR_UNSUPPORTED with that call's reasons.  No particles set: NBODY_ERR_STATE.
 *
 * Time, ticks, levels, frames and the ragged-state rule are those of the fourth-order block steps, word for word: tick =
 * ldexp(dt_max, -levels), 0 <= levels <= 40, body i at T_i (int64 ticks) with level k_i whose step is dt_max 2^-k_i, T_i always a multiple
 * of that step, every multiple of 2^levels ticks a FRAME end where the stored state is synchronised.  (x_i, v_i) AT T_i are in the state
 * buffers, (a0, j0, s0, a3, a4, a5)_i at T_i in the sixth-order cache: the session lives on THAT cache, a session of its own beside the
 * fourth-order one.  nbody_hermite_block_stats is reused as it is.
 *
 * One block step — every bracket ONE correctly rounded fp64 operation, contraction off:
 *   schedule   T_next = min_i (T_i + step_i); the active set = the bodies that attain it, ascending body index, no atomics
 *   predict    EVERY body: dt_i = (double)(T_next - T_i) * tick; on the device d2 = dt_i dt_i, c2 = d2 0.5, c3 = (d2 dt_i) / 6,
 *              c4 = (d2 d2) / 24, c5 = ((d2 d2) dt_i) / 120; then the sixth-order predictor above for xp, vp, ap with these constants
 *   evaluate   (a1, j1, s1) of the ACTIVE bodies against all N predicted bodies with input accelerations ap: for every active body, in
 *              every bit, what nbody_get_snap_f64(acc_in = ap) returns for that body on a context holding (xp, vp)
 *   correct    the active bodies: the chunks' rows added from 0.0 in chunk order, then the sixth-order corrector above with the body's own
 *              dt_i (d2 = dt_i dt_i, d4 = d2 d2, ch = dt_i 0.5, c2 = d2 0.5, c10 = d2 / 10, c120 = (d2 dt_i) / 120, d3 = d2 dt_i,
 *              d5 = d4 dt_i, formed on the device); x, v, NBODY_BUF_ACC := (a1, 0), (a0, j0, s0) := (a1, j1, s1), a3, a4, a5,
 *              T_i := T_next.  Inactive bodies keep every byte.
 *   levels     kk = nbody_hermite6_timescale's per-body k = (|a3| |a5| + |a4|^2) / (|a0| |s0| + |j0|^2) of the NEW vectors, with its
 *              0 / 0 -> 0, x / 0 -> +inf, not finite -> +inf rules; kw = nbody_hermite6_block_level(kk, dt_max, levels, eta, &hit);
 *              then the fourth-order block steps' rule: kw > k_i: k_i := kw; kw < k_i and T_next a multiple of 2^(levels - k_i + 1):
 *              k_i := k_i - 1; otherwise k_i stays.
 * nbody_steps_done grows by one per block step; a block step is one pass under NBODY_KERNEL_FORCES and one under NBODY_KERNEL_UPDATE.
 * The host reads 16 bytes per block step.
 *
 * nbody_hermite6_block_level (host only, no context): THE LEVEL RULE HAS NO CUBE ROOT.  The step the criterion asks for is
 *   eta kk^(-1/6); nbody_hermite6_timescale forms 1 / cbrt(sqrt(k)) on the host, and cbrt is not correctly rounded, so a device and numpy
 *   could not agree on it in every bit.  The rule compares in the cubed domain instead: r = sqrt(kk), e3 = (eta eta) eta, and the level is
 *   the smallest k in 0 .. levels with ((h h) h) r <= e3, h = ldexp(dt_max, -k).  h^3 shrinks by exactly 2^-3 per level while normal, so the
 *   test is monotone in k; kk == 0 gives level 0; kk = +inf or NaN makes every comparison false.  If no k passes it returns `levels` and
 *   *floor_hit = 1 (clamped and counted), otherwise *floor_hit = 0 (floor_hit may be NULL).  levels outside 0 .. 40: -1.  NOTE: eta
 *   multiplies the sixth-root time scale DIRECTLY, as in nbody_hermite6_advance: 0.3 .. 1 here plays the part that 0.01 .. 0.04 plays in
 *   nbody_hermite_block_begin.
 * nbody_hermite6_block_begin: starts a session at tick 0 from the stored (x, v), taken as synchronised.  (a0, j0, s0) come from the
 *   sixth-order cache where it is valid (its a3, a4, a5 too, if a step left them) and otherwise from nbody_hermite6_step's start: a jerk
 *   pass, then a snap pass with that a — two passes under NBODY_KERNEL_FORCES; a3, a4, a5 then read as zeros until a body has stepped.
 *   level_in, if not NULL: n_total levels, each 0 .. levels (else NBODY_ERR_INVALID).  NULL: nbody_hermite_block_begin's start rule on
 *   the cached (a0, j0): k = |j|^2 / |a|^2, t = 1 / sqrt(k) with the same zero and not-finite rules, dt_c = eta_start * t, level =
 *   nbody_hermite_block_level(dt_c, ...) (a body no level fits is a floor hit).  dt_max, eta and eta_start must be finite and > 0,
 *   levels 0 .. 40, the tick AND (tick tick) tick normal doubles (the level rule cubes the step): anything else is NBODY_ERR_INVALID.
 *   NBODY_HERMITE6_BLOCK_LANES=1|2, read here, forces the bodies per lane of the evaluation (otherwise one up to 1024 active bodies, two
 *   beyond); neither choice enters any sum.  Synchronises.
 * nbody_hermite6_block_advance, nbody_hermite6_block_get: nbody_hermite_block_advance's and _get's semantics and error codes.
 *
 * What ends a session: everything that invalidates the sixth-order cache (uploads, nbody_step / nbody_tick / nbody_step_end with dt > 0,
 * nbody_bind_device_state, nbody_device_ptr, checkpoints loaded) and nbody_hermite_restart.  While a session is IN MID-FRAME,
 * nbody_hermite6_step / _timescale / _advance, nbody_hermite_step / _timescale / _advance, nbody_hermite_block_begin and a second
 * nbody_hermite6_block_begin report NBODY_ERR_STATE with a message that says why; AT A FRAME END they end the session and proceed as
 * they always do — the sixth-order ones from the cache, the fourth-order ones invalidating it.  nbody_hermite6_block_begin meets a
 * fourth-order block session the same way: NBODY_ERR_STATE in mid-frame, at a frame end that session ends.  nbody_hermite6_get works
 * during a session: a row belongs to its own T_i.  nbody_get_snap_f64 and nbody_get_jerk_f64 leave the session alone.  Checkpoints stay
 * NBDYCKP2 byte for byte and hold no levels: "save, nbody_hermite_restart, begin with the levels of nbody_hermite6_block_get, go on"
 * equals "load, begin with those levels, go on" in every byte.
 */
NBODY_AMD_API int nbody_hermite6_block_level(double k, double dt_max, int32_t levels, double eta, int32_t *floor_hit);
NBODY_AMD_API int nbody_hermite6_block_begin(nbody_ctx *ctx, double dt_max, int32_t levels, double eta, double eta_start,
                                             const int32_t *level_in);
NBODY_AMD_API int nbody_hermite6_block_advance(nbody_ctx *ctx, int64_t frames, int64_t max_block_steps, nbody_hermite_block_stats *out);
NBODY_AMD_API int nbody_hermite6_block_get(nbody_ctx *ctx, int64_t *ticks, int32_t *level);

/*
 * fp64 point queries and fp64 TRACERS on the shared-step Hermite calls (build-defined: the reference has neither) — what nbody_jerk_at and
 * nbody_set_tracers are to fp32 contexts, for the contexts that answer nbody_hermite_step: NBODY_PREC_F64, one device, owning all bodies.
 * NBODY_PREC_F32, NBODY_PREC_F32_KAHAN, slice and nbody_create_multi contexts report NBODY_ERR_UNSUPPORTED with a message that says why;
 * no particles set, or a pending nbody_step_begin: NBODY_ERR_STATE.  nbody_field_at, nbody_potential_at, nbody_tidal_at, nbody_jerk_at,
 * nbody_set_tracers and nbody_get_tracers stay what they were: fp32 only.
 *
 * The pair form.  A point at x moving with v (and, for the snap, with an INPUT acceleration acc) against ALL bodies j: d = x_j - x,
 * w = v_j - v, b = acc_j - acc, s^2 = |d|^2 + eps^2, t = 1 / s — and then nbody_get_jerk_f64's and nbody_get_snap_f64's per-pair
 * operations in their order, over their chunks (a function of n_total alone) and tiles, the chunks' rows added from 0.0 in chunk order:
 *     A = G m_j d t^3      J = G m_j w t^3 - 3 al A      S = G m_j b t^3 - 6 al J - 3 be A      (al, be: as above)
 * The ONE difference to the bodies' passes: NO pair is dropped by index.  The d == 0 rule is t = (s^2 > 0) ? 1 / s : 0 — with eps == 0 a
 * point exactly on a body drops that pair from every sum; with eps > 0 that pair adds G m w / eps^3 to the jerk, G m b / eps^3 to the snap
 * and nothing to a (what nbody_get_snap_f64 documents for coincident bodies).  A point's sums depend on the point and the bodies ALONE —
 * not on n, the other points, the slab of the staging area the point falls into, the points per lane or the device; a body of mass 0
 * adds exactly nothing.  So a body asked about at its own (x, v) gets nbody_get_jerk_f64's row IN EVERY BIT, and N bodies with M tracers
 * equal, in every bit, a context that holds the tracers as M bodies of mass 0 appended behind them (while both have 256-body chunks:
 * N + M <= 32768) — at N^2 + M N pairs a pass instead of (N + M)^2, and without the tracers entering the shared step.
 *
 * nbody_jerk_at_f64: a and j at n moving points from the LIVE (positions, velocities), unrounded fp64 sums.  pos, vel: 3 doubles per
 *   point, strides >= 24 bytes; vel == NULL: at rest (the bits an array of zeros gives).  acc, jerk: 3 doubles per point, strides >= 24;
 *   either may be NULL, not both.  n == 0: a no-op.  NULL pos, n < 0 or a stride too small: NBODY_ERR_INVALID.  Synchronises; changes
 *   nothing a getter shows, leaves both Hermite caches and any block session alone; ONE pass under NBODY_KERNEL_FORCES.
 *
 * Tracers.  nbody_set_tracers_f64 replaces any earlier set (vel == NULL: at rest; n == 0 removes them; pos / vel as above); uploads keep
 * the tracers, checkpoints do NOT store them (NBDYCKP2 stays byte for byte); nbody_get_tracers_f64 (either array may be NULL) followed by
 * nbody_set_tracers_f64 restores them bit for bit.  Tracers never act on bodies or on each other: a context with tracers advances its
 * bodies BYTE FOR BYTE as the same context without them — positions, velocities, accelerations, both caches, nbody_hermite_timescale
 * and the dt nbody_hermite_advance picks.  They do NOT enter the shared step: a host that wants them to limit it reads
 * nbody_hermite[6]_tracers_timescale and caps dt_max itself.
 * ONLY nbody_hermite_step, nbody_hermite_advance, nbody_hermite6_step and nbody_hermite6_advance advance the fp64 tracers.  nbody_step,
 * nbody_tick, nbody_step_begin / _end and nbody_compute_forces leave their state untouched (and, moving the bodies, invalidate their
 * caches with the bodies').
 *
 * Fourth order, inside every step of nbody_hermite_step / nbody_hermite_advance — the tracers keep a cache (a0, j0, a2, a3) of their own:
 *   predict    the step's dt and nbody_hermite_step's predictor on the tracers' (x, v, a0, j0)
 *   evaluate   (a1, j1) of the predicted tracers against the bodies' PREDICTED (xp, vp) — the field the bodies' own evaluation uses
 *   correct    nbody_hermite_step's corrector, every bracket one correctly rounded operation in its written order
 *   entry      while the tracers' cache is invalid a call first evaluates (a0, j0) of the stored tracers against the stored bodies: one
 *              pass more; a2 and a3 then read as zeros
 * Sixth order, the same inside nbody_hermite6_step / _advance with a cache (a0, j0, s0, a3, a4, a5):
 *   start      behind the bodies' own start, a point jerk pass gives the tracers' a, and ONE point snap pass with that a and the bodies'
 *              cached a0 as its inputs gives the tracers' (a0, j0, s0): two passes more
 *   step       the sixth-order predictor gives the tracers' own ap; one point snap pass against the bodies' (xp, vp, ap); the corrector
 * Invalidation.  Whatever invalidates the bodies' cache of an order invalidates the tracers' cache of that order (the lists above, the
 * other order's steps included); nbody_set_tracers_f64 invalidates BOTH tracer caches and only those; nbody_hermite_restart forgets all
 * four; after nbody_bind_device_state or nbody_device_ptr every call evaluates the tracers anew at entry, as it does the bodies.
 * Timers.  Every tracer evaluation is ONE MORE pass under NBODY_KERNEL_FORCES; the tracers' predictor and corrector add their time to
 * the step's one pass under NBODY_KERNEL_UPDATE.  Without tracers every count is what it was.
 *
 * nbody_hermite_tracers_get / nbody_hermite6_tracers_get: the tracers' cache — 12 doubles (a0, j0, a2, a3; stride >= 96) / 18 doubles
 *   (a0, j0, s0, a3, a4, a5; stride >= 144) per tracer, else NBODY_ERR_INVALID.  No tracers: a no-op.  NBODY_ERR_STATE while the tracers'
 *   (a0, j0[, s0]) are invalid; the derivatives read as zeros until a step has been taken.  Synchronises.
 * nbody_hermite_tracers_timescale / nbody_hermite6_tracers_timescale: nbody_hermite_timescale's / nbody_hermite6_timescale's criterion,
 *   rules and fixed-order reduction over the TRACERS, by the same kernels: *kind = 1 from the derivatives; *kind = 0 |a| / |j| from
 *   (a0, j0), which the call evaluates first if they are invalid.  *tracer: the lowest index that attains the maximum.  No tracers:
 *   NBODY_ERR_STATE.  Any output may be NULL, not all three.  Synchronises; changes no position, velocity or acceleration of a body or
 *   a tracer.  What it does change is the CACHES: it fills the tracers' cache of its order where that was invalid (one / two passes
 *   under NBODY_KERNEL_FORCES; nbody_hermite[6]_tracers_get succeeds afterwards), and the SIXTH-order call, whose tracer start reads
 *   the bodies' a0, first fills the bodies' sixth-order cache like nbody_hermite6_timescale does where that is invalid: two more passes
 *   under NBODY_KERNEL_FORCES, the allocations of a first sixth-order call, and nbody_hermite6_get succeeds afterwards where it would
 *   have reported NBODY_ERR_STATE.  The fourth-order call needs and touches nothing of the bodies' caches.
 *
 * Block sessions and fp64 tracers.  nbody_hermite_block_begin and nbody_hermite6_block_begin still report NBODY_ERR_UNSUPPORTED on a
 * context that holds some — nbody_set_tracers_f64(ctx, NULL, 0, NULL, 0, 0) removes them, nbody_hermite[6]_block_begin_tracers starts a
 * session that CARRIES them —, and nbody_set_tracers_f64 with n > 0 reports NBODY_ERR_STATE while a block session of either order is
 * active.
 *
 * nbody_hermite_block_begin_tracers / nbody_hermite6_block_begin_tracers: the plain begin of the order — its argument rules, contexts
 *   and error codes — for a context that may hold fp64 tracers.  WITHOUT tracers it IS the plain begin, every byte and every launch
 *   (a non-NULL tracer_level_in is then NBODY_ERR_INVALID).  WITH tracers it applies the plain begin's rules to the bodies, fills the
 *   tracers' cache of its order where that is invalid (one pass under NBODY_KERNEL_FORCES more in fourth order, two in sixth, behind the
 *   bodies' own start; the higher derivatives then read as zeros), sets every tracer's T := 0 and takes the tracers' levels from
 *   tracer_level_in: nbody_tracer_count_f64 values, each 0 .. levels (else NBODY_ERR_INVALID, the message names the index).  NULL: the
 *   bodies' start rule on the tracer's own (a0, j0): k = |j|^2 / |a|^2, dt_c = eta_start t, nbody_hermite_block_level(dt_c, ...); a
 *   tracer that no level fits is a TRACER floor hit.
 * One block step of a session that carries tracers — the joint schedule:
 *   schedule   T_next = min over bodies AND tracers of T + step.  Two active lists, each in ascending index: the m_b bodies and the m_t
 *              tracers that attain T_next; m_b + m_t >= 1, either may be 0.  EVERY body and EVERY tracer is predicted to T_next with its
 *              own dt_i = (double)(T_next - T_i) tick by the order's block predictor.
 *   bodies     the active bodies are evaluated against all N predicted bodies and corrected, exactly as without tracers.
 *   tracers    the active tracers are evaluated against all N PREDICTED bodies — fourth order: (xp, vp); sixth: (xp, vp, ap), with the
 *              tracer's own predicted ap as its input acceleration — by the point forms of the jerk / snap pass, and corrected by the
 *              order's block corrector with the tracer's own dt_i: T_i := T_next, the same level rule, one level up at most and only
 *              when aligned.  Inactive tracers and inactive bodies keep every byte.
 *   A tracer's result depends neither on other tracers, nor on its place in the list, nor on M, the slab or the points per lane
 *   (NBODY_HERMITE_BLOCK_LANES / NBODY_HERMITE6_BLOCK_LANES govern the tracers' evaluation too), and the bodies advance BYTE FOR BYTE
 *   as in the same session without tracers.  N bodies with M tracers equal, in every byte after every block step, a context that holds
 *   the tracers as M bodies of mass 0 behind the bodies in a plain session with level_in = the bodies' levels followed by the tracers'
 *   (N + M <= 32768) — at (m_b + m_t) N pairs a block step instead of (m_b + m_t) (N + M).
 *   nbody_steps_done and nbody_hermite_block_stats.block_steps grow by one per block step, tracer-only ones included; body_steps, pairs,
 *   floor_hits and level_min / level_max of nbody_hermite_block_stats stay the BODIES' alone.  A block step is one pass under
 *   NBODY_KERNEL_UPDATE and one under NBODY_KERNEL_FORCES per non-empty evaluation: one or two.  The host waits once per block step and
 *   reads 32 bytes.
 * nbody_hermite_block_tracers_get / nbody_hermite6_block_tracers_get: T_i and k_i of the tracers the session carries and their totals
 *   since begin (set stats->struct_size = sizeof(nbody_hermite_block_tracer_stats) first, another size is NBODY_ERR_INVALID); any of the
 *   three outputs may be NULL, not all three.  A session without tracers: carried = 0, nothing else written.  No session of that order:
 *   NBODY_ERR_STATE.  Synchronises.
 * Sessions.  At a frame end every tracer is at the frame end too; once a whole frame has passed the tracers' cache has its higher
 *   derivatives, like the bodies'.  Shared-step calls at a frame end end the session and go on from both caches, carrying the tracers as
 *   they always do; in mid-frame they report NBODY_ERR_STATE, and nbody_hermite[6]_tracers_timescale follows nbody_hermite[6]_timescale's
 *   rule there.  nbody_hermite[6]_tracers_get and nbody_get_tracers_f64 work during a session: a row belongs to its tracer's own T_i,
 *   the state is ragged in mid-frame.  nbody_set_tracers_f64 with ANY n, 0 included, reports NBODY_ERR_STATE while a session that
 *   carries tracers is active (nbody_hermite_restart ends it first).  Whatever ends a plain session ends a carrying one.  Checkpoints
 *   stay NBDYCKP2 byte for byte: "save, nbody_hermite_restart, begin_tracers with the levels of _block_get and _block_tracers_get, go on"
 *   on the writing context equals, in every byte, "load, nbody_set_tracers_f64 with what nbody_get_tracers_f64 gave, the same begin, go
 *   on" on a fresh one.
 */
NBODY_AMD_API int nbody_jerk_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n,
                                    double *acc, size_t acc_stride, double *jerk, size_t jerk_stride);
NBODY_AMD_API int nbody_set_tracers_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n);
NBODY_AMD_API int nbody_get_tracers_f64(nbody_ctx *ctx, double *pos, size_t pos_stride, double *vel, size_t vel_stride);
NBODY_AMD_API int nbody_tracer_count_f64(nbody_ctx *ctx, int32_t *n);
typedef struct nbody_hermite_block_tracer_stats {
  uint32_t struct_size;        /* caller sets sizeof(nbody_hermite_block_tracer_stats) before the call */
  int32_t carried;             /* tracers the session carries (0: a session without tracers) */
  int64_t tracer_steps;        /* sum over block steps of m_t, the active tracers */
  int64_t pairs;               /* sum of m_t * n_total */
  int64_t tracer_only_steps;   /* block steps in which no BODY was due */
  int64_t floor_hits;          /* tracers clamped to the deepest level, begin's included */
  int32_t level_min, level_max;   /* over the tracers, now (0, 0 when carried == 0) */
} nbody_hermite_block_tracer_stats;   /* 48 bytes */
NBODY_AMD_API int nbody_hermite_block_begin_tracers(nbody_ctx *ctx, double dt_max, int32_t levels, double eta, double eta_start,
                                                    const int32_t *level_in, const int32_t *tracer_level_in);
NBODY_AMD_API int nbody_hermite6_block_begin_tracers(nbody_ctx *ctx, double dt_max, int32_t levels, double eta, double eta_start,
                                                     const int32_t *level_in, const int32_t *tracer_level_in);
NBODY_AMD_API int nbody_hermite_block_tracers_get(nbody_ctx *ctx, int64_t *ticks, int32_t *level, nbody_hermite_block_tracer_stats *stats);
NBODY_AMD_API int nbody_hermite6_block_tracers_get(nbody_ctx *ctx, int64_t *ticks, int32_t *level, nbody_hermite_block_tracer_stats *stats);
NBODY_AMD_API int nbody_hermite_tracers_get(nbody_ctx *ctx, double *d12, size_t stride);
NBODY_AMD_API int nbody_hermite6_tracers_get(nbody_ctx *ctx, double *d18, size_t stride);
NBODY_AMD_API int nbody_hermite_tracers_timescale(nbody_ctx *ctx, double *t_min, int32_t *tracer, int32_t *kind);
NBODY_AMD_API int nbody_hermite6_tracers_timescale(nbody_ctx *ctx, double *t_min, int32_t *tracer, int32_t *kind);

/*
 * The fp64 POTENTIAL, TIDAL TENSOR and SNAP AT POINTS (build-defined: the reference computes none) — what nbody_potential_at,
 * nbody_get_potentials, nbody_tidal_at, nbody_get_tidal and nbody_tidal_time are to fp32 contexts, for the contexts that answer
 * nbody_jerk_at_f64: NBODY_PREC_F64, one device, owning all bodies (such contexts are at theta == 0).  NBODY_PREC_F32,
 * NBODY_PREC_F32_KAHAN, slice and nbody_create_multi contexts report NBODY_ERR_UNSUPPORTED with a message that names the call and says
 * why; no particles set, or a pending nbody_step_begin: NBODY_ERR_STATE.  The fp32 calls stay exactly what they are, their refusal of
 * fp64 contexts included.  nbody_jerk_at_f64 with vel == NULL already is the fp64 form of nbody_field_at.
 *
 * Definitions.  With d = x_j - x and s^2 = |d|^2 + eps^2, over ALL bodies j of the LIVE positions:
 *     phi(x)  = -sum_j G m_j / s
 *     T_ab(x) =  sum_j G m_j [3 d_a d_b / s^5 - delta_ab / s^3]          six components: xx, yy, zz, xy, xz, yz
 * The pair form.  nbody_get_jerk_f64's chunks (a function of n_total alone), tiles, s^2 = fma(dx, dx, fma(dy, dy, dz dz [+ eps^2]))
 * and 1 / sqrt; then, with contraction off and every bracket one fp64 operation, gm = G m_j,
 *     t2 = t * t;  q = (gm * t) * t2                                     (the jerk's q)
 *     potential:  P = fma(gm, t, P)
 *     tidal:      h = (3.0 * q) * t2;  hx = h * dx;  hy = h * dy;  hz = h * dz
 *                 Sxx = fma(hx, dx, Sxx);  Sxy = fma(hx, dy, Sxy);  Sxz = fma(hx, dz, Sxz)
 *                 Syy = fma(hy, dy, Syy);  Syz = fma(hy, dz, Syz);  Szz = fma(hz, dz, Szz);  Q = Q + q
 * — one chain per sum and chunk, in body order; the chunks' rows are added from 0.0 in chunk order, then phi = -P and T_aa = S_aa - Q,
 * one operation each.  The results are those doubles, unrounded.  (s^-5 is formed: unlike fp32, fp64 has the range for it.)
 * The d == 0 rule.  Point forms (_at): t = (s^2 > 0) ? 1 / s : 0 — NO pair is dropped by index.  Per-body forms (_get_, _time): the
 * body itself is additionally left out BY INDEX.  A pair with t == 0 and a body of mass 0 add exactly nothing.  So
 *   - a point's bits depend on the point and the bodies ALONE: not on n, the other points, the slab of the staging area, the rows per
 *     lane or the device;
 *   - N bodies queried at M points equal, in every bit, rows N .. N + M - 1 of the per-body call on a context that holds the points
 *     appended as bodies of mass 0 (while both have 256-body chunks: N + M <= 32768), at every eps;
 *   - with eps == 0 a body asked about at its own position gets its per-body row in every bit, and a point exactly on a body (or two
 *     coincident bodies) drops that pair from every sum;
 *   - with eps > 0 a point exactly on body i additionally feels -G m_i / eps in phi and -G m_i / eps^3 on the diagonal of T (S gets
 *     exactly 0 from that pair, Q gets q); coincident bodies feel each other the same way.
 *
 * nbody_potential_at_f64 / nbody_tidal_at_f64: phi / T at n points.  pos: 3 doubles per point, stride >= 24 bytes; phi: one double per
 *   point, stride >= 8; t6: six doubles per point, stride >= 48.  n == 0: a no-op.  NULL pointers (NULL pos even with n == 0), n < 0 or
 *   a stride too small: NBODY_ERR_INVALID.
 * nbody_get_potentials_f64 / nbody_get_tidal_f64: every body's phi / T from all OTHER bodies — n_total rows, `stride` bytes apart
 *   (>= 8 / >= 48).  A single body gets 0.
 * nbody_tidal_time_f64: nbody_tidal_time's rule, in every detail, on the unrounded tensors of nbody_get_tidal_f64:
 *   n2 = (Txx^2 + Tyy^2) + Tzz^2 + 2 ((Txy^2 + Txz^2) + Tyz^2) per body, the largest n2 and the lowest body index that attains it from the
 *   same fixed-order reduction; *t_min = 1 / sqrt(sqrt(max n2)), +inf when the maximum is 0 (a single body), 0 when it is not finite.
 *   Either output may be NULL, not both (NBODY_ERR_INVALID).
 * nbody_snap_at_f64: the PHYSICAL a, j and s = d^2 a / dt^2 at n moving points (pos, vel as nbody_jerk_at_f64; vel == NULL: at rest).
 *   Three passes: the bodies' fp64 jerk pass of the live state gives their unrounded accelerations (as nbody_get_snap_f64 with
 *   acc_in == NULL), the point jerk pass gives the points' own, and the point snap pass takes both as its input accelerations (the pair
 *   form of nbody_jerk_at_f64 above).  A body asked about at its own (x, v) gets the row of nbody_get_snap_f64(acc_in = NULL) in every
 *   bit.  acc, jerk, snap: 3 doubles per point, strides >= 24; any may be NULL, not all three.  n == 0, NULL pos, n < 0, short strides:
 *   as nbody_jerk_at_f64.  THREE passes under NBODY_KERNEL_FORCES.
 * Every other call here is ONE pass under NBODY_KERNEL_FORCES.  All six synchronise, read the live buffers, change nothing a getter
 * shows, and leave both Hermite caches, the fp64 tracers and any block session alone.
 */
NBODY_AMD_API int nbody_potential_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, int32_t n, double *phi, size_t phi_stride);
NBODY_AMD_API int nbody_get_potentials_f64(nbody_ctx *ctx, double *phi, size_t stride);
NBODY_AMD_API int nbody_tidal_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, int32_t n, double *t6, size_t t_stride);
NBODY_AMD_API int nbody_get_tidal_f64(nbody_ctx *ctx, double *t6, size_t stride);
NBODY_AMD_API int nbody_tidal_time_f64(nbody_ctx *ctx, double *t_min, int32_t *body);
NBODY_AMD_API int nbody_snap_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n,
                                    double *acc, size_t acc_stride, double *jerk, size_t jerk_stride, double *snap, size_t snap_stride);

/* The fp64 pair census (build-defined: the reference has none): per row the NEAREST body and the most-bound PARTNER, and the closest
 * and the hardest pair of the system — which pairs are close and which are bound, the question a Hermite run starts with (one hard
 * binary sets the shared step and drives block sessions to their level floor).  On the contexts that answer nbody_potential_at_f64;
 * every other kind refuses with that call's refusals (fp32 state, slices, multi-device: NBODY_ERR_UNSUPPORTED; an open step:
 * NBODY_ERR_STATE).  theta plays no part: an argmin over ALL pairs of the LIVE (posm, vel).
 *
 * Definitions.  For a row at (x, v) with mass term g (a body: g = G m_i; a point: g = 0) and body j, contraction off, every bracket
 * one fp64 operation, G m_j formed once per body as in the jerk pass:
 *     d = x_j - x;   d2 = fma(dx, dx, fma(dy, dy, dz dz))                  NEVER softened
 *     s2 = d2 + eps^2 (d2 itself when eps == 0);   t = (s2 > 0 and j is not the row's own body) ? 1 / sqrt(s2) : 0   (the jerk's 1 / sqrt)
 *     w = v_j - v;   w2 = fma(wx, wx, fma(wy, wy, wz wz))
 *     e = fma(-(G m_j + g), t, 0.5 w2)                                     the pair's specific orbital energy under the context's pair law
 *   Nearest: the body j, not the row's own, with the smallest d2 under strict <; the lowest index wins ties.  A coincident body
 *     (d2 == 0) is a neighbour, and the nearest, at every eps.
 *   Partner: the body j, not the row's own, with the smallest e under strict <; the lowest index wins ties.  Its d2 is reported too.
 *   A candidate whose value is NaN is never chosen, and neither is one whose d2 is not finite (+inf or NaN — so a body whose position
 *     is NaN is nobody's partner although its e, with t = 0, is the finite 0.5 w2).  No candidate chosen (N == 1, or none admissible):
 *     index -1, d2 = +inf, e = +inf.
 *   Zero-mass bodies are bodies and count.  Point forms (_at) drop nothing by index: a point exactly on a body gets that body at d2 = 0.
 * e_ij and e_ji, d2_ij and d2_ji come from the same operations on negated operands and are equal in every bit, so "mutual" (index[index[i]]
 * == i) is meaningful.  A row's result depends on the row and the bodies ALONE: not on n, the other rows, the slab of the staging area,
 * the rows per lane or the device.
 *
 * nbody_get_nearest_f64 / nbody_get_partners_f64: every body's row — index, (energy,) d2: contiguous [n_total] arrays; each may be NULL,
 *   not all (NBODY_ERR_INVALID).
 * nbody_nearest_at_f64 / nbody_partner_at_f64: the rows of n points.  pos (vel): 3 doubles per point, stride >= 24 bytes; vel == NULL: at
 *   rest, as nbody_snap_at_f64.  Outputs contiguous [n], each may be NULL, not all.  n == 0: a no-op.  NULL pos, n < 0, a stride too small:
 *   NBODY_ERR_INVALID.
 * nbody_closest_pair_f64 / nbody_hardest_pair_f64: the smallest d2 / e of the per-body pass, reduced on the device in a fixed order; the
 *   lowest row i wins, j is that row's index — so i < j.  -1, -1, +inf (, +inf) when there is none.  Outputs may be NULL, not all.
 * nbody_pair_time_f64: *t_min = sqrt(d2 sqrt(d2) / (G (m_i + m_j))) of the closest pair (i, j), formed on the host from that pair's d2 and
 *   the two masses: the free-fall scale a host compares with dt_max 2^-levels.  +inf for a missing pair or G (m_i + m_j) <= 0.
 * Each per-body or point pass is ONE pass under NBODY_KERNEL_FORCES (the pair calls: one, their reduction is not a pass).  All seven
 * synchronise, read the live buffers, change nothing a getter shows, and leave both Hermite caches, the fp64 tracers and any block
 * session alone — in a mid-frame session the rows describe each body at its own time, as nbody_get_potentials_f64's do.
 */
NBODY_AMD_API int nbody_get_nearest_f64(nbody_ctx *ctx, int32_t *index, double *d2);
NBODY_AMD_API int nbody_nearest_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, int32_t n, int32_t *index, double *d2);
NBODY_AMD_API int nbody_closest_pair_f64(nbody_ctx *ctx, int32_t *i, int32_t *j, double *d2);
NBODY_AMD_API int nbody_get_partners_f64(nbody_ctx *ctx, int32_t *index, double *energy, double *d2);
NBODY_AMD_API int nbody_partner_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, const double *vel, size_t vel_stride, int32_t n,
                                       int32_t *index, double *energy, double *d2);
NBODY_AMD_API int nbody_hardest_pair_f64(nbody_ctx *ctx, int32_t *i, int32_t *j, double *energy, double *d2);
NBODY_AMD_API int nbody_pair_time_f64(nbody_ctx *ctx, double *t_min, int32_t *i, int32_t *j);

/* The fp64 neighbour census (build-defined: the reference has none): per row the k NEAREST bodies, and on top of them every body's local
 * density and the system's density centre and core radius (Casertano & Hut 1985, in NBODY6's convention) — where the cluster is and
 * how concentrated, which the centre of mass (escapers drag it) cannot say.  On the contexts that answer nbody_get_nearest_f64; every
 * other kind refuses with that call's refusals.  An fp64 sibling of the pair census, with its conventions throughout.
 *
 * Lists.  d2 = fma(dx, dx, fma(dy, dy, dz dz)), d = x_j - x, NEVER softened.  A row's list holds the k bodies j, not the row's own, with
 *   the smallest d2, sorted ascending in lexicographic (d2, index) order: strict <, the lowest index wins every tie.  A coincident body
 *   (d2 == 0) is a neighbour and comes first; zero-mass bodies count; a candidate whose d2 is NaN or +inf is never listed.  Slots with
 *   nobody to list (N <= k, or fewer admissible bodies) read index -1, d2 = +inf.  Point forms (_at) drop nothing by index: a point
 *   exactly on a body gets that body at d2 = 0.  The answer for k is, byte for byte, the first k entries of the answer for any larger k,
 *   and k = 1 is nbody_get_nearest_f64 / nbody_nearest_at_f64 in every byte.  A row depends on the row and the bodies ALONE: not on n,
 *   the other rows, the slab of the staging area, the rows per lane, the compiled list width or the device.
 * Density of a body with its k nearest listed (2 <= k), every bracket one correctly rounded fp64 operation:
 *     msum = ((m_1 + m_2) + ...) + m_(k-1)      the raw masses of the k - 1 nearest, in neighbour order
 *     r2 = d2_k;   rho = msum / ((4.0 * M_PI / 3.0) * (r2 * sqrt(r2)))
 *   The k-th neighbour sets the sphere and is left out of the mass, as is the body itself.  The k-th missing (N <= k): rho = 0, r2 = +inf.
 *   A NaN quotient becomes 0; r2 == 0 with msum > 0 gives +inf.
 * Density centre and core radius, with w_i = rho_i where 0 < rho_i < +inf, else 0, summed on the device in a fixed order (no atomics:
 *   the same bits every run):
 *     rho_sum = sum w_i;    centre = (sum w_i x_i) / rho_sum
 *     rho2_sum = sum w_i^2; core_radius = sqrt((sum w_i^2 |x_i - centre|^2) / rho2_sum)
 *   rho_max, densest: the largest w and the lowest body that attains it; used: the bodies with w > 0.  used == 0: centre and
 *   core_radius are NaN, densest -1, rho_max 0, and the call returns NBODY_OK.
 *
 * nbody_get_neighbours_f64: every body's list — index, d2: [n_total x k] each, row-major; either may be NULL, not both.
 * nbody_neighbours_at_f64: the lists of n points.  pos: 3 doubles per point, stride >= 24 bytes.  index, d2: [n x k]; either may be NULL,
 *   not both.  n == 0: a no-op.  NULL pos, n < 0, a stride too small: NBODY_ERR_INVALID.
 * nbody_get_density_f64: rho and rk2 = d2_k per body, [n_total] each; either may be NULL, not both.
 * nbody_density_centre_f64: set out->struct_size = sizeof(nbody_core) first; out == NULL or another size is NBODY_ERR_INVALID.
 * k outside 1 .. NBODY_NEIGHBOURS_MAX (the lists) or 2 .. NBODY_NEIGHBOURS_MAX (the density calls): NBODY_ERR_INVALID.  No particles
 * set: NBODY_ERR_STATE.  Each call is ONE pass under NBODY_KERNEL_FORCES (the reductions are not passes), synchronises, reads the live
 * buffers, changes nothing a getter shows, and leaves both Hermite caches, the fp64 tracers and any block session alone.
 */
#define NBODY_NEIGHBOURS_MAX 8
typedef struct nbody_core {
  uint32_t struct_size;   /* caller sets sizeof(nbody_core) before the call */
  int32_t k;              /* the k the densities were formed with */
  int32_t used;           /* bodies with 0 < rho < +inf */
  int32_t densest;        /* the lowest body with the largest such rho; -1: none */
  double rho_max;         /* that rho; 0: none */
  double centre[3];       /* the density centre; NaN: used == 0 */
  double core_radius;     /* NaN: used == 0 */
  double rho_sum;         /* sum w */
  double rho2_sum;        /* sum w^2 */
} nbody_core;
NBODY_AMD_API int nbody_get_neighbours_f64(nbody_ctx *ctx, int32_t k, int32_t *index, double *d2);
NBODY_AMD_API int nbody_neighbours_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, int32_t n, int32_t k, int32_t *index, double *d2);
NBODY_AMD_API int nbody_get_density_f64(nbody_ctx *ctx, int32_t k, double *rho, double *rk2);
NBODY_AMD_API int nbody_density_centre_f64(nbody_ctx *ctx, int32_t k, nbody_core *out);

/* The fp64 radial census (build-defined: the reference has none): the bodies in radial order about a centre — usually the density centre
 * above —, the cumulative mass in that order, and the LAGRANGIAN RADII read from it: the distance of the body at which the cumulative
 * mass reaches a given fraction of the total, the half-mass radius (f = 0.5) among them.  One sort on the device (eight stable radix
 * passes on the bit patterns of d2) instead of a bisection with nbody_mass_within or a host argsort of the whole state.  On the contexts
 * that answer nbody_get_nearest_f64; every other kind refuses with that call's refusals.  Every line below is reproducible in numpy.
 *
 * d2.  dx = x - centre[0] (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz, contraction off: nbody_mass_within's expression in every
 *   operation.  So for any r the count of nbody_mass_within(centre, r) equals the number of sorted d2 <= r*r, and a row's r2 compares
 *   with that call's threshold exactly.
 * Order.  Ascending in lexicographic (d2, index): the lowest index wins every tie; coincident and zero-mass bodies count.  The finite
 *   d2 come first, then d2 == +inf, then NaN, each group in index order; *n_finite is the number of finite d2.  (The device sorts
 *   key = isnan(d2) ? ~0 : bits(d2): d2 is never negative and never -0, so the bit pattern orders as the value does.)  d2[p] is the
 *   sorted value; a NaN's payload is unspecified.  The order is total, so the answer is unique — np.argsort(d2, kind="stable") on the
 *   finite part — and does not depend on how it was sorted.
 * Cumulative mass — a function of the sorted masses and n_total ALONE: the grid, the device and the run never change its bits.  With
 *   w_p = the raw mass of order[p] where its d2 is finite, else +0.0, in blocks of 256 consecutive positions (p = 256 b + t; the last
 *   block padded with +0.0), every + one correctly rounded fp64 addition:
 *     loc[b][t] = ((w_0 + w_1) + ...) + w_t             left to right inside block b
 *     off[0] = 0.0;   off[b + 1] = off[b] + loc[b][255]
 *     mass_cum[p] = off[b] + loc[b][t]
 *   (numpy: loc = np.cumsum(w.reshape(-1, 256), axis=1); off = np.cumsum(np.concatenate(([0.0], loc[:-1, -1]))); off[:, None] + loc.)
 *   It is non-decreasing for non-negative masses.  total_mass = mass_cum[n_total - 1].
 * Selection.  For each fraction f (finite, 0 < f <= 1): target = f * total_mass (one multiply); p = the FIRST position with
 *   mass_cum[p] >= target, searched linearly, so that negative masses still have an answer; the row is (f, d2[p], sqrt(d2[p]) correctly
 *   rounded, mass_cum[p], order[p], p + 1).  No position qualifies unless total_mass > 0 — not when it is <= 0 or NaN, so not when no d2
 *   is finite —: the row is then (f, NaN, NaN, NaN, -1, 0) and the call still returns NBODY_OK.  A row depends neither on the other
 *   fractions nor on their order.  f = 1 selects the last position that adds mass.
 *
 * nbody_radial_order_f64: order, d2, mass_cum: [n_total] each; n_finite: one value.  Each output may be NULL, not all four.
 * nbody_lagrange_radii_f64: k rows for k fractions, 1 <= k <= NBODY_LAGRANGE_MAX; total_mass may be NULL.
 * NULL centre, fractions or rows, a centre that is not finite, k out of range, a fraction outside (0, 1]: NBODY_ERR_INVALID.  No
 * particles set: NBODY_ERR_STATE.  Both calls read the live buffers and synchronise, change nothing a getter shows, and leave both
 * Hermite caches, the fp64 tracers and any block session of either order alone; tracers are never listed.  This is no pair pass: it is
 * counted neither under NBODY_KERNEL_FORCES nor under NBODY_KERNEL_UPDATE, as nbody_get_moments is not.
 */
#define NBODY_LAGRANGE_MAX 64
typedef struct nbody_lagrange {   /* 40 bytes, one row per fraction */
  double fraction;        /* echoed */
  double r2;              /* d2 of the selected body: exact, compares with nbody_mass_within's threshold */
  double radius;          /* sqrt(r2), correctly rounded */
  double mass;            /* mass_cum at the selected position */
  int32_t body;           /* order[p]; -1: none */
  int32_t count;          /* p + 1; 0: none */
} nbody_lagrange;
NBODY_AMD_API int nbody_radial_order_f64(nbody_ctx *ctx, const double centre[3], int32_t *order, double *d2, double *mass_cum,
                                         int32_t *n_finite);
NBODY_AMD_API int nbody_lagrange_radii_f64(nbody_ctx *ctx, const double centre[3], const double *fractions, int32_t k,
                                           nbody_lagrange *rows, double *total_mass);

/* The fp64 group census (build-defined: the reference has none): how many bodies lie within a distance of each body or point — the
 * radius counts —, and WHICH BODIES BELONG TOGETHER: the connected components of the graph "closer than a linking length", which is
 * friends-of-friends (FoF) — the multiples around the binaries of the pair census, the clumps of a fractal or merging initial condition,
 * a remnant against its tail.  On the contexts that answer nbody_get_nearest_f64 (fp64 state, one device, all bodies, no open step);
 * every other kind refuses with that call's refusals.  theta and eps play no part: nothing is softened.  The calls read the live
 * positions.  Every line below is reproducible in numpy, bit for bit; nothing but `rounds` depends on how it was computed.
 *
 * Distance.  dx = x_j - x_i (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz, contraction off: nbody_mass_within's expression, not the pair
 *   census's fma form.  The threshold is r2 = radius * radius, one fp64 multiply.  d2_ij == d2_ji in every bit (the differences are
 *   exact negations), so the graph is undirected by construction, and nbody_radius_counts_at_f64 at one point c equals the count of
 *   nbody_mass_within(c, radius) exactly.  radius must be finite and >= 0 and r2 finite, else NBODY_ERR_INVALID with nothing written;
 *   radius == 0 links coincident bodies only.
 * Link.  Bodies i != j are linked iff d2 <= r2.  A NaN coordinate gives a NaN d2 and no link: that body is a group of one.  A +inf d2
 *   never passes a finite r2.  A zero-mass body links like any other.
 * Per body.  degree[i] = the number of j != i linked to i;  label[i] = the lowest index among the bodies of i's connected component;
 *   members[i] = the size of that component.
 * Summary.  groups = the number of i with label[i] == i;  multiples = those with members >= 2;  largest = the label of the group with
 *   the most members, the lowest label among ties;  largest_members = its size;  links = sum of degree / 2;  rounds = the N^2 passes
 *   the device took: each round every body learns the smallest label among its linked bodies, the ROOT of its tree is hooked to it by an
 *   integer minimum, and every tree is flattened; the first round that changes nothing is the last and is counted.  rounds <= n_total;
 *   NBODY_ERR_INTERNAL beyond.
 *
 * nbody_get_radius_counts_f64: count[n_total] = degree, one pass.
 * nbody_radius_counts_at_f64: count[n] for n points of three doubles, pos_stride (>= 24) bytes apart; NO body is dropped by index: a
 *   point on a body counts that body.  n == 0: NBODY_OK.
 * nbody_get_groups_f64: label, members, degree: [n_total] each; any output may be NULL, not all four.
 * NULL count or points, n < 0, a stride < 24: NBODY_ERR_INVALID.  No particles set: NBODY_ERR_STATE.  The calls synchronise, change
 * nothing a getter shows, and leave both Hermite caches, the fp64 tracers and any block session of either order alone; nothing is kept
 * per context between calls.  Each N^2 pass counts once under NBODY_KERNEL_FORCES — one for a radius-count call, summary.rounds for a
 * groups call —, nothing under NBODY_KERNEL_UPDATE.
 */
typedef struct nbody_groups {   /* 32 bytes */
  int32_t groups;           /* connected components, singles included */
  int32_t multiples;        /* those of two or more bodies */
  int32_t largest;          /* the label of the group with the most members, the lowest label among ties */
  int32_t largest_members;  /* its size */
  int32_t rounds;           /* N^2 passes taken */
  int32_t reserved;         /* 0 */
  int64_t links;            /* linked pairs: sum of degree / 2 */
} nbody_groups;
NBODY_AMD_API int nbody_get_radius_counts_f64(nbody_ctx *ctx, double radius, int32_t *count);
NBODY_AMD_API int nbody_radius_counts_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, int32_t n, double radius, int32_t *count);
NBODY_AMD_API int nbody_get_groups_f64(nbody_ctx *ctx, double radius, int32_t *label, int32_t *members, int32_t *degree,
                                       nbody_groups *summary);

/* The fp64 separation census (build-defined: the reference has none): HOW MANY PAIRS LIE WITHIN r, AS A FUNCTION OF r — the pair-count
 * function C(r), from which the pair-separation histogram, the DD / DR / RR counts of the two-point correlation function, the correlation
 * dimension d log C / d log r and the radial distribution function are read — at up to NBODY_PAIR_RADII_MAX radii from ONE call, where
 * nbody_get_radius_counts_f64 takes one N^2 pass per radius and leaves the sum to the host.  The pair form of nbody_mass_within.  On the
 * contexts that answer nbody_get_radius_counts_f64 (fp64 state, one device, all bodies, no open step); every other kind refuses with
 * that call's refusals.  theta and eps play no part: nothing is softened.  The calls read the live positions.  Every count is an exact
 * integer, reproducible in numpy; nothing depends on how it was computed.
 *
 * Distance.  dx = x_j - x_i (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz, contraction off: the group census's expression in every
 *   operation, symmetric in every bit.
 * Threshold.  r2 = radii[q] * radii[q], one fp64 multiply.
 * Link.  A pair counts at radius q iff d2 <= r2.  A NaN d2 never counts; a +inf d2 never passes a finite r2.  A zero-mass body counts
 *   like any other.
 * Radii.  1 <= k <= NBODY_PAIR_RADII_MAX; each radius finite and >= 0 with a finite square.  The radii may come in ANY ORDER and WITH
 *   REPEATS; each is answered on its own (equal radii get equal answers), as in nbody_mass_within.
 *
 * nbody_get_pair_counts_f64: count[q] = the number of UNORDERED pairs {i, j}, i != j BY INDEX, with d2 <= r2_q.  Coincident distinct
 *   bodies count at radius 0.  (d2_ij == d2_ji in every bit, so the ordered count is even; this is half of it.)
 * nbody_pair_counts_at_f64: count[q] = the number of (point, body) pairs within radii[q], over n points of three doubles, pos_stride
 *   (>= 24) bytes apart, and all bodies.  NO body is dropped by index: a point on a body counts that body.  n == 0: NBODY_OK, zeros
 *   written.
 * Identities, all exact:  nbody_get_pair_counts_f64's count[q] == nbody_groups.links of nbody_get_groups_f64(radii[q]) == the sum of
 *   nbody_get_radius_counts_f64(radii[q])'s degrees / 2;  nbody_pair_counts_at_f64's count[q] == the sum of
 *   nbody_radius_counts_at_f64(radii[q])'s counts;  with one point c it equals the count of nbody_mass_within(c, radii[q]).
 *
 * NULL radii, count or points, k outside 1 .. NBODY_PAIR_RADII_MAX, a radius that is NaN, negative, infinite or whose square overflows,
 * n < 0, a stride < 24: NBODY_ERR_INVALID.  No particles set: NBODY_ERR_STATE.  Every check runs before anything is written: a refused
 * call leaves count[] untouched.  The calls synchronise, change nothing a getter shows, and leave both Hermite caches, the fp64 tracers
 * and any block session of either order alone; nothing is kept per context between calls.  The distinct r2 among the k radii are
 * answered NBODY_PAIR_RADII_PER_PASS to an N^2 pass: a call takes ceil(k_distinct / NBODY_PAIR_RADII_PER_PASS) passes, each counted
 * once under NBODY_KERNEL_FORCES, nothing under NBODY_KERNEL_UPDATE (nbody_pair_counts_at_f64 with n == 0: none).
 */
#define NBODY_PAIR_RADII_MAX 64
#define NBODY_PAIR_RADII_PER_PASS 16
NBODY_AMD_API int nbody_get_pair_counts_f64(nbody_ctx *ctx, const double *radii, int32_t k, int64_t *count);
NBODY_AMD_API int nbody_pair_counts_at_f64(nbody_ctx *ctx, const double *pos, size_t pos_stride, int32_t n, const double *radii, int32_t k,
                                           int64_t *count);

/* The fp64 minimum spanning tree (build-defined: the reference has none): the Euclidean minimum spanning tree of the bodies — what the
 * mass-segregation ratio, the Q parameter and the single-linkage dendrogram are read from; cutting it at a length gives the
 * friends-of-friends groups at THAT length, at every length from one call.  On the contexts that answer nbody_get_groups_f64 (fp64
 * state, one device, all bodies, no open step); every other kind refuses with that call's refusals.  theta and eps play no part.  The
 * call reads the live positions.  Every line below is reproducible in numpy, bit for bit; nothing but `rounds` depends on how it was
 * computed.
 *
 * Weight.  dx = x_j - x_i (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz, contraction off: the group census's expression, symmetric in
 *   every bit, so that the edges with d2 <= radius * radius connect exactly nbody_get_groups_f64(radius)'s groups.
 * Edges.  The unordered pairs i < j whose d2 is finite.  A NaN or +inf d2 — a coordinate that is not finite, or an overflow between two
 *   finite bodies — is no edge: such bodies end in components of their own, and the result is a minimum spanning FOREST.  A zero-mass
 *   body is a vertex like any other; coincident bodies are joined by edges of d2 = 0.
 * Order.  Edges compare by the key (d2, i, j), i < j, lexicographically: a strict total order, so the forest is UNIQUE — a function of
 *   the positions alone, the same bytes every run.
 * Output.  edges = n_total - components records (i, j, d2), ascending by that key, in i, j, d2: [n_total - 1] each; the entries from
 *   `edges` on read (-1, -1, +inf).  component[n_total] = the lowest index among the bodies of each body's component (the groups' label
 *   convention).
 * Summary.  length = sum of sqrt(d2) over the edges in output order, added left to right from 0.0;  longest_d2 = the last edge's d2, 0.0
 *   with no edge;  rounds = the N^2 passes the device took: Boruvka rounds — every body finds its nearest body in ANOTHER component,
 *   every component keeps the least such edge by the key, the components are merged along them.  The components that still have an
 *   edge at least halve every round: rounds <= ceil(log2 n_total) + 1, NBODY_ERR_INTERNAL beyond.  No pass is made once one component
 *   remains (n_total == 1: 0 rounds); where several remain, one last pass that finds no edge ends the call and is counted.
 *
 * Any output may be NULL, not all five: NBODY_ERR_INVALID.  No particles set: NBODY_ERR_STATE.  The call synchronises, changes nothing
 * a getter shows, and leaves both Hermite caches, the fp64 tracers and any block session of either order alone; nothing is kept per
 * context between calls.  Each pass counts once under NBODY_KERNEL_FORCES, nothing under NBODY_KERNEL_UPDATE.
 */
typedef struct nbody_mst {   /* 32 bytes */
  int32_t edges;            /* n_total - components */
  int32_t components;       /* trees of the forest, singles included */
  int32_t rounds;           /* N^2 passes taken */
  int32_t reserved;         /* 0 */
  double length;            /* sum of sqrt(d2) in output order */
  double longest_d2;        /* d2 of the last edge; 0.0 with no edge */
} nbody_mst;
NBODY_AMD_API int nbody_get_mst_f64(nbody_ctx *ctx, int32_t *i, int32_t *j, double *d2, int32_t *component, nbody_mst *summary);

/* ComputeCubeSize (OctreeSearch.cpp:47-56): max over owned bodies of max(|x|,|y|,|z|). */
NBODY_AMD_API int nbody_get_bounds(nbody_ctx *ctx, float *size);

/* ---- state out ---------------------------------------------------------------------------- */

/* What DrawDebugPoint reads (OctreeSearch.cpp:41): positions of bodies [first, first+count) of the
 * whole system, 3 floats each, `stride` bytes apart (>= 12). */
NBODY_AMD_API int nbody_get_positions(nbody_ctx *ctx, float *xyz, size_t stride, int32_t first, int32_t count);

/* Owned records [i_begin, i_begin+i_count) into aos[0..i_count): Mass, Position, Velocity, Acceleration. */
NBODY_AMD_API int nbody_get_particles(nbody_ctx *ctx, void *aos, size_t stride);

/* One frame of AOctreeSearch::Tick (OctreeSearch.cpp:21-34) with a single host synchronisation: if dt > 0, *size =
 * ComputeCubeSize of the current positions (.cpp:26) and one Tick body (.cpp:27-31); then the owned FParticle records
 * as nbody_get_particles delivers them (what .cpp:33,41 draws).  size and aos may each be NULL.  Same results as
 * nbody_get_bounds + nbody_step(dt, 1) + nbody_get_particles; not for sharded symmetric contexts (phased step).
 * Systems whose step is a kernel or two (theta = 0 up to 16384 bodies) and every theta > 0 frame (its walk) write the records from that
 * kernel straight into page-locked host memory — into `aos` itself when it lies in a range pinned with
 * nbody_pin_host_buffer (stride 40), so that the frame queues no copy of the mirror at all. */
NBODY_AMD_API int nbody_tick(nbody_ctx *ctx, float dt, float *size, void *aos, size_t stride);

/* Renderer hand-off straight into the caller's buffer (what OctreeSearch.cpp:41 reads every frame):
 * page-lock `bytes` of caller memory at `host` for this context.  nbody_get_positions (stride 12) and
 * nbody_get_particles (stride 40) whose destination lies inside a pinned range then DMA into it directly — one copy,
 * device to destination — instead of going through the context's own staging buffer and a host memcpy.  The memory
 * stays the caller's; unpin it (or destroy the context) before freeing it.  Results are identical either way. */
NBODY_AMD_API int nbody_pin_host_buffer(nbody_ctx *ctx, void *host, size_t bytes);
NBODY_AMD_API int nbody_unpin_host_buffer(nbody_ctx *ctx, void *host);

/* Owned bodies, native layout (fp32; converted down from fp64 contexts).  Either pointer may be NULL. */
NBODY_AMD_API int nbody_get_state_soa(nbody_ctx *ctx, float *posm4, float *vel4, float *acc4);
NBODY_AMD_API int nbody_get_state_soa_f64(nbody_ctx *ctx, double *posm4, double *vel4, double *acc4);

/* Kinetic energy of the owned bodies and their share of the potential energy (1/2 m_i phi_i),
 * evaluated in fp64 on the device.  Sum over contexts for the system total.  Build-defined (no
 * reference counterpart). */
NBODY_AMD_API int nbody_energy(nbody_ctx *ctx, double *ke, double *pe);

/*
 * Bulk diagnostics of the owned bodies in one O(N) pass over the state (build-defined: the reference computes none): what a host checks
 * after "does the energy hold", without reading 40 B per body back.  Every context answers: all three precisions, theta == 0 and
 * theta > 0, deep-tree contexts, slice contexts and nbody_create_multi.
 *
 * nbody_get_moments: RAW sums over the owned bodies [i_begin, i_begin + i_count), about the ORIGIN.  Raw sums add: the shares of slice
 *   contexts add field by field to the system's totals, as nbody_energy's shares do, and a multi-device context adds its parts' shares
 *   in part order 0 .. n_dev - 1 in fp64 (n_dev = 1: nbody_create's result, bit for bit).  What is wanted about the centre of mass follows
 *   on the host from the parallel-axis identities — com = mx / mass, v_com = p / mass, L_com = l - com x p,
 *   second_com[ab] = second[ab] - mx[a] mx[b] / mass, kinetic_com = kinetic - p.p / (2 mass), torque_com = torque - com x force —
 *   there are no entry points for them.
 *   Every term is formed in fp64 from the state as it is held — fp32 widened to double on NBODY_PREC_F32 and _F32_KAHAN contexts, the
 *   doubles themselves on NBODY_PREC_F64 — and summed in fp64.  Positions, velocities and accelerations are the ones nbody_get_particles /
 *   nbody_get_state_soa would deliver at that moment: the live buffers, whichever the stepping path has left current, bound buffers
 *   (nbody_bind_device_state) included.  The accelerations are the STORED ones: after nbody_step or nbody_tick that is a(x_n) beside
 *   x_(n+1) — the field the bodies just felt; for the consistent set — virial, force and torque of the current positions — call
 *   nbody_compute_forces first.  force and torque vanish to rounding for a pair sum (theta == 0); at theta > 0 they are what the
 *   reference's monopole walk leaves.  On an unsoftened system (eps == 0) the consistent virial IS the potential energy.
 *   Tracers are never summed.
 *   Reproducibility: per-workgroup sums in fixed slots, folded in a fixed order, no atomics; the launch geometry is a function of i_count
 *   alone (csrc/kernels_moments.hip) — not of the CU count, the precision or the device.  The same context state gives the same bits on
 *   every call and on any part.
 *   The call synchronises and changes nothing any getter shows; its device time is NOT counted under NBODY_KERNEL_FORCES / _UPDATE.
 *   Set out->struct_size = sizeof(nbody_moments) first (as nbody_launch_policy): out == NULL or another size is NBODY_ERR_INVALID; no
 *   particles set NBODY_ERR_STATE.
 *
 * nbody_mass_within: the cumulative mass profile about `centre`.  For each of k radii (1 <= k <= 64, each finite and >= 0, in any order,
 *   each answered on its own): count[q] = number of owned bodies with d2 <= radii[q] * radii[q], mass[q] = the sum of their masses (fp64,
 *   the same fixed order).  d2 is computed in fp64 with contraction off: dx = (double)x - centre[0] (dy, dz alike), d2 = (dx*dx + dy*dy)
 *   + dz*dz; the threshold is one fp64 multiply.  Membership is therefore reproducible in plain C or numpy, and the counts are exact.
 *   A radius' results depend neither on the other radii nor on their order.  Either output may be NULL, not both.  One pass over the
 *   positions answers all k radii; Lagrangian radii (a selection) are nbody_lagrange_radii_f64's on fp64 contexts, with this d2.
 *   Slices, multi-device contexts (counts and masses add in part order), precisions, tracers and side effects: as nbody_get_moments.
 *   NULL centre / radii, k outside 1 .. 64, a negative or non-finite radius: NBODY_ERR_INVALID.
 */
typedef struct nbody_moments {
  uint32_t struct_size;   /* caller sets sizeof(nbody_moments) before the call */
  int32_t  reserved;      /* written 0 */
  int64_t  count;         /* bodies summed: the context's i_count */
  double mass;            /* sum m */
  double mx[3];           /* sum m x                       (centre of mass = mx / mass) */
  double p[3];            /* sum m v                       linear momentum */
  double l[3];            /* sum m (x cross v)             angular momentum about the origin */
  double second[6];       /* sum m (xx, yy, zz, xy, xz, yz)  second moments about the origin */
  double kinetic;         /* sum 1/2 m v.v */
  double virial;          /* sum m (x . a)   a = the STORED accelerations (Clausius) */
  double force[3];        /* sum m a         net force of the last force pass */
  double torque[3];       /* sum m (x cross a) */
} nbody_moments;          /* 16 + 24 * 8 = 208 bytes */
NBODY_AMD_API int nbody_get_moments(nbody_ctx *ctx, nbody_moments *out);
NBODY_AMD_API int nbody_mass_within(nbody_ctx *ctx, const double centre[3], const double *radii, int32_t k, double *mass, int64_t *count);

/* ---- device plumbing (torch / RCCL interop) -------------------------------------------------- */

/* Launch on the caller's HIP stream (hipStream_t as void*); NULL = the context's own stream. */
NBODY_AMD_API int nbody_set_stream(nbody_ctx *ctx, void *hip_stream);

/* Raw device pointer of one state buffer (e.g. as the send/recv buffer of an all-gather).  It stays valid, and keeps
 * naming the live buffer, until nbody_destroy or a nbody_bind_device_state of that buffer.  Asking for NBODY_BUF_POSM
 * tells the context that positions may change behind its back: from then on it re-reads them before every force pass
 * (no fused update + preparation, no buffer-swapping one-launch step on systems of up to 16384 bodies) — same results, a
 * little slower. */
NBODY_AMD_API int nbody_device_ptr(nbody_ctx *ctx, int32_t which, void **ptr, size_t *bytes);

/* Use caller-owned device memory for the state (any may be NULL = keep the context's own).
 * Sizes as in NBODY_BUF_*.  The caller keeps them alive until nbody_destroy. */
NBODY_AMD_API int nbody_bind_device_state(nbody_ctx *ctx, void *posm, void *vel, void *acc);

/* Block until everything queued on the context's stream has finished. */
NBODY_AMD_API int nbody_synchronize(nbody_ctx *ctx);

/* Sum of device time (ms) and number of launches of one kernel since the last reset, from HIP
 * events recorded on the launch stream (needs params.time_kernels).  Synchronises. */
NBODY_AMD_API int nbody_kernel_time(nbody_ctx *ctx, int32_t which, double *total_ms, int64_t *launches);
NBODY_AMD_API int nbody_kernel_time_reset(nbody_ctx *ctx);

/* The shader clock the timed force kernels actually ran at since the last nbody_kernel_time_reset, in MHz (needs
 * params.time_kernels): every workgroup of forces_sym_pk_kernel / forces_tile_pk_kernel / forces_sym_f64_kernel reads the
 * shader-clock counter and the fixed reference counter at both ends and the ratio of the sums is reported — the power-limited force
 * loops hold a different clock on different boxes (2.13 - 2.33 GHz seen; the fp64 loop moves it most), and time x clock is what tells
 * a slower box from slower code.  0 when no instrumented kernel has run (the generic scalar, block and Barnes-Hut kernels are not
 * instrumented).  compute_units: of the context's device.
 * A multi-device context reports its slowest device.  Synchronises. */
NBODY_AMD_API int nbody_kernel_clock(nbody_ctx *ctx, double *shader_mhz, int32_t *compute_units);

/* Launch geometry actually chosen (for logs and DESIGN.md tables). */
NBODY_AMD_API int nbody_get_launch_config(nbody_ctx *ctx, int32_t *tile, int32_t *i_per_thread, int32_t *j_split,
                                      int32_t *blocks, int32_t *threads);

/* Name of the force kernel this context launches (for logs and profiles). */
NBODY_AMD_API const char *nbody_force_kernel_name(const nbody_ctx *ctx);

/* NBODY_ALGO_* actually in use, and (symmetric only) the bodies per i-set = per block of the ring, 256 x i_per_thread
 * (the parameter keeps its round-1 name). */
NBODY_AMD_API int nbody_get_algorithm(nbody_ctx *ctx, int32_t *algorithm, int32_t *super_tile);

/* The symmetric pass's partial-sum pool: its size in bytes (0 for the one-sided kernels) and how many phases share its
 * j-side area (1 unless the pool of a one-pass plan would exceed a third of the card: N = 2^23 on one 288 GB card). */
NBODY_AMD_API int nbody_sym_pool_info(nbody_ctx *ctx, uint64_t *pool_bytes, int32_t *phases);

/* Symmetric contexts (fp32, Kahan fp32, fp64): did the last force pass run the equal-mass form of the kernel?  When every
 * body has the same mass (the usual Plummer-sphere set-up) the pair loop sums |d|^-3 d with no mass factor — fp32: 14
 * packed instructions per register pair and step instead of 16; fp64: 20 operations per pair instead of 22 — and the
 * common G m is applied once per body afterwards; same pair law, summation
 * order and d == 0 handling, results equal to the general form's to rounding.  Found out on the device before every
 * pass (from the host's copy when only this library writes the positions), so a mass changed through a bound or
 * handed-out buffer is seen.  *in_use = 0 on every other kind of context.  Synchronises the stream. */
NBODY_AMD_API int nbody_equal_mass_form(nbody_ctx *ctx, int32_t *in_use);

/* Host only (no device needed): the work plan of the symmetric force pass for a context owning [i_begin, i_begin +
 * i_count) of n_total bodies — i-sets of `bodies_per_iset` bodies (256 x i_per_thread) against strips of 64-body
 * subtiles, strip lengths by guided self-scheduling over `slots` resident workgroups (csrc/sym_plan.h).  items, when
 * not NULL, receives 8 int32 per work item: i0, j0, n_sub, flags (1 = the strip lies inside the i-set's own block, 2 = it
 * writes no j-side sums), slot_i, slot_j (element offsets of its partial-sum segments), 0, 0.  own_mode: how own-block strips are
 * costed — 1 = the fp32 kernels (symmetric between register pairs of two slots), 2 = the fp64 kernel (between slots).  Build-defined diagnostics; the CPU tests use it
 * to check that every body pair is evaluated exactly once. */
NBODY_AMD_API int nbody_sym_plan_describe(int32_t n_total, int32_t i_begin, int32_t i_count, int32_t bodies_per_iset,
                                      int32_t slots, int32_t k_guided, int32_t min_sub, int32_t own_mode, int32_t *n_items,
                                      uint64_t *pool_elems, int32_t *items, int32_t items_cap);
/* The same with the strip divisor K given in tenths (the library's own choices include K = 1.5). */
NBODY_AMD_API int nbody_sym_plan_describe_tenths(int32_t n_total, int32_t i_begin, int32_t i_count, int32_t bodies_per_iset,
                                             int32_t slots, int32_t k_guided_x10, int32_t min_sub, int32_t own_mode,
                                             int32_t *n_items, uint64_t *pool_elems, int32_t *items, int32_t items_cap);

/* A plan whose j-side partial-sum segments must share an area of at most j_budget_elems pool elements: the items run in
 * phases (consecutive runs of the launch order), each phase's j-side sums are folded before the next reuses the area — how
 * the library keeps the symmetric pass beyond N = 2^22 on one card.  phases[] receives n_phases + 1 item numbers. */
NBODY_AMD_API int nbody_sym_plan_describe_phased(int32_t n_total, int32_t i_begin, int32_t i_count, int32_t bodies_per_iset,
                                             int32_t slots, int32_t k_guided_x10, int32_t min_sub, uint64_t j_budget_elems,
                                             int32_t *n_items, uint64_t *pool_elems, int32_t *items, int32_t items_cap,
                                             int32_t *n_phases, int32_t *phases, int32_t phases_cap);

/* The even-share plan of the symmetric pass (plain fp32 contexts that own all bodies, mid sizes: csrc/sym_plan.h): exactly
 * n_items_wanted work items (at least one per i-set) of equal cost — a row of the pair matrix, i.e. an i-set against its own
 * block and then its forward blocks in ring order, cut at equal cumulative cost to four steps of a subtile's 64.  items
 * receives 8 int32 per work item: i0, j0 (first subtile; the run goes on in ring order, from the system's last granule to
 * granule 0), n_sub (subtiles touched), flags (4 | 1 if the first subtile lies in the own block), slot_i, slot_j, k0 (first
 * step of the first subtile), k_skip (steps of the last subtile left to the next item). */
NBODY_AMD_API int nbody_sym_plan_describe_even(int32_t n_total, int32_t bodies_per_iset, int32_t n_items_wanted, int32_t *n_items,
                                           uint64_t *pool_elems, int32_t *items, int32_t items_cap);

/* 1 when the context's symmetric pass runs an even-share plan (above), 0 otherwise (guided strips, or not symmetric). */
NBODY_AMD_API int32_t nbody_sym_plan_is_even(const nbody_ctx *ctx);

/* Host only: register pairs of bodies (2 ... 8; two bodies each) a workgroup of forces_block_pk_kernel owns for a plain fp32
 * system of n_total bodies on a device with `compute_units` CUs — the rule of csrc/launch_policy.cpp (smallest ceil(workgroups /
 * CUs) x pairs, larger workgroups on a tie).  No result depends on it; the CPU tests check the rule. */
NBODY_AMD_API int32_t nbody_block_pairs_describe(int32_t n_total, int32_t compute_units);

/* Host only (no device needed): what a context created with these parameters reports on a device with `compute_units` CUs
 * (<= 0: 256) and `device_total_bytes` of memory (0: unknown — no plan is refused for its size).  The launch policy is a function
 * of exactly these inputs (csrc/launch_policy.h), so the CPU tests pin every size threshold through this call.  Set struct_size
 * first.  Returns the code nbody_create would return for these parameters on such a device (NBODY_OK, NBODY_ERR_INVALID,
 * NBODY_ERR_UNSUPPORTED); nbody_last_error(NULL) then gives the same text. */
typedef struct nbody_launch_policy {
    uint32_t struct_size;
    int32_t tile, i_per_thread, j_split, blocks, threads;   /* nbody_get_launch_config */
    int32_t algorithm, super_tile;                          /* nbody_get_algorithm */
    int32_t plan_is_even;                                   /* nbody_sym_plan_is_even */
    int32_t phases;                                         /* nbody_sym_pool_info ... */
    int32_t exchange_ranks;                                 /* nbody_exchange_info: n_ranks */
    int32_t wave;                                           /* block kernels: register pairs (fp32) / bodies per workgroup; 0 otherwise */
    int32_t detector_slots;                                 /* hash slots of the coincident-body detector; 0 = none */
    int32_t sym_slots, sym_min_sub;                         /* symmetric plan: resident workgroups, shortest strip in subtiles ... */
    double sym_k;                                           /* ... and the strip divisor K (0 for an even-share plan) */
    uint64_t pool_bytes;                                    /* ... nbody_sym_pool_info */
    char kernel[64];                                        /* nbody_force_kernel_name */
} nbody_launch_policy;
NBODY_AMD_API int nbody_launch_policy_describe(const nbody_params *p, int32_t compute_units, uint64_t device_total_bytes,
                                               nbody_launch_policy *out);

/* ---- checkpoint / resume (build-defined: the reference keeps its state in a non-serialised TArray) ---------- */

/* Raw little-endian dump of the context's state: header (format NBDYCKP2: sizes, steps, G, eps, theta and — Barnes-Hut —
 * the previous tree's centre of mass, where the reference roots the next tree, OctreeSearch.cpp:77-79), all
 * positions+masses, owned velocities and accelerations.  Resuming from it continues the trajectory bit for bit, at
 * theta = 0 and at theta > 0.  A sharded job writes one file per rank; a multi-device context writes the single file a
 * one-device context of the whole system would. */
NBODY_AMD_API int nbody_save_checkpoint(nbody_ctx *ctx, const char *path);
/* The context must have the same n_total, precision, G and eps as the one that saved the file, and an owned range inside
 * the file's (so a whole-system file also feeds every slice of a sharded or multi-device job).  An fp32 context that
 * owns all bodies also takes over theta and the tree root. */
NBODY_AMD_API int nbody_load_checkpoint(nbody_ctx *ctx, const char *path, int64_t *steps_done);
/* Updates applied since the state was set or loaded. */
NBODY_AMD_API int nbody_steps_done(nbody_ctx *ctx, int64_t *steps);

/* ---- initial conditions (host only; no device needed) ---------------------------------------- */

/*
 * CreateSpacePoints (OctreeSearch.cpp:58-72) with a seeded generator: uniform box
 * (+-size, +-size, +-size/10) about `center`, isotropic velocities of magnitude 250..500, masses
 * 1..5000, body 0 pinned at the origin at rest with mass 5000.  The reference uses the engine's
 * unseeded RNG, so only the distribution is reproduced.  Out: n x 4 floats each.
 */
NBODY_AMD_API int nbody_ic_reference_box(int32_t n, float size, const float center[3], uint64_t seed,
                                     float *posm4, float *vel4);

/* Seeded equal-mass Plummer sphere in virial equilibrium for constant G (build-defined workload). */
NBODY_AMD_API int nbody_ic_plummer(int32_t n, double total_mass, double scale_radius, double G, uint64_t seed,
                               float *posm4, float *vel4);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_AMD_H */
