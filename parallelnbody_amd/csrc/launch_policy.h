// Launch policy: which kernel, geometry and work plan a context gets — a function of nbody_params and of two facts about the
// device (CU count, total memory), never of what happens to be free, so that equal GPUs arrive at equal plans (the ranks of a sharded
// job must) and results are reproducible from box to box.  Every size threshold of the library lives in launch_policy.cpp.
// Host-only C++ (no HIP): nbody_create (capi.hip) asks the device once and calls choose_policy; the CPU tests reach the same code
// through nbody_launch_policy_describe (include/nbody.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nbody.h"
#include "sym_plan.h"

namespace nbody {

inline thread_local std::string g_create_error;   // what nbody_last_error(nullptr) reports: a failed creation has no context to keep it

struct DeviceFacts {
  int cus;                // compute units; <= 0 (the query failed): 256
  uint64_t total_bytes;   // the card's total memory; 0 = unknown: no plan is refused for its size
};

struct LaunchPolicy {
  // one-sided kernels (choose_geometry)
  int tile = 256, ipt = 1, j_split = 1, j_chunk = 0;
  int wave = 0;           // block kernels: register pairs (plain fp32) / bodies (Kahan, fp64) per workgroup; 0 = tile / symmetric kernels
  // symmetric pass (choose_algorithm): the scalars nbody_ctx keeps, and the plan to upload
  bool sym = false, sym_even = false;
  int sym_bi = 0, sym_np = 1, sym_pad = 0, sym_items_n = 0, sym_nsrc = 1, sym_slots = 0, sym_min_sub = 0, sym_n_local = 0, sym_n_gran = 0;
  double sym_k = 0.0;
  uint64_t sym_pool_elems = 0;
  SymPlan plan;
  // what nbody_create allocates besides
  int dup_slots = 0;      // coincident-body detector: hash slots (0 = none) ...
  int dup_tables = 0;     // ... and tables: 2 where fused stepping alternates between them
  bool equal_mass_word = false;   // the device word the equal-mass kernels are gated on
  bool recv_is_send = true;       // symmetric contexts that own all bodies: no receive rows of their own
};

// Environment overrides (tuning, A/B measurements, tests).  env_int: a positive integer or dflt.  env_flag: 1 / 0 when the
// variable starts with '1' / '0', -1 otherwise (unset included).
int env_int(const char *name, int dflt);
int env_flag(const char *name);

// nbody_create's argument checks: NBODY_OK, or the code with the message in *why.
int validate_params(const nbody_params &p, std::string *why);
inline int owned_count(const nbody_params &p) { return p.i_count ? p.i_count : p.n_total - p.i_begin; }

// The policy for validated parameters whose i_count is filled in (owned_count): NBODY_OK, or NBODY_ERR_UNSUPPORTED with the message
// nbody_create reports in *why.
int choose_policy(const nbody_params &p, DeviceFacts dev, LaunchPolicy *out, std::string *why);

int block_pairs(int n_total, int cus);     // register pairs per workgroup of forces_block_pk_kernel (nbody_block_pairs_describe)
size_t detector_table_bytes(int slots);    // the coincident-body detector's table: hash slots + {flag, count}

// Blocks / threads of the one-sided force launch (kernels.h forces_geometry).
void forces_geometry(int wave, int precision, int ipt, int j_split, int i_count, int *blocks, int *threads);

// nbody_force_kernel_name for a context with these policy fields (LaunchPolicy / nbody_ctx: sym, wave, ipt) at opening angle theta
const char *force_kernel_name(bool sym, int wave, int ipt, const nbody_params &p, float theta);

}  // namespace nbody
