// Frames of a deep context (nbody_set_bh_max_depth) whose tree goes below the path keys' 42 levels — see bh_common.h.
//
// The keys and their cold sort are the larger systems' own.  A *deep cluster* is a run of sorted bodies whose keys agree in all 42
// digits: any order of such a run keeps the key order valid, so bh_deep_runs_kernel orders each run by its bodies' paths below
// level 42 (bh_deep_path.h, Octree::Add's arithmetic) and writes the extended shared-digit counts as ints.  The rest is the compact
// tree of kernels_bh_build.hip with those counts: the node numbering (one workgroup scans the counts), node words whose level field
// saturates at 63 while the hop word carries the level's own threshold (the lane walk reads nothing else), ComputeMass a launch per
// level, and the lane walk itself (bh_walk_lane_kernel).  Default contexts never launch any of this.
#include "bh_common.h"
#include "bh_deep_path.h"

namespace nbody {
namespace bh {

// the acceptance thresholds of levels 0 .. levels (bh_frame_setup's rule, .h:74 / .h:103) — Size from the root the key kernel set
__global__ __launch_bounds__(kB) void bh_deep_thr_kernel(SmallTree T, float theta, int levels, float *__restrict__ thr) {
  const int t = threadIdx.x;
  if (T.hdr[3] != 0 || t > levels) return;
  float s_l = T.root[3];
  for (int q = 0; q < t; ++q) s_l = (float)(0.5 * (double)s_l);
  thr[t] = accept_threshold(s_l, theta);
}

// digits the bodies at sorted positions ia, ib share in their keys (0 .. 42)
__device__ __forceinline__ int deep_key_shared(const SmallTree &T, int ia, int ib) {
  const unsigned long long ha = T.khi[ia], hb = T.khi[ib];
  const unsigned long long x = ha ^ hb;
  if (x != 0ull) return (__clzll((long long)x) - 1) / 3;
  return shared_digits(ha, second_word(T, ia), hb, second_word(T, ib));
}

// lcpD[i] = shared digits of sorted positions i - 1 and i (-1 at both ends), below level 42 as Add continues the paths.  A thread
// that sees the start of a run of keys equal in all 42 digits orders the run by the paths' continuations (insertion sort; a run is a
// handful of bodies in any scene that is not refused anyway) and writes the run's counts; a pair still together at `levels` refuses
// the frame (status 1), as coincident bodies must.  Runs longer than kDeepRunMax: status kStatusDeepRun.
__global__ __launch_bounds__(kB) void bh_deep_runs_kernel(SmallTree T, const float4 *__restrict__ posm, int n, int levels,
                                                          int *__restrict__ lcpD, unsigned long long *__restrict__ xkey) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (T.hdr[3] != 0) return;
  const int s = i + 1 < n ? deep_key_shared(T, i, i + 1) : -1;
  // header word 6: neighbours that agree in the whole first key word (the next cold sort's choice, as bh_lcp_scan_kernel counts them)
  const unsigned long long tb = __ballot(s >= kLevelsPerKey);
  if (tb != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)tb) - 1) atomicAdd(&T.hdr[6], (int)__popcll(tb));
  if (i >= n) return;
  if (i == 0) { lcpD[0] = -1; lcpD[n] = -1; }
  if (i + 1 >= n) return;
  // (a cold sort that left keys out of order: an internal error, as in bh_lcp_scan_kernel)
  if (T.khi[i + 1] < T.khi[i] || (T.khi[i + 1] == T.khi[i] && second_word(T, i + 1) < second_word(T, i))) T.hdr[3] = kStatusUnsorted;
  if (s < kMaxLevels) { lcpD[i + 1] = s; return; }
  if (i > 0 && deep_key_shared(T, i - 1, i) == kMaxLevels) return;   // inside a run: its first body's thread does the run
  int e = i + 1;
  while (e + 1 < n && deep_key_shared(T, e, e + 1) == kMaxLevels) ++e;
  const int len = e - i + 1;
  if (len > kDeepRunMax) { T.hdr[3] = kStatusDeepRun; return; }
  // the run's cell of level 42: Add's descent of its first body (every body of the run takes the same 42 steps)
  float o42[3] = {T.root[0], T.root[1], T.root[2]};
  float s42 = T.root[3];
  {
    const float4 p = posm[T.sidx[i]];
    for (int lev = 0; lev < kMaxLevels; ++lev) (void)deep_descend(p.x, p.y, p.z, o42, s42);
  }
  const int count = levels - kMaxLevels;                       // digits below level 42 that can still tell bodies apart
  unsigned long long *X = xkey + (size_t)i * kDeepWords;
  for (int q = 0; q < len; ++q) {
    const float4 p = posm[T.sidx[i + q]];
    float o[3] = {o42[0], o42[1], o42[2]};
    float sz = s42;
    unsigned long long w[kDeepWords];
    deep_digits(p.x, p.y, p.z, o, sz, kMaxLevels, levels, w);
    for (int k = 0; k < kDeepWords; ++k) X[q * kDeepWords + k] = w[k];
  }
  for (int q = 1; q < len; ++q) {                              // insertion sort of the run by continuation (stable)
    unsigned long long w[kDeepWords];
    for (int k = 0; k < kDeepWords; ++k) w[k] = X[q * kDeepWords + k];
    const unsigned int b = T.sidx[i + q];
    int r = q;
    while (r > 0 && deep_before(w, X + (r - 1) * kDeepWords)) {
      for (int k = 0; k < kDeepWords; ++k) X[r * kDeepWords + k] = X[(r - 1) * kDeepWords + k];
      T.sidx[i + r] = T.sidx[i + r - 1];
      --r;
    }
    for (int k = 0; k < kDeepWords; ++k) X[r * kDeepWords + k] = w[k];
    T.sidx[i + r] = b;
  }
  for (int q = 0; q + 1 < len; ++q) {
    const int c = deep_common_digits(X + q * kDeepWords, X + (q + 1) * kDeepWords, count);
    if (c >= count) T.hdr[3] = 1;                              // together at the limit: the reference would recurse on
    lcpD[i + q + 1] = kMaxLevels + c;
  }
}

// first[i] = the first node of body i's group (the exclusive scan of max(lcp(i) - lcp(i-1), 0) + 1), first[n] = all nodes; the
// deepest level with a cell of >= 2 bodies goes to the header's first deep slot (bh_finish_kernel reads them all).  One workgroup.
__global__ __launch_bounds__(1024) void bh_deep_scan_kernel(SmallTree T, int n, const int *__restrict__ lcpD, int *__restrict__ first) {
  __shared__ int s_sum[1024];
  __shared__ int s_max[1024];
  const int t = threadIdx.x;
  if (T.hdr[3] != 0) return;
  const int per = (n + 1023) / 1024, a = min(t * per, n), b = min(a + per, n);
  int sum = 0, deep = -1;
  for (int i = a; i < b; ++i) {
    const int lp = lcpD[i], ln = lcpD[i + 1];
    sum += (ln > lp ? ln - lp : 0) + 1;
    deep = max(deep, ln);
  }
  s_sum[t] = sum; s_max[t] = deep;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {                   // inclusive scan (Hillis-Steele) of the threads' sums
    const int v = t >= off ? s_sum[t - off] : 0;
    const int m = t >= off ? s_max[t - off] : -1;
    __syncthreads();
    s_sum[t] += v; s_max[t] = max(s_max[t], m);
    __syncthreads();
  }
  int run = s_sum[t] - sum;
  for (int i = a; i < b; ++i) {
    const int lp = lcpD[i], ln = lcpD[i + 1];
    first[i] = run;
    run += (ln > lp ? ln - lp : 0) + 1;
  }
  if (t == 1023) {
    const int total = s_sum[1023];
    first[n] = total;
    if (total > T.cap) { T.hdr[0] = 0; T.hdr[3] = 2; return; }   // the node pool
    T.hdr[0] = total;
    T.hdr[kHdrDeep] = s_max[1023];
  }
}

// body i (key order): the words of the cells it opens, its leaf's word, CoM and level (bh_nodes_kernel with the extended counts).  A
// cell's end: a binary search on the keys down to level 42, the counts of the run below it.
__global__ __launch_bounds__(kB) void bh_deep_nodes_kernel(SmallTree T, const float4 *__restrict__ posm, int n, const int *__restrict__ first,
                                                           const int *__restrict__ lcpD, const float *__restrict__ thr) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n || T.hdr[3] != 0) return;
  const int lp = lcpD[i], ln = lcpD[i + 1], m0 = first[i];
  const int open = ln > lp ? ln - lp : 0;
  const unsigned long long h0 = T.khi[i], l0 = second_word(T, i);
  for (int q = 0; q < open; ++q) {
    const int l = lp + 1 + q;
    int upper;
    if (l <= kMaxLevels) {
      int x = i + 1, y = n;
      while (x < y) {
        const int mid = (x + y) >> 1;
        if (same_prefix(T.khi[mid], second_word(T, mid), h0, l0, l)) x = mid + 1; else y = mid;
      }
      upper = x;
    } else {
      upper = i + 1;
      while (lcpD[upper] >= l) ++upper;                        // (lcpD[n] = -1 ends it)
    }
    const unsigned int past = (unsigned int)first[upper];
    T.meta[m0 + q] = ((unsigned int)min(l, 63) << kLevelShift) | past;
    T.hop[m0 + q] = make_uint2(past, __float_as_uint(thr[l]));
  }
  const int level = (lp > ln ? lp : ln) + 1;
  const unsigned int body = T.sidx[i];
  T.meta[m0 + open] = kLeafBit | ((unsigned int)min(level, 63) << kLevelShift) | body;
  T.hop[m0 + open] = make_uint2(kLeafBit | (unsigned int)(m0 + open + 1), 0u);
  T.com[m0 + open] = posm[body];                               // CenterOfMass = Position, TotalMass = Mass (.h:85-88)
  T.leaf_level[i] = (unsigned char)level;
}

// ComputeMass (.h:89-95) of the cells of level l: body i opens one iff lcp(i-1) < l <= lcp(i)
__global__ __launch_bounds__(kB) void bh_deep_sweep_level_kernel(SmallTree T, const float4 *__restrict__ posm, int n,
                                                                 const int *__restrict__ first, const int *__restrict__ lcpD, int l,
                                                                 int div_mode) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n || T.hdr[3] != 0) return;
  const int lp = lcpD[i];
  if (!(lp < l && l <= lcpD[i + 1])) return;
  const int m = first[i] + (l - lp - 1);
  T.com[m] = sweep_compact_cell(T.com, T.meta, m, T.meta[m], l, div_mode, posm, T.root);
}

// What DrawOctreeBoxes hands to DrawDebugBox (.cpp:39-40): the leaf's box from the body's path digits — the keys' 42, then the
// continuation its run was ordered by
__global__ __launch_bounds__(kB) void bh_deep_leaf_boxes_kernel(SmallTree T, int n, const unsigned long long *__restrict__ xkey,
                                                                float4 *__restrict__ out) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= n) return;
  const unsigned long long h = T.khi[i];
  const int level = T.leaf_level[i];
  const unsigned long long l = level > kLevelsPerKey ? second_word(T, i) : 0ull;
  float o[3] = {T.root[0], T.root[1], T.root[2]};
  float size = T.root[3];
  for (int lev = 0; lev < level; ++lev) {
    int c;
    if (lev < kLevelsPerKey) c = (int)((h >> (3 * (kLevelsPerKey - 1 - lev))) & 7ull);
    else if (lev < kMaxLevels) c = (int)((l >> (3 * (kMaxLevels - 1 - lev))) & 7ull);
    else {
      const int k = lev - kMaxLevels;
      c = (int)((xkey[(size_t)i * kDeepWords + k / kDeepDigitsPerWord] >> (3 * (kDeepDigitsPerWord - 1 - k % kDeepDigitsPerWord))) & 7ull);
    }
    float no[3], ns;
    child_box(o, size, c, no, &ns);
    o[0] = no[0]; o[1] = no[1]; o[2] = no[2]; size = ns;
  }
  out[T.sidx[i]] = make_float4(o[0], o[1], o[2], size);
}

}  // namespace bh
}  // namespace nbody
