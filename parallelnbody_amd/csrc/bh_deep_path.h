// bh_deep_path.h — Octree::Add's descent below the path keys' 42 levels (OctreeSearch.h:60-81), for contexts whose tree may go
// deeper (nbody_set_bh_max_depth).  Plain C++ with no HIP dependency: the device includes it (kernels_bh_deep.hip) and a CPU test
// compiles it with g++ against the CPU restatement of the reference (tests/test_bh_deep_path.py).
//
// Every level is the reference's own arithmetic: octant = 4[x >= ox] + 2[y >= oy] + [z >= oz], child centre = float(double(o) +-
// double(Size) * 0.5), child Size = float(0.5 * double(Size)).  (The keys' descend_level takes the plain fp32 form above Size 2^-100;
// deep cells go below that, where only this form is the reference's.)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_DEEP_HD __host__ __device__ inline
#else
#define BH_DEEP_HD inline
#endif

namespace nbody {
namespace bh {

constexpr int kDeepMaxLevels = 200;          // the largest limit a context takes (the CPU checker cuts Add off there too)
constexpr int kDeepDigitsPerWord = 21;       // digits below level 42, three bits each, packed like the path keys (most significant first)
constexpr int kDeepWords = (kDeepMaxLevels - 42 + kDeepDigitsPerWord - 1) / kDeepDigitsPerWord;   // 8
constexpr int kDeepRunMax = 64;              // bodies of one level-42 cell the device resolves (status kStatusDeepRun above)

// one level of Add's descent of the point (px, py, pz) in the cell (o, size): the octant, and the child's box in (o, size)
BH_DEEP_HD int deep_descend(float px, float py, float pz, float o[3], float &size) {
  const int c = (px >= o[0] ? 4 : 0) | (py >= o[1] ? 2 : 0) | (pz >= o[2] ? 1 : 0);
  o[0] = (float)((double)o[0] + (double)size * ((c & 4) ? 0.5 : -0.5));
  o[1] = (float)((double)o[1] + (double)size * ((c & 2) ? 0.5 : -0.5));
  o[2] = (float)((double)o[2] + (double)size * ((c & 1) ? 0.5 : -0.5));
  size = (float)(0.5 * (double)size);
  return c;
}

// The digits of levels `from` .. `to` - 1 of a point whose descent stands at (o, size) of level `from`, packed into words[]
// (digit from + k in word k / 21, bits 3 * (20 - k % 21) up); o and size are left at level `to`.
BH_DEEP_HD void deep_digits(float px, float py, float pz, float o[3], float &size, int from, int to,
                            unsigned long long words[kDeepWords]) {
  for (int w = 0; w < kDeepWords; ++w) words[w] = 0ull;
  for (int lev = from, k = 0; lev < to; ++lev, ++k) {
    const unsigned long long c = (unsigned long long)deep_descend(px, py, pz, o, size);
    words[k / kDeepDigitsPerWord] |= c << (3 * (kDeepDigitsPerWord - 1 - k % kDeepDigitsPerWord));
  }
}

// digits two packed continuations share, at most `count`
BH_DEEP_HD int deep_common_digits(const unsigned long long *a, const unsigned long long *b, int count) {
  for (int w = 0; w < kDeepWords; ++w) {
    const unsigned long long x = a[w] ^ b[w];
    if (x != 0ull) {
      int lz = 0;
      while (!((x << lz) & 0x8000000000000000ull)) ++lz;
      const int d = w * kDeepDigitsPerWord + (lz - 1) / 3;
      return d < count ? d : count;
    }
  }
  return count;
}

// true iff continuation a comes before b in the tree's depth-first order (children 0..7)
BH_DEEP_HD bool deep_before(const unsigned long long *a, const unsigned long long *b) {
  for (int w = 0; w < kDeepWords; ++w)
    if (a[w] != b[w]) return a[w] < b[w];
  return false;
}

// Levels two points' paths share from level `from`, where both stand in the cell (o, size), down to at most level `to`: where Add
// splits them apart — the device's own steps (deep_digits, deep_common_digits), as bh_deep_runs_kernel takes them below level 42.
// Their leaves lie one level below: from the root (from = 0), the depth Add reaches on the two-body scene is this + 1.
BH_DEEP_HD int deep_split_level(const float o_from[3], float size_from, int from, int to, float ax, float ay, float az, float bx,
                                float by, float bz) {
  unsigned long long wa[kDeepWords], wb[kDeepWords];
  int lev = from;
  float oa[3] = {o_from[0], o_from[1], o_from[2]}, ob[3] = {o_from[0], o_from[1], o_from[2]};
  float sa = size_from, sb = size_from;
  while (lev < to) {                                           // (kDeepWords * 21 levels a go: the packing's own width)
    const int next = to - lev < kDeepWords * kDeepDigitsPerWord ? to : lev + kDeepWords * kDeepDigitsPerWord;
    deep_digits(ax, ay, az, oa, sa, lev, next, wa);
    deep_digits(bx, by, bz, ob, sb, lev, next, wb);
    const int c = deep_common_digits(wa, wb, next - lev);
    if (c < next - lev) return lev + c;
    lev = next;                                                // (still together: both stand in the same cell of level `next`)
  }
  return to;
}

}  // namespace bh
}  // namespace nbody
