// The fp64 group census of an fp64 state (nbody_get_radius_counts_f64, nbody_radius_counts_at_f64, nbody_get_groups_f64; build-defined:
// the reference computes none of it).  For a row at x and body j, with d = x_j - x and contraction OFF:
//     d2 = (dx*dx + dy*dy) + dz*dz          nbody_mass_within's expression, not the pair census's fma form
//     linked iff d2 <= r2                   r2 = radius * radius, one fp64 multiply on the host
//   groups_tile_f64_kernel<., MIN = false, COUNT = true, .>  <- the number of linked bodies per row (the radius counts; the points)
//   groups_tile_f64_kernel<., MIN = true,  COUNT = true, .>  <- and the smallest parent label among them (round 1 of the groups)
//   groups_tile_f64_kernel<., MIN = true,  COUNT = false, .> <- the smallest parent label alone (the later rounds)
//   <., ., ., SELF = true>                  <- the rows are the bodies (i_first + il of posm), each leaves itself out BY INDEX
//   <., ., ., SELF = false>                 <- the rows are caller points (ipos[il]); NO body is dropped by index
//   groups_fold_f64_kernel                  <- the chunks' rows in chunk order: min of the minima, sum of the counts
//   groups_iota / _hook / _compress / _members_count / _members_summary_kernel   <- the O(N) kernels of a round and of the summary
// A row scan (scan_tile64.h).  The tile's fourth component carries body j's current parent label (the low word of the double's bits, never computed
// with) where the census carries G m.  Each lane keeps per row an int32 minimum of the linked bodies' parents — from the row's own parent
// — and an int32 count, updated with compare and select.  A NaN d2 fails <=, a +inf d2 never passes a finite r2: neither links.  The
// candidates are the bodies j0 <= j < j1 of the chunk: the zero padding of a chunk's last tile is kept out BY INDEX (j < j1).  A
// zero-mass body links like any other.  d2_ij and d2_ji come from the same operations on negated operands: the graph is undirected in
// every bit.  A chunk's partial row is two int32 (minimum, count), 8 of the 16 bytes of a width-1 slot.  No scratch, no fp atomics.
//
// The groups are the connected components of the links, found in rounds the HOST drives (capi_query64.hip): a pass and its fold give
// every body the smallest parent among its linked bodies; the hook lowers the parent of the body's ROOT to it with an integer atomicMin
// on a COPY of the parent array (integer min is order-independent: the same array whatever the order); the compression chases that copy
// — read-only while it runs — to its fixed point for every body and writes the other array.  Parents never ascend (parent[i] <= i), so
// a chase ends; every round but the last merges at least two components.  No kernel waits on another workgroup or loops on a word
// another thread sets.
#include "kernels.h"

#include "scan_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

// local row il = blockIdx.x * (kBlock * IPT) + t + k * kBlock — the lanes past m repeat row m - 1 and write nothing — is
// SELF: body i_first + il of ipos (== posm);  else: point il of ipos — against the bodies of chunk blockIdx.y
template <int IPT, bool MIN, bool COUNT, bool SELF>
__global__ __launch_bounds__(kBlock) void groups_tile_f64_kernel(const double4 *__restrict__ posm, const int *__restrict__ parent,
                                                                 const double4 *__restrict__ ipos, int *__restrict__ part, int n_total, int m,
                                                                 int i_first, int j_chunk, double r2) {
  constexpr int JB = kJerk64Jb, TILE = kJerkTile;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  static_assert(MIN || COUNT, "a form computes something");
  static_assert(SELF || !MIN, "a point has no parent");
  __shared__ double4 shp[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT];
  int self[IPT], mn[IPT], cnt[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    self[k] = i_first + min(ibase + t + k * kBlock, m - 1);        // (the points' i_first is 0: the index into ipos)
    const double4 p = ipos[self[k]];
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z;
    mn[k] = MIN ? parent[self[k]] : 0;
    cnt[k] = 0;
  }

  double4 rp;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) { rp = posm[j]; rp.w = MIN ? __hiloint2double(0, parent[j]) : 0.0; }
    else        { rp = make_double4(0.0, 0.0, 0.0, 0.0); }          // padding: never linked
  };

  if (ntiles > 0) { load_tile(0); shp[0][t] = rp; }
  __syncthreads();
  for (int tile = 0; tile < ntiles; ++tile) {
    const int buf = tile & 1;
    const bool more = tile + 1 < ntiles;
    if (more) load_tile(tile + 1);
    const int jt = j0 + tile * TILE;
#pragma unroll 2
    for (int jj = 0; jj < TILE; jj += JB) {
      double4 pj[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) pj[b] = shp[buf][jj + b];
#pragma unroll
      for (int b = 0; b < JB; ++b)
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double dx = pj[b].x - xi[k], dy = pj[b].y - yi[k], dz = pj[b].z - zi[k];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          const int j = jt + jj + b;
          bool link = j < j1 && d2 <= r2;
          if (SELF) link = link && j != self[k];
          if (MIN) { const int pl = __double2loint(pj[b].w); mn[k] = (link && pl < mn[k]) ? pl : mn[k]; }
          if (COUNT) cnt[k] += link ? 1 : 0;
        }
    }
    if (more) shp[buf ^ 1][t] = rp;
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    if (il < m) {
      int *row = part + ((size_t)c * m + il) * 2;
      row[0] = mn[k]; row[1] = cnt[k];
    }
  }
}

// row k's answer: the chunks' rows in chunk order — min of the minima (mn, may be null), sum of the counts (count, may be null)
__global__ __launch_bounds__(kBlock) void groups_fold_f64_kernel(const int *__restrict__ part, int m, int j_split, int *__restrict__ mn,
                                                                 int *__restrict__ count) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  int lo = 0x7fffffff, sum = 0;
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const int *row = part + ((size_t)c * m + k) * 2;
    lo = min(lo, row[0]);
    sum += row[1];
  }
  if (mn) mn[k] = lo;
  if (count) count[k] = sum;
}

__global__ __launch_bounds__(kBlock) void groups_iota_kernel(int *__restrict__ parent, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) parent[i] = i;
}

// `hooked` is a copy of `parent`, whose every entry is a root (parent[parent[i]] == parent[i]): the root of a body that has a linked
// body under a smaller root is lowered to the smallest such root — integer atomicMin, the same array in whatever order they land
__global__ __launch_bounds__(kBlock) void groups_hook_kernel(const int *__restrict__ parent, const int *__restrict__ mn, int *__restrict__ hooked,
                                                             int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int root = parent[i], lo = mn[i];
  if (lo < root) atomicMin(&hooked[root], lo);
}

// parent[i] = the fixed point of `hooked` from i: hooked is read-only here and hooked[r] <= r, so the chase descends and ends within n
// steps (the bound is the loop's own: nothing here waits for another thread).  *changed = 1 where a label changed.
__global__ __launch_bounds__(kBlock) void groups_compress_kernel(const int *__restrict__ hooked, int *__restrict__ parent, int n,
                                                                 int *__restrict__ changed) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int r = i;
  for (int step = 0; step < n; ++step) {
    const int up = hooked[r];
    if (up >= r) break;
    r = up;
  }
  if (parent[i] != r) { parent[i] = r; *changed = 1; }
}

// size[label[i]] += 1 — integer atomicAdd on a cleared array
__global__ __launch_bounds__(kBlock) void groups_members_count_kernel(const int *__restrict__ label, int n, int *__restrict__ size) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) atomicAdd(&size[label[i]], 1);
}

// members[i] = size[label[i]], and the summary in sum[4] (cleared beforehand), integer atomics only — each is order-independent:
//   sum[0] += the groups (label[i] == i)     sum[1] += those with size >= 2     sum[2] += degree[i]
//   sum[3]  = max over the groups of (size << 32 | 0x7fffffff - label): the most members, the LOWEST label among ties
__global__ __launch_bounds__(kBlock) void groups_members_summary_kernel(const int *__restrict__ label, const int *__restrict__ size,
                                                                        const int *__restrict__ degree, int n, int *__restrict__ members,
                                                                        unsigned long long *__restrict__ sum) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  unsigned long long groups = 0, multiples = 0, links = 0, key = 0;
  if (i < n) {
    const int l = label[i], sz = size[l];
    members[i] = sz;
    links = (unsigned long long)degree[i];
    if (l == i) {
      groups = 1;
      multiples = sz >= 2 ? 1 : 0;
      key = ((unsigned long long)sz << 32) | (unsigned long long)(0x7fffffff - l);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    groups += __shfl_xor(groups, off, 64);
    multiples += __shfl_xor(multiples, off, 64);
    links += __shfl_xor(links, off, 64);
    const unsigned long long other = __shfl_xor(key, off, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) {
    if (groups) atomicAdd(&sum[0], groups);
    if (multiples) atomicAdd(&sum[1], multiples);
    if (links) atomicAdd(&sum[2], links);
    if (key) atomicMax(&sum[3], key);
  }
}

bool bad(const Groups64Launch &L) {
  return L.m <= 0 || L.n_total <= 0 || !L.posm || !L.part || !(L.r2 >= 0.0) || L.part_elems < probe_part_elems(L.n_total, L.m, kGroups64Width);
}

// the pass over the slabs and its fold — at the bodies (MIN: their smallest linked parent; COUNT: their links) or, ppos given, the counts
// at points; nothing is launched where an argument is missing, the bodies' form is asked for other than all bodies, or the staging area
// does not hold a slab's partial rows
template <bool MIN, bool COUNT>
hipError_t launch(const Groups64Launch &L, hipStream_t s) {
  const bool self = L.ppos == nullptr;
  if (bad(L) || (self && L.m != L.n_total) || (MIN && (!self || !L.parent || !L.mn)) || (COUNT && !L.count)) return hipErrorInvalidValue;
  const double4 *posm = (const double4 *)L.posm;
  for_row_slabs64(L.n_total, L.m, kGroups64Width, self, L.lanes, [&](const RowSlab64 &b) {
    if (self) {
      hipLaunchKernelGGL((groups_tile_f64_kernel<kScan64Ipt, MIN, COUNT, true>), b.grid, dim3(kBlock), 0, s, posm, L.parent, posm, (int *)L.part,
                         L.n_total, b.m, (int)b.first, b.j_chunk, L.r2);
    } else if constexpr (!MIN) {
      auto kernel = b.ipt == 2 ? groups_tile_f64_kernel<2, false, true, false> : groups_tile_f64_kernel<1, false, true, false>;
      hipLaunchKernelGGL(kernel, b.grid, dim3(kBlock), 0, s, posm, (const int *)nullptr, (const double4 *)L.ppos + b.first, (int *)L.part,
                         L.n_total, b.m, 0, b.j_chunk, L.r2);
    }
    hipLaunchKernelGGL(groups_fold_f64_kernel, b.fold, dim3(kBlock), 0, s, (const int *)L.part, b.m, b.j_split, MIN ? L.mn + b.first : nullptr,
                       COUNT ? L.count + b.first : nullptr);
  });
  return hipGetLastError();
}

}  // namespace

hipError_t launch_radius_counts_f64(const Groups64Launch &L, hipStream_t s) { return launch<false, true>(L, s); }

hipError_t launch_groups_pass_f64(const Groups64Launch &L, bool first_round, hipStream_t s) {
  return first_round ? launch<true, true>(L, s) : launch<true, false>(L, s);
}

hipError_t launch_groups_identity(int *parent, int n, hipStream_t s) {
  if (n <= 0 || !parent) return hipErrorInvalidValue;
  hipLaunchKernelGGL(groups_iota_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, parent, n);
  return hipGetLastError();
}

hipError_t launch_groups_merge(int *parent, const int *mn, int *hooked, int n, int *changed, hipStream_t s) {
  if (n <= 0 || !parent || !mn || !hooked || !changed) return hipErrorInvalidValue;
  const dim3 grid((n + kBlock - 1) / kBlock);
  hipError_t e = hipMemcpyAsync(hooked, parent, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(changed, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(groups_hook_kernel, grid, dim3(kBlock), 0, s, (const int *)parent, mn, hooked, n);
  hipLaunchKernelGGL(groups_compress_kernel, grid, dim3(kBlock), 0, s, (const int *)hooked, parent, n, changed);
  return hipGetLastError();
}

hipError_t launch_groups_members(const int *label, const int *degree, int n, int *size, int *members, unsigned long long *sum, hipStream_t s) {
  if (n <= 0 || !label || !degree || !size || !members || !sum) return hipErrorInvalidValue;
  const dim3 grid((n + kBlock - 1) / kBlock);
  hipError_t e = hipMemsetAsync(size, 0, (size_t)n * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(sum, 0, 4 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(groups_members_count_kernel, grid, dim3(kBlock), 0, s, label, n, size);
  hipLaunchKernelGGL(groups_members_summary_kernel, grid, dim3(kBlock), 0, s, label, (const int *)size, degree, n, members, sum);
  return hipGetLastError();
}

}  // namespace nbody
