// The fp64 minimum spanning forest of an fp64 state (nbody_get_mst_f64; build-defined: the reference computes none of it), in Boruvka
// rounds the HOST drives (capi_query64.hip).  For a row at x and body j, with d = x_j - x and contraction OFF:
//     d2 = (dx*dx + dy*dy) + dz*dz          the group census's expression, not the pair census's fma form
//     an edge iff d2 is finite; edges compare by the key (d2, lo, hi), lo < hi: a strict total order
//   mst_tile_f64_kernel<IPT>                <- per row the body of ANOTHER label with the smallest d2, the lowest index among ties
//   mst_fold_f64_kernel                     <- the chunks' rows taken in chunk order with strict <, from (+inf, -1)
//   mst_iota / _pick_d2 / _pick_pair / _hook / _compress / _lowest / _component_kernel   <- the O(N) kernels of a round and of the labels
// A row scan (scan_tile64.h): the pair census's nearest form with the group census's distance and its label in the tile's fourth
// component (the low word of the double's bits, never computed with).  Each lane keeps (best d2, index) per row and updates them with
// compare and select in ASCENDING j under strict <: the lowest index wins a tie, a NaN is never taken (< is false), nor is +inf
// (+inf < +inf is false).  The candidates are the bodies j0 <= j < j1 of the chunk whose label is not the row's: the zero padding of a
// chunk's last tile is kept out BY INDEX (j < j1), the row's own component — the row itself included — BY LABEL.  For row i the pairs
// (min(i, j), max(i, j)) ascend with j, so the row's answer is the smallest KEY among the edges that leave its component at i.  d2_ij and
// d2_ji come from the same operations on negated operands: both ends of an edge see the same bits.  A chunk's partial row is
// (d2, index), 16 B, the index as a double (exact).  No scratch, no fp atomics.
//
// A round, behind the pass: every label keeps the smallest key among its bodies' answers — a finite d2 >= +0 orders as its bit pattern,
// so an integer atomicMin of the bits finds the d2, and a second one, among the bodies that attain it, the packed pair —; the label is
// hooked to the label at the foreign end of that edge; the successors are chased to their root for every body.  Under a strict total
// order the only cycle the successors can close is two labels that chose the SAME edge: the lower one stays a root there, and that edge
// is appended once.  Integer minima do not depend on the order they land in; the edges are appended in whatever order, and the host
// sorts them.  No kernel waits on another workgroup or loops on a word another thread sets.
#include "kernels.h"

#include "scan_tile64.h"

#pragma clang fp contract(off)

namespace nbody {

namespace {

constexpr unsigned long long kMstNone = ~0ull;

// local row il = blockIdx.x * (kBlock * IPT) + t + k * kBlock — the lanes past m repeat row m - 1 and write nothing — is body
// i_first + il of posm, against the bodies of chunk blockIdx.y
template <int IPT>
__global__ __launch_bounds__(kBlock) void mst_tile_f64_kernel(const double4 *__restrict__ posm, const int *__restrict__ label,
                                                              double *__restrict__ part, int n_total, int m, int i_first, int j_chunk) {
  constexpr int JB = kJerk64Jb, TILE = kJerkTile;
  static_assert(TILE == kBlock, "a lane stages one body per tile");
  __shared__ double4 shp[2][TILE];

  const int t = threadIdx.x;
  const int ibase = blockIdx.x * (kBlock * IPT);
  const int c = blockIdx.y;
  const int j0 = c * j_chunk;
  const int j1 = min(j0 + j_chunk, n_total);
  const int ntiles = (j1 > j0) ? (j1 - j0 + TILE - 1) / TILE : 0;

  double xi[IPT], yi[IPT], zi[IPT], best[IPT];
  int mine[IPT], at[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int self = i_first + min(ibase + t + k * kBlock, m - 1);
    const double4 p = posm[self];
    xi[k] = p.x; yi[k] = p.y; zi[k] = p.z;
    mine[k] = label[self];
    best[k] = __builtin_inf(); at[k] = -1;
  }

  double4 rp;
  auto load_tile = [&](int tile) {
    const int j = j0 + tile * TILE + t;
    if (j < j1) { rp = posm[j]; rp.w = __hiloint2double(0, label[j]); }
    else        { rp = make_double4(0.0, 0.0, 0.0, 0.0); }          // padding: never a candidate
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
      for (int b = 0; b < JB; ++b)                                 // ascending j: b, then the next group
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const double dx = pj[b].x - xi[k], dy = pj[b].y - yi[k], dz = pj[b].z - zi[k];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          const int j = jt + jj + b;
          const bool take = j < j1 && __double2loint(pj[b].w) != mine[k] && d2 < best[k];
          best[k] = take ? d2 : best[k];
          at[k] = take ? j : at[k];
        }
    }
    if (more) shp[buf ^ 1][t] = rp;
    __syncthreads();
  }

#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int il = ibase + t + k * kBlock;
    if (il < m) {
      double *row = part + ((size_t)c * m + il) * 2;
      row[0] = best[k]; row[1] = (double)at[k];
    }
  }
}

// row k's answer: the chunks' rows in chunk order under strict <, from (+inf, -1) — the chunks ascend in j, so the lowest index wins
__global__ __launch_bounds__(kBlock) void mst_fold_f64_kernel(const double *__restrict__ part, int m, int j_split, int *__restrict__ index,
                                                              double *__restrict__ d2) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= m) return;
  double best = __builtin_inf(), at = -1.0;
#pragma unroll 4
  for (int c = 0; c < j_split; ++c) {
    const double *row = part + ((size_t)c * m + k) * 2;
    const bool take = row[0] < best;
    best = take ? row[0] : best;
    at = take ? row[1] : at;
  }
  index[k] = (int)at;
  d2[k] = best;
}

__global__ __launch_bounds__(kBlock) void mst_iota_kernel(int *__restrict__ label, int *__restrict__ lowest, int *__restrict__ cursor, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) { label[i] = i; lowest[i] = i; }
  if (i == 0) *cursor = 0;
}

// best[label[i]] = min over the bodies with an answer of the bits of their d2 (finite and >= +0: the bits order as the values)
__global__ __launch_bounds__(kBlock) void mst_pick_d2_kernel(const int *__restrict__ label, const int *__restrict__ near_j,
                                                             const double *__restrict__ near_d2, unsigned long long *__restrict__ best, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || near_j[i] < 0) return;
  atomicMin(&best[label[i]], (unsigned long long)__double_as_longlong(near_d2[i]));
}

// pair[label[i]] = min over the bodies whose d2 is their label's best of (lo << 32 | hi), lo < hi the body and its answer
__global__ __launch_bounds__(kBlock) void mst_pick_pair_kernel(const int *__restrict__ label, const int *__restrict__ near_j,
                                                               const double *__restrict__ near_d2, const unsigned long long *__restrict__ best,
                                                               unsigned long long *__restrict__ pair, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int j = near_j[i], l = label[i];
  if (j < 0 || (unsigned long long)__double_as_longlong(near_d2[i]) != best[l]) return;
  const unsigned long long lo = (unsigned long long)min(i, j), hi = (unsigned long long)max(i, j);
  atomicMin(&pair[l], (lo << 32) | hi);
}

// every root r (label[r] == r): succ[r] = the label at the foreign end of its edge; itself where it has none, or where that label chose the
// same edge and r is the lower of the two.  The edge is appended by every root but the higher of such two.  label, best and pair are
// read-only here.
__global__ __launch_bounds__(kBlock) void mst_hook_kernel(const int *__restrict__ label, const unsigned long long *__restrict__ best,
                                                          const unsigned long long *__restrict__ pair, int *__restrict__ succ,
                                                          int *__restrict__ edge_i, int *__restrict__ edge_j, double *__restrict__ edge_d2,
                                                          int *__restrict__ cursor, int n) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n || label[r] != r) return;
  const unsigned long long p = pair[r];
  if (p == kMstNone) { succ[r] = r; return; }
  const int lo = (int)(p >> 32), hi = (int)(p & 0xffffffffull);
  const int llo = label[lo], lhi = label[hi];
  const int other = llo == r ? lhi : llo;
  const bool both = pair[other] == p;                              // the two labels chose each other's edge: the same one
  succ[r] = (both && r < other) ? r : other;
  if (both && r > other) return;
  const int slot = atomicAdd(cursor, 1);
  if (slot < n - 1) { edge_i[slot] = lo; edge_j[slot] = hi; edge_d2[slot] = __longlong_as_double((long long)best[r]); }
}

// label[i] = the root the successors lead to from label[i]: succ is read-only here and a forest, so the chase ends; it is capped at n
// steps all the same (the bound is the loop's own: nothing here waits for another thread)
__global__ __launch_bounds__(kBlock) void mst_compress_kernel(const int *__restrict__ succ, int *__restrict__ label, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int r = label[i];
  for (int step = 0; step < n; ++step) {
    const int up = succ[r];
    if (up == r) break;
    r = up;
  }
  label[i] = r;
}

// lowest[label[i]] = min(., i) on lowest = identity: a root's slot starts at the root, a body of its own component
__global__ __launch_bounds__(kBlock) void mst_lowest_kernel(const int *__restrict__ label, int *__restrict__ lowest, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) atomicMin(&lowest[label[i]], i);
}
__global__ __launch_bounds__(kBlock) void mst_component_kernel(const int *__restrict__ label, const int *__restrict__ lowest,
                                                               int *__restrict__ component, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) component[i] = lowest[label[i]];
}

bool whole(const Mst64Work &W) {
  return W.near_d2 && W.best && W.pair && W.edge_d2 && W.edge_i && W.edge_j && W.component && W.label && W.near_j && W.succ && W.lowest && W.cursor;
}

}  // namespace

// nothing is launched where an argument is missing, the rows are not all the bodies, or the staging area does not hold a slab's partial rows
hipError_t launch_mst_pass_f64(const Mst64Launch &L, hipStream_t s) {
  if (L.m <= 0 || L.n_total <= 0 || L.m != L.n_total || L.ppos || !L.posm || !L.part || !L.label || !L.index || !L.d2) return hipErrorInvalidValue;
  if (L.part_elems < probe_part_elems(L.n_total, L.m, kMst64Width)) return hipErrorInvalidValue;
  const double4 *posm = (const double4 *)L.posm;
  for_row_slabs64(L.n_total, L.m, kMst64Width, true, L.lanes, [&](const RowSlab64 &b) {
    hipLaunchKernelGGL(mst_tile_f64_kernel<kScan64Ipt>, b.grid, dim3(kBlock), 0, s, posm, L.label, (double *)L.part, L.n_total, b.m, (int)b.first,
                       b.j_chunk);
    hipLaunchKernelGGL(mst_fold_f64_kernel, b.fold, dim3(kBlock), 0, s, (const double *)L.part, b.m, b.j_split, L.index + b.first, L.d2 + b.first);
  });
  return hipGetLastError();
}

hipError_t launch_mst_begin(const Mst64Work &W, int n, hipStream_t s) {
  if (n <= 0 || !whole(W)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mst_iota_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, W.label, W.lowest, W.cursor, n);
  return hipGetLastError();
}

hipError_t launch_mst_clear(const Mst64Work &W, int n, hipStream_t s) {
  if (n <= 0 || !whole(W) || W.pair != W.best + n) return hipErrorInvalidValue;
  return hipMemsetAsync(W.best, 0xff, 2 * (size_t)n * sizeof(unsigned long long), s);
}

hipError_t launch_mst_merge(const Mst64Work &W, int n, hipStream_t s) {
  if (n <= 0 || !whole(W)) return hipErrorInvalidValue;
  const dim3 grid((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(mst_pick_d2_kernel, grid, dim3(kBlock), 0, s, (const int *)W.label, (const int *)W.near_j, (const double *)W.near_d2, W.best, n);
  hipLaunchKernelGGL(mst_pick_pair_kernel, grid, dim3(kBlock), 0, s, (const int *)W.label, (const int *)W.near_j, (const double *)W.near_d2,
                     (const unsigned long long *)W.best, W.pair, n);
  hipLaunchKernelGGL(mst_hook_kernel, grid, dim3(kBlock), 0, s, (const int *)W.label, (const unsigned long long *)W.best,
                     (const unsigned long long *)W.pair, W.succ, W.edge_i, W.edge_j, W.edge_d2, W.cursor, n);
  hipLaunchKernelGGL(mst_compress_kernel, grid, dim3(kBlock), 0, s, (const int *)W.succ, W.label, n);
  return hipGetLastError();
}

hipError_t launch_mst_components(const Mst64Work &W, int n, hipStream_t s) {
  if (n <= 0 || !whole(W)) return hipErrorInvalidValue;
  const dim3 grid((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(mst_lowest_kernel, grid, dim3(kBlock), 0, s, (const int *)W.label, W.lowest, n);
  hipLaunchKernelGGL(mst_component_kernel, grid, dim3(kBlock), 0, s, (const int *)W.label, (const int *)W.lowest, W.component, n);
  return hipGetLastError();
}

}  // namespace nbody
