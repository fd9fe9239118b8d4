// What the fp64 row scans share (kernels_pot64.hip, kernels_census64.hip, kernels_neighbours64.hip, kernels_groups64.hip, kernels_mst64.hip, kernels_pairs64.hip): rows held in
// registers — the bodies themselves or caller points, one or two per lane — against every body of one chunk, the bodies going through
// LDS.  The shape of all six tile kernels is deriv_tile_f64_kernel's (deriv_tile64.h; DESIGN.md, "The fp64 row scans"):
//   grid.x : blocks of kBlock * IPT rows (lane t holds rows ibase + t + k * kBlock: coalesced; the lanes past m repeat row m - 1 and
//            write nothing)
//   grid.y : the chunks of probe_geometry(n_total), [c * j_chunk, min((c + 1) * j_chunk, n_total)); each writes its own partial rows
// in double-buffered tiles of kJerkTile bodies, tile t + 1 fetched before tile t is consumed, the last tile padded with zeros ON THE
// ORIGIN (a kernel whose padding must not count keeps it out BY INDEX, j < j1; the separation census, which has no per-pair select to
// put that in, pads with NaNs and writes totals per workgroup, not partial rows), the bodies of a tile taken kJerk64Jb at a time by
// broadcast reads in ASCENDING j.
// Here: the HOST side of that shape, written once — the rows' slabs and the launch grids.  The DEVICE loop stays written out in each of
// the kernels.  It was tried as one function template with hooks (how body j is fetched, what is staged, what a group of bodies
// does to the lane's rows, what a row writes out), both with the sums captured by reference and with the sums as the template's own
// local: the group loop came out the same, but the compiler optimises such a template on its own before it inlines it, and every kernel
// then differed from its written-out form behind the first barrier — at best two independent instructions exchanged where a tile is
// staged, in the census the index conversion hoisted out of the write-out, in the neighbour kernels some fifty instructions more.  None
// of that is the same instructions with other registers, so the kernels keep their loops (profiles/query64_refactor_isa_compare.txt).
#pragma once
#include <algorithm>

#include "deriv_tile64.h"   // kJerkTile, kJerk64Jb

namespace nbody {
namespace {

constexpr int kScan64Ipt = 2;   // rows per lane where the rows are the bodies, as the jerk pass

// Rows in slabs whose partial rows fit the staging area (probe_slab_points(n_total, width) x j_split x width float4): run(slab) per slab
// launches the tile kernel on slab.grid and the fold on slab.fold.  self: the rows are the bodies, kScan64Ipt per lane; else caller
// points, hermite_block_lanes(m_all, lanes) per lane.  Which slab a row falls into, and how many rows its lane holds, changes nothing it
// is computed from.
struct RowSlab64 { size_t first; int m, ipt, j_split, j_chunk; dim3 grid, fold; };
template <class Run>
void for_row_slabs64(int n_total, int m_all, int width, bool self, int lanes, Run run) {
  RowSlab64 s;
  s.ipt = self ? kScan64Ipt : hermite_block_lanes(m_all, lanes);
  probe_geometry(n_total, &s.j_split, &s.j_chunk);
  const size_t slab = probe_slab_points(n_total, width);
  for (s.first = 0; s.first < (size_t)m_all; s.first += slab) {
    s.m = (int)std::min(slab, (size_t)m_all - s.first);
    s.grid = dim3((s.m + kBlock * s.ipt - 1) / (kBlock * s.ipt), s.j_split);
    s.fold = dim3((s.m + kBlock - 1) / kBlock);
    run(s);
  }
}

}  // namespace
}  // namespace nbody
