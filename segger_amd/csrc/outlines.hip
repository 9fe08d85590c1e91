// segger_cell_outlines: one concave boundary polygon per segmented cell -- the reference's generate_boundaries with its
// DEFAULT method="delaunay" (src/segger/export/boundary.py:57-154): triangulate the cell's transcripts, peel long and flat
// triangles off the rim, keep the outline of the largest piece that remains; optionally rounded by Chaikin corner cutting.
// include/segger_amd.h has the contract, DESIGN 3.5j the argument why the peel's order does not decide the result.
//
// The front end (keys, keys-only sort, compaction to present cells) and the back end (scan, emit with the Chaikin stage)
// are boundaries.hip's, shared through cell_rings.h: their kernels, and the host code that lays out the workspace, refuses
// a call and launches them.  In between:
//   out_bin_kernel       one thread per present cell: its length and its route (rings.h: append_by_route);
//   out_cell_kernel<N>   one single-wave WORKGROUP per cell, the whole per-cell state in LDS, N = 256 for a cell of at
//                        most 256 rows (17 KB: nine cells per CU) and N = SEGGER_OUTLINE_MAX_POINTS otherwise.
// Both kernels and the per-cell code are outline_cell.h's, shared with outlines_large.hip: stages 2 to 6 are written once
// over a route (outline_stages<R>), and LdsRoute<N> is the route described here.  This unit's own part is what a cell with
// more distinct points than N gets: the refusal.
// Why a single-wave workgroup and not a wave of a larger one: the state of a large cell is 136 KB, so only one fits a CU
// whatever the workgroup's shape, and the triangulation is a chain of dependent steps (a triangle is found, then its
// edges are looked up) in which more waves would wait on one another at a barrier per step; with one wave a barrier
// costs nothing, the control flow is scalar, and the many small cells fill the CU with independent workgroups instead.
//
// Stages of a cell, each loop with a trip count fixed before it is entered:
//   1 stage the rows into LDS (round after round when there are more than 2 N: sort what is staged, drop duplicates, stage
//     behind the distinct points), bitonic sort by (x, y), drop exact duplicates remembering multiplicity > 1;
//   2 Delaunay by growing edge by edge: the seed is point 0 and its nearest neighbour; directed edge id e = 3 t + k is edge
//     k of triangle t, the triangle list itself is the work queue (e runs over it while it grows), a hash of directed
//     edges in LDS says which edge already has its triangle, nb[e] is the twin of e or "hull";
//   3 d_max from the minimum incident edge per vertex (integer atomicMin on the bits of the squared length);
//   4 the two peels to their fixed points, 5 components by min-label propagation and their areas, 6 the ring walk.
// A table that overflows, a directed edge met twice or a walk that exceeds its bound refuses the cell through a counter
// (possible only when rounded predicates contradict each other); nothing loops on it.
//
// Arithmetic: float64, FMA contraction off.  orient2d and incircle are one expression each, on coordinate differences:
// exact when the coordinates share a grid and span fewer than 2^11 steps of it per cell.
//
// LDS of out_cell_kernel<N>, bytes (N = 2048: 139264 of the CU's 163840):
//   16 N  points, sorted distinct                      |  staging area of 2 N points while rows are read
//   16 N  directed-edge hash, 8 N uint16 slots; later the per-vertex minimum, N uint64  |
//   12 N  triangle vertices, 3 uint16 x 2 N triangles (2 n - 5 at most)
//   12 N  twins, uint16 per directed edge
//    6 N  predicate bits per directed edge
//    4 N  component label per triangle (0xffff: peeled)
//    2 N  multiplicity flag per staged point
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel of the unit, the library's
// included; out_cell_kernel<256> 17408 B and out_cell_kernel<2048> 139264 B of LDS.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "sort_config.h"
#include "cell_rings.h"
#include "outline_cell.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

// a cell above the capacity of its LDS route is refused through the counters
struct RefuseTooMany {
  __device__ __forceinline__ bool every_cell() const { return false; }
  __device__ __forceinline__ int limit(int n) const { return n; }
  __device__ __forceinline__ void operator()(const BndSegs& s, int j, int n, unsigned long long* counters) const { refuse_cell(s, j, counters); }
};

// ---------------------------------------------------------------- host ---
// cell_rings.h's head and nothing else
struct OutLayout { CellRingsLayout head; size_t total; };

OutLayout out_layout(int64_t n_rows, int64_t n_cells) {
  OutLayout l;
  Carver c;
  l.head = take_cell_rings(c, n_rows, n_cells);
  l.total = c.total();
  return l;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_cell_outlines_workspace_bytes(int64_t n_rows, int64_t n_cells) {
  const int rc = bnd_check_sizes("segger_cell_outlines_workspace_bytes", n_rows, n_cells);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)out_layout(n_rows, n_cells).total;
}

extern "C" int segger_cell_outlines(const double* xy, const int32_t* cell, const uint8_t* keep, int64_t n_rows, int64_t n_cells,
                                    double connectivity, int32_t smoothing, int64_t* ring_offsets, double* xy_out,
                                    int64_t xy_capacity, int32_t* cell_ids, int64_t* n_transcripts, uint64_t* counters,
                                    void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_cell_outlines";
  hipStream_t stream = (hipStream_t)stream_;
  const CellRingsCall a{xy, cell, keep, n_rows, n_cells, smoothing, ring_offsets, xy_out, xy_capacity, cell_ids, n_transcripts,
                        counters, workspace, workspace_bytes};
  int rc = bnd_check_sizes(who, n_rows, n_cells);
  if (rc != SEGGER_OK) return rc;
  const OutLayout l = out_layout(n_rows, n_cells);
  bool empty = false;
  rc = check_cell_rings_call(who, a, l.total, [&] { return check_connectivity(who, connectivity); }, &empty);
  if (rc != SEGGER_OK || empty) return rc;

  const CellRingsViews v = cell_rings_views(a, l.head);
  const BndSegs& s = v.s;
  const OutParams prm{connectivity};
  const int cus = cu_count_or_default();
  const int64_t cap = l.head.cells_cap;

  rc = launch_cell_rings_front(a, l.head, v, SEGGER_OUTLINE_COUNTERS, cus, stream);
  if (rc != SEGGER_OK) return rc;
  const RefuseTooMany refuse;
  hipLaunchKernelGGL(out_bin_kernel<RefuseTooMany>, dim3(grid_stride_blocks(cap, kBndThreads, (int64_t)cus * 8)), dim3(kBndThreads), 0,
                     stream, s, v.cnt, v.words, v.list_short, v.list_long, refuse);
  SEGGER_LAUNCH_CHECK("out_bin_kernel");
  hipLaunchKernelGGL((out_cell_kernel<kOutSmall, RefuseTooMany>), dim3(grid_stride_blocks(cap, 1, (int64_t)cus * 9)), dim3(kWave), 0,
                     stream, xy, s, (const int32_t*)v.words, (int)kWordShort, (const int32_t*)v.list_short, prm, refuse, v.cnt);
  SEGGER_LAUNCH_CHECK("out_cell_kernel<256>");
  hipLaunchKernelGGL((out_cell_kernel<kOutMax, RefuseTooMany>), dim3(grid_stride_blocks(n_rows / (kOutSmall + 1), 1, (int64_t)cus)),
                     dim3(kWave), 0, stream, xy, s, (const int32_t*)v.words, (int)kWordLong, (const int32_t*)v.list_long, prm, refuse, v.cnt);
  SEGGER_LAUNCH_CHECK("out_cell_kernel<max>");
  return launch_cell_rings_back(a, l.head, v, cus, stream);
}
