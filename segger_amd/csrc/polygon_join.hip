// segger_polygon_join_count / _fill: every (point, polygon) pair for which the point lies in the polygon grown by a
// per-polygon distance d -- the reference's points_in_polygons (src/segger/geometry/query.py, a cuSpatial quadtree join)
// over polygons.buffer(d) (src/segger/data/utils/neighbors.py:223-238).  include/segger_amd.h has the contract and the
// predicate; this is the exact offset of the ring (Minkowski sum with a disc), not GEOS's polyline approximation of it.
//
// Six kernels and one radix sort on one stream, no host synchronisation (the grid and its cell_of are rings.h's; the
// scan kernel and the slot of a match, hit_slot, are post_common.h's):
//   pjoin_keys_kernel   one thread per point: key = cell << 32 | point id (cells clamped to the nx x ny grid);
//   (rocprim keys sort: stable by construction, the id is part of the key)
//   pjoin_cells_kernel  one thread per sorted position: cell_start[] and the cell-ordered float64 copy of the points (the
//                       ids stay in the low words of the sorted keys);
//   pjoin_bin_kernel    one thread per polygon: checks its ring (rings.h) and its distance, zeroes its count and appends
//                       a ring of 3 or more vertices to the list of its route;
//   pjoin_short_kernel  n <= 64: one wave per polygon, the ring in registers, edges broadcast by readlane, no LDS;
//   pjoin_long_kernel   64 < n <= SEGGER_MORPH_MAX_VERTS: one single-wave workgroup per polygon, the ring in LDS (64 KB),
//                       every lane reading the same edge (an LDS broadcast);
//   counts_to_offsets_kernel<int64>  one workgroup: counts -> pair_offsets, in place.
// The two polygon kernels are rings.h's loops (short_ring_loop, long_ring_loop) around polygon_body, a template on
// "count" / "fill" and the join's sink of THE walk, ring_predicate.h's walk_grown_ring: the wave walks the rows of grid
// cells that overlap the ring's bounds grown by d and a rounding margin, each row one contiguous span of the cell-ordered
// points, 64 points at a time, one point per lane, and loops over the edges accumulating the crossing parity and the
// smallest squared distance.  buffered_counts.hip and nearest_boundaries.hip are two more sinks of the same walk.
// A match's slot is the polygon's offset + the matches before it in the traversal (hit_slot): no atomic decides a slot,
// so the list of a polygon is in (cell row, cell, point id) order whatever the scheduling, and the same call gives the
// same bytes.  The keys, cells and binning kernels wrap join_grid.h's bodies; the layout, the host checks, the shared
// kernel arguments (WalkCommon) and the launches (grid_front, launch_ring_kernels, launch_offsets_scan) are that header's
// too.  What is left here is the wrappers, JoinArgs, polygon_body and the two entry points.
//
// Arithmetic: float64, the point and the vertices translated to the ring's first vertex, FMA contraction off, so with
// coordinates that are exactly representable after the translation the cross product, and with it the parity and "on the
// ring" (dist2 == 0), are exact.  Per edge (a, b) and point t:  e = b - a, w = t - a, cr = e.x w.y - e.y w.x,
// dot = w.e, len2 = e.e;  dist2 = |w|^2 if dot <= 0 or len2 == 0, |t - b|^2 if dot >= len2, cr cr / len2 otherwise.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel of this unit (the sort is
// instantiated with NoScratchSortConfig); pjoin_long_kernel holds 65536 B of LDS, two single-wave workgroups per CU.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "ring_predicate.h"
#include "sort_config.h"
#include "join_grid.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kPjThreads = kGridThreads;
constexpr int kPjWaves = kPjThreads / kWave;

// ---------------------------------------------------------------- the points, the polygons: join_grid.h ---
__global__ __launch_bounds__(kPjThreads) void pjoin_keys_kernel(const double* __restrict__ pts, int64_t n, UniformGrid g,
                                                                unsigned long long* __restrict__ keys) {
  grid_keys_body(pts, n, g, keys);
}

__global__ __launch_bounds__(kPjThreads) void pjoin_cells_kernel(const unsigned long long* __restrict__ keys_sorted,
                                                                 const double* __restrict__ pts, const int32_t*, int64_t n,
                                                                 int64_t n_cells, int32_t* __restrict__ cell_start,
                                                                 double2* __restrict__ sorted_pts, int32_t*) {
  grid_cells_body<false>(keys_sorted, pts, nullptr, n, n_cells, cell_start, sorted_pts, nullptr);
}

__global__ __launch_bounds__(kPjThreads) void pjoin_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                               const double* __restrict__ buffer, int64_t P, int64_t V,
                                                               int64_t* __restrict__ pair_offsets, int64_t*, int32_t* __restrict__ words,
                                                               int32_t* __restrict__ list_short, int32_t* __restrict__ list_long) {
  bin_rings_body(off, xy, buffer, P, V, pair_offsets, nullptr, words, list_short, list_long);
}

constexpr FrontKernels kPjFront{pjoin_keys_kernel, pjoin_cells_kernel, pjoin_bin_kernel,
                                "pjoin_keys_kernel", "pjoin_cells_kernel", "pjoin_bin_kernel"};

struct JoinArgs {
  WalkCommon c;                                                      // join_grid.h
  int64_t* pair_offsets;                                             // count: [p + 1] is written; fill: read
  int64_t* out;                                                      // fill: the point ids
  int64_t capacity;
};

// One polygon, one wave, every lane active: r is what rings.h's loops hand over.  The join's sink of the walk: a match's
// slot is the polygon's offset + the matches before it.
template <bool kFill, class Ring>
__device__ __forceinline__ void polygon_body(const ListedRing<Ring>& r, const JoinArgs& a) {
  const int64_t p = r.p;
  int64_t begin = 0, end = 0;
  if (kFill) {
    begin = a.pair_offsets[p];
    end = a.pair_offsets[p + 1];
    if (end > a.capacity) end = a.capacity;                          // nothing is ever written at or beyond either
  }
  int64_t found = 0;
  walk_polygon(a.c, r, [&](bool hit, int s, const RingDistance&) {
    hit_slot<kFill>(hit, begin, end, found, [&](int64_t slot) { a.out[slot] = (int64_t)(a.c.keys[s] & 0xffffffffull); });
  });
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (!kFill) a.pair_offsets[p + 1] = found;
    else if (begin + found != a.pair_offsets[p + 1] || begin + found > a.capacity) atomicOr(&a.c.words[kWordFlag], SEGGER_PJOIN_ERR_FILL);
  }
}

template <bool kFill>
__global__ __launch_bounds__(kPjThreads) void pjoin_short_kernel(JoinArgs a, const int32_t* __restrict__ list) {
  short_ring_loop(a.c.off, a.c.xy, a.c.words, list, kPjWaves, [&](const auto& r) { polygon_body<kFill>(r, a); });
}

template <bool kFill>
__global__ __launch_bounds__(kWave) void pjoin_long_kernel(JoinArgs a, const int32_t* __restrict__ list) {
  __shared__ double2 pts[SEGGER_MORPH_MAX_VERTS];
  long_ring_loop(a.c.off, a.c.xy, a.c.words, list, pts, [&](const auto& r) { polygon_body<kFill>(r, a); });
}

template <bool kFill>
constexpr RingKernels<JoinArgs> kPjRings{pjoin_short_kernel<kFill>, "pjoin_short_kernel", kPjWaves, 8,
                                         pjoin_long_kernel<kFill>, "pjoin_long_kernel", 2};

using PjLayout = GridLayout;                                         // join_grid.h: the layout and the checks
using PjCall = GridCall;
constexpr const char* kPjNames8 = "ring_offsets, pair_offsets and buffer";

PjLayout pj_layout(int64_t N, int64_t P, int64_t n_cells) { return grid_layout(N, P, n_cells, false); }

// everything both entry points reject; *empty = nothing to do (no pointer was looked at)
int pj_check(const char* who, const PjCall& c, bool* empty) {
  *empty = false;
  const int rc = grid_check_sizes(who, c.N, c.P, c.nx, c.ny);
  return rc != SEGGER_OK ? rc : grid_check(who, c, empty);
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_polygon_join_workspace_bytes(int64_t n_points, int64_t n_polygons, int32_t nx, int32_t ny) {
  const int rc = grid_check_sizes("segger_polygon_join_workspace_bytes", n_points, n_polygons, nx, ny);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)pj_layout(n_points, n_polygons, (int64_t)nx * ny).total;
}

extern "C" int segger_polygon_join_count(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                                         int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate,
                                         double x0, double y0, double cell, int32_t nx, int32_t ny, int64_t* pair_offsets,
                                         void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_polygon_join_count";
  hipStream_t stream = (hipStream_t)stream_;
  const PjCall c = grid_call(points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                             pair_offsets, workspace, workspace_bytes, kPjNames8);
  bool empty = false;
  int rc = pj_check(who, c, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  const PjLayout l = pj_layout(n_points, n_polygons, (int64_t)nx * ny);
  rc = grid_front(kPjFront, c, l, pair_offsets, nullptr, stream);
  if (rc == SEGGER_OK) rc = launch_ring_kernels(kPjRings<false>, c, l, JoinArgs{walk_common(c, l), pair_offsets, nullptr, 0}, stream);
  return rc != SEGGER_OK ? rc : launch_offsets_scan(pair_offsets, n_polygons, nullptr, stream);
}

extern "C" int segger_polygon_join_fill(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                                        int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate,
                                        double x0, double y0, double cell, int32_t nx, int32_t ny, const int64_t* pair_offsets,
                                        int64_t* point_index_out, int64_t capacity, void* workspace, int64_t workspace_bytes,
                                        segger_stream_t stream_) {
  const char* who = "segger_polygon_join_fill";
  hipStream_t stream = (hipStream_t)stream_;
  const PjCall c = grid_call(points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                             pair_offsets, workspace, workspace_bytes, kPjNames8);
  bool empty = false;
  int rc = pj_check(who, c, &empty);
  if (rc == SEGGER_OK) rc = grid_check_capacity(who, capacity, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  SEGGER_REQUIRE(point_index_out, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(point_index_out, 8), "%s: point_index_out must be 8-byte aligned", who);
  const PjLayout l = pj_layout(n_points, n_polygons, (int64_t)nx * ny);
  return launch_ring_kernels(kPjRings<true>, c, l, JoinArgs{walk_common(c, l), const_cast<int64_t*>(pair_offsets), point_index_out, capacity},
                             stream);
}
