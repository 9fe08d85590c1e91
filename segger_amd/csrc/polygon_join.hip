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
// The two polygon kernels are templates on "count" / "fill" over ONE traversal (polygon_body): the wave walks the rows of
// grid cells that overlap the ring's bounds grown by d and a rounding margin, each row one contiguous span of the
// cell-ordered points, 64 points at a time, one point per lane, and loops over the edges accumulating the crossing parity
// and the smallest squared distance (ring_predicate.h: ring_match and the cell range, shared with buffered_counts.hip).
// A match's slot is the polygon's offset + the matches before it in the traversal (hit_slot): no atomic decides a slot,
// so the list of a polygon is in (cell row, cell, point id) order whatever the scheduling, and the same call gives the
// same bytes.  The keys, cells and binning kernels wrap join_grid.h's bodies, and the layout and the host checks are that
// header's too: buffered_counts.hip bins with the same code.
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
                                                                 const double* __restrict__ pts, int64_t n, int64_t n_cells,
                                                                 int32_t* __restrict__ cell_start, double2* __restrict__ sorted_pts) {
  grid_cells_body<false>(keys_sorted, pts, nullptr, n, n_cells, cell_start, sorted_pts, nullptr);
}

__global__ __launch_bounds__(kPjThreads) void pjoin_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                               const double* __restrict__ buffer, int64_t P, int64_t V,
                                                               int64_t* __restrict__ pair_offsets, int32_t* __restrict__ words,
                                                               int32_t* __restrict__ list_short, int32_t* __restrict__ list_long) {
  bin_rings_body(off, xy, buffer, P, V, pair_offsets, nullptr, words, list_short, list_long);
}

struct JoinArgs {
  const int64_t* off;
  const double* xy;
  const double* buffer;                                              // [P] or NULL = 0
  int predicate;
  UniformGrid g;
  const int32_t* cell_start;
  const double2* pts;                                                // cell-ordered
  const unsigned long long* keys;                                    // cell-ordered; the low word is the point id
  int64_t* pair_offsets;                                             // count: [p + 1] is written; fill: read
  int64_t* out;                                                      // fill: the point ids
  int64_t capacity;
  int32_t* words;
};

// One polygon, one wave, every lane active.  n >= 3 vertices translated to org; xmin .. ymax are the ring's bounds on the
// coordinates as given (the same in every lane).
template <bool kFill, class Ring>
__device__ __forceinline__ void polygon_body(const Ring& ring, int n, P2 org, double xmin, double ymin, double xmax, double ymax,
                                             int64_t p, const JoinArgs& a) {
  const int lane = threadIdx.x & (kWave - 1);
  const double d = a.buffer ? a.buffer[p] : 0.0;
  const double dd = d * d;
  const CellRange r = grown_cell_range(xmin, ymin, xmax, ymax, d, a.g);              // ring_predicate.h: margin and all
  const int cx0 = r.cx0, cx1 = r.cx1, cy0 = r.cy0, cy1 = r.cy1;
  int64_t begin = 0, end = 0;
  if (kFill) {
    begin = a.pair_offsets[p];
    end = a.pair_offsets[p + 1];
    if (end > a.capacity) end = a.capacity;                          // nothing is ever written at or beyond either
  }
  int64_t found = 0;
  for (int cy = cy0; cy <= cy1; ++cy) {
    const int64_t row = (int64_t)cy * a.g.nx;
    const int s0 = __builtin_amdgcn_readfirstlane(a.cell_start[row + cx0]);
    const int s1 = __builtin_amdgcn_readfirstlane(a.cell_start[row + cx1 + 1]);
    for (int sb = s0; sb < s1; sb += kWave) {
      const int s = sb + lane;
      const bool valid = s < s1;
      const double2 t = a.pts[valid ? s : s0];
      const double px = t.x - org.x, py = t.y - org.y;
      const bool hit = valid && ring_match(ring, n, px, py, dd, a.predicate);            // ring_predicate.h: the one predicate
      hit_slot<kFill>(hit, begin, end, found, [&](int64_t slot) { a.out[slot] = (int64_t)(a.keys[s] & 0xffffffffull); });
    }
  }
  if (lane == 0) {
    if (!kFill) a.pair_offsets[p + 1] = found;
    else if (begin + found != a.pair_offsets[p + 1] || begin + found > a.capacity) atomicOr(&a.words[kWordFlag], SEGGER_PJOIN_ERR_FILL);
  }
}

template <bool kFill>
__global__ __launch_bounds__(kPjThreads) void pjoin_short_kernel(JoinArgs a, const int32_t* __restrict__ list) {
  const int count = a.words[kWordShort];
  const int n_waves = (int)gridDim.x * kPjWaves;
  for (int w = (int)blockIdx.x * kPjWaves + (int)(threadIdx.x >> 6); w < count; w += n_waves) {                // wave-uniform
    const int64_t p = list[w];
    const ShortRing s = load_short_ring(a.off, a.xy, p);             // 3 .. 64 vertices
    polygon_body<kFill>(s.ring, s.n, s.first, wave_min_f64(s.mine.x), wave_min_f64(s.mine.y), wave_max_f64(s.mine.x),
                        wave_max_f64(s.mine.y), p, a);
  }
}

template <bool kFill>
__global__ __launch_bounds__(kWave) void pjoin_long_kernel(JoinArgs a, const int32_t* __restrict__ list) {
  __shared__ double2 pts[SEGGER_MORPH_MAX_VERTS];
  const int count = a.words[kWordLong];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int64_t p = list[w];
    const LongRing r = stage_long_ring(a.off, a.xy, p, pts);
    LdsRing ring{pts};
    polygon_body<kFill>(ring, r.n, r.first, wave_min_f64(r.xmin), wave_min_f64(r.ymin), wave_max_f64(r.xmax), wave_max_f64(r.ymax),
                        p, a);
  }
}

using PjLayout = GridLayout;                                         // join_grid.h: the layout and the checks
using PjCall = GridCall;

PjLayout pj_layout(int64_t N, int64_t P, int64_t n_cells) { return grid_layout(N, P, n_cells, false); }

// everything both entry points reject; *empty = nothing to do (no pointer was looked at)
int pj_check(const char* who, const PjCall& c, bool* empty) {
  *empty = false;
  const int rc = grid_check_sizes(who, c.N, c.P, c.nx, c.ny);
  return rc != SEGGER_OK ? rc : grid_check(who, c, empty);
}

JoinArgs join_args(const PjCall& c, const PjLayout& l, int64_t* pair_offsets, int64_t* out, int64_t capacity) {
  JoinArgs a;
  a.off = c.ring_offsets;
  a.xy = c.xy;
  a.buffer = c.buffer;
  a.predicate = c.predicate;
  a.g = UniformGrid{c.x0, c.y0, 1.0 / c.cell, c.nx, c.ny};
  a.cell_start = at<int32_t>(c.workspace, l.cell_start);
  a.pts = at<double2>(c.workspace, l.pts);
  a.keys = at<unsigned long long>(c.workspace, l.keys);
  a.pair_offsets = pair_offsets;
  a.out = out;
  a.capacity = capacity;
  a.words = at<int32_t>(c.workspace, l.rings.words);
  return a;
}

template <bool kFill>
int launch_polygons(const PjCall& c, const PjLayout& l, const JoinArgs& a, hipStream_t stream) {
  const int cus = cu_count_or_default();
  hipLaunchKernelGGL((pjoin_short_kernel<kFill>), dim3(grid_stride_blocks(c.P, kPjWaves, (int64_t)cus * 8)), dim3(kPjThreads), 0,
                     stream, a, (const int32_t*)at<int32_t>(c.workspace, l.rings.list_short));
  SEGGER_LAUNCH_CHECK("pjoin_short_kernel");
  hipLaunchKernelGGL((pjoin_long_kernel<kFill>), dim3(grid_stride_blocks(c.P, 1, (int64_t)cus * 2)), dim3(kWave), 0, stream, a,
                     (const int32_t*)at<int32_t>(c.workspace, l.rings.list_long));
  SEGGER_LAUNCH_CHECK("pjoin_long_kernel");
  return SEGGER_OK;
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
  const PjCall c{points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                 pair_offsets, workspace, workspace_bytes, false, nullptr, "ring_offsets, pair_offsets and buffer"};
  bool empty = false;
  const int rc = pj_check(who, c, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  const int64_t n_cells = (int64_t)nx * ny;
  const PjLayout l = pj_layout(n_points, n_polygons, n_cells);
  const JoinArgs a = join_args(c, l, pair_offsets, nullptr, 0);
  unsigned long long* keys_in = at<unsigned long long>(workspace, l.pts);      // dead once sorted: the points go there
  unsigned long long* keys = at<unsigned long long>(workspace, l.keys);
  const int cus = cu_count_or_default();
  SEGGER_HIP(hipMemsetAsync(a.words, 0, kRingWordsBytes, stream));
  hipLaunchKernelGGL(pjoin_keys_kernel, dim3(grid_stride_blocks(n_points, kPjThreads, (int64_t)cus * 32)), dim3(kPjThreads), 0,
                     stream, points, n_points, a.g, keys_in);
  SEGGER_LAUNCH_CHECK("pjoin_keys_kernel");
  size_t temp_bytes = l.temp_bytes;
  SEGGER_HIP(rocprim::radix_sort_keys<NoScratchSortConfig>(at<char>(workspace, l.temp), temp_bytes, keys_in, keys, (size_t)n_points,
                                                           0, (unsigned)l.key_bits, stream));
  hipLaunchKernelGGL(pjoin_cells_kernel, dim3(grid_stride_blocks(n_points, kPjThreads, (int64_t)cus * 32)), dim3(kPjThreads), 0,
                     stream, (const unsigned long long*)keys, points, n_points, n_cells, at<int32_t>(workspace, l.cell_start),
                     at<double2>(workspace, l.pts));
  SEGGER_LAUNCH_CHECK("pjoin_cells_kernel");
  hipLaunchKernelGGL(pjoin_bin_kernel, dim3(grid_stride_blocks(n_polygons, kPjThreads, (int64_t)cus * 8)), dim3(kPjThreads), 0,
                     stream, ring_offsets, xy, buffer, n_polygons, n_vertices, pair_offsets, a.words,
                     at<int32_t>(workspace, l.rings.list_short), at<int32_t>(workspace, l.rings.list_long));
  SEGGER_LAUNCH_CHECK("pjoin_bin_kernel");
  const int rc2 = launch_polygons<false>(c, l, a, stream);
  if (rc2 != SEGGER_OK) return rc2;
  hipLaunchKernelGGL((counts_to_offsets_kernel<int64_t>), dim3(1), dim3(kScanThreads), 0, stream, pair_offsets, n_polygons,
                     (int64_t*)nullptr);
  SEGGER_LAUNCH_CHECK("counts_to_offsets_kernel");
  return SEGGER_OK;
}

extern "C" int segger_polygon_join_fill(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                                        int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate,
                                        double x0, double y0, double cell, int32_t nx, int32_t ny, const int64_t* pair_offsets,
                                        int64_t* point_index_out, int64_t capacity, void* workspace, int64_t workspace_bytes,
                                        segger_stream_t stream_) {
  const char* who = "segger_polygon_join_fill";
  hipStream_t stream = (hipStream_t)stream_;
  const PjCall c{points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                 pair_offsets, workspace, workspace_bytes, false, nullptr, "ring_offsets, pair_offsets and buffer"};
  bool empty = false;
  const int rc = pj_check(who, c, &empty);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(capacity >= 0, "%s: negative capacity", who);
  if (empty || capacity == 0) return SEGGER_OK;
  SEGGER_REQUIRE(point_index_out, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(point_index_out, 8), "%s: point_index_out must be 8-byte aligned", who);
  const PjLayout l = pj_layout(n_points, n_polygons, (int64_t)nx * ny);
  const JoinArgs a = join_args(c, l, const_cast<int64_t*>(pair_offsets), point_index_out, capacity);
  return launch_polygons<true>(c, l, a, stream);
}
