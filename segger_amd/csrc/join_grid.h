// Everything around the walk (ring_predicate.h) that the units walking points against grown rings share (polygon_join.hip,
// buffered_counts.hip, nearest_boundaries.hip; included after rings.h and sort_config.h).  Device: the points binned into
// the uniform grid (keys, cell starts, cell-ordered points and -- for the counts -- their genes), the polygons binned by
// route, and WalkCommon, what the polygon kernels of every unit read.  Host: the layout of the workspace, the checks of an
// entry point, and its launches -- grid_front (words, keys, sort, cells, binning), launch_ring_kernels (a unit's short and
// long polygon kernel) and launch_offsets_scan.  "The join's grid" is one definition: the key format, the cell-start
// writing, the layout and the grid-stride factors are fixed here and nowhere else.  Each unit keeps thin __global__
// wrappers of its own around the bodies below (its kernels keep their names in its assembly), as with post_common.h's
// scan, and hands them over as FrontKernels / RingKernels; a unit is then its wrappers, its argument struct and what it
// does at a hit.
#pragma once
#include <math.h>

#include "post_common.h"
#include "rings.h"
#include "ring_predicate.h"
#include "sort_config.h"

namespace segger {

constexpr int kGridThreads = 256;                                    // the workgroup of the three kernels made of these bodies

// ---------------------------------------------------------------- the points ---
// one thread per point: key = cell << 32 | point id (cells clamped to the nx x ny grid)
__device__ __forceinline__ void grid_keys_body(const double* __restrict__ pts, int64_t n, const UniformGrid& g,
                                               unsigned long long* __restrict__ keys) {
  const int64_t stride = (int64_t)gridDim.x * kGridThreads;
  for (int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x; i < n; i += stride) {
    const double2 p = reinterpret_cast<const double2*>(pts)[i];
    const int cx = cell_of(p.x, g.x0, g.inv_cell, g.nx), cy = cell_of(p.y, g.y0, g.inv_cell, g.ny);
    keys[i] = ((unsigned long long)((int64_t)cy * g.nx + cx) << 32) | (unsigned long long)i;
  }
}

// one thread per sorted position: cell_start[] and the cell-ordered float64 copy of the points (the ids stay in the low
// words of the sorted keys); kGene: the points' int32 payload in cell order beside them
template <bool kGene>
__device__ __forceinline__ void grid_cells_body(const unsigned long long* __restrict__ keys_sorted, const double* __restrict__ pts,
                                                const int32_t* __restrict__ gene, int64_t n, int64_t n_cells,
                                                int32_t* __restrict__ cell_start, double2* __restrict__ sorted_pts,
                                                int32_t* __restrict__ sorted_gene) {
  const int64_t stride = (int64_t)gridDim.x * kGridThreads;
  for (int64_t s = (int64_t)blockIdx.x * kGridThreads + threadIdx.x; s < n; s += stride) {
    const unsigned long long key = keys_sorted[s];
    const int64_t id = (int64_t)(key & 0xffffffffull);               // < n: the keys kernel wrote it
    sorted_pts[s] = reinterpret_cast<const double2*>(pts)[id];
    if (kGene) sorted_gene[s] = gene[id];
    const int64_t k = (int64_t)(key >> 32);                          // < n_cells: the keys kernel clamped it
    const int64_t kprev = s > 0 ? (int64_t)(keys_sorted[s - 1] >> 32) : -1;
    for (int64_t c = kprev + 1; c <= k; ++c) cell_start[c] = (int32_t)s;
    if (s == n - 1)
      for (int64_t c = k + 1; c <= n_cells; ++c) cell_start[c] = (int32_t)n;
  }
}

// ---------------------------------------------------------------- the polygons ---
// one thread per polygon: checks its ring (rings.h) and its distance, zeroes its entry of `sizes` (the counts a scan turns
// into offsets: [p + 1], and [0]; NULL in a unit whose sizes are per point) and of `zeroed` (may be NULL), appends a ring of 3 or
// more vertices to the list of its route
__device__ __forceinline__ void bin_rings_body(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                               const double* __restrict__ buffer, int64_t P, int64_t V, int64_t* __restrict__ sizes,
                                               int64_t* __restrict__ zeroed, int32_t* __restrict__ words,
                                               int32_t* __restrict__ list_short, int32_t* __restrict__ list_long) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kGridThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kGridThreads + (threadIdx.x & ~(kWave - 1)); base < P; base += stride) {
    const int64_t p = base + lane;
    int route = -1;                                                  // -1: matches nothing
    if (p < P) {
      const RingClass c = classify_ring(off, xy, p, V);
      int bad = c.bad;
      if (buffer && !(buffer[p] >= 0.0 && buffer[p] < INFINITY)) bad |= SEGGER_PJOIN_ERR_BUFFER;
      if (bad) atomicOr(&words[kWordFlag], bad);
      if (sizes) {
        sizes[p + 1] = 0;                                            // the count; the polygon kernels overwrite theirs
        if (p == 0) sizes[0] = 0;
      }
      if (zeroed) zeroed[p] = 0;
      if (!bad && c.n >= 3) route = ring_route(c.n);
    }
    append_by_route(route, p, words, list_short, list_long);
  }
}

// ---------------------------------------------------------------- the polygon kernels ---
// what the polygon kernels of every unit read; a unit's argument struct embeds it (kernel parameters go by value)
struct WalkCommon {
  const int64_t* off;
  const double* xy;
  const double* buffer;                                              // [P] or NULL = 0
  int predicate;
  UniformGrid g;
  const int32_t* cell_start;
  const double2* pts;                                                // cell-ordered
  const unsigned long long* keys;                                    // cell-ordered; the low word is the point id
  int32_t* words;
};

// ring_predicate.h's walk of a listed ring (rings.h) with the distance, the predicate and the grid of a call
template <class Ring, class Visit>
__device__ __forceinline__ void walk_polygon(const WalkCommon& c, const ListedRing<Ring>& r, Visit&& visit) {
  walk_grown_ring(r.ring, r.n, r.first, r.xmin, r.ymin, r.xmax, r.ymax, c.buffer ? c.buffer[r.p] : 0.0, c.predicate, c.g,
                  c.cell_start, c.pts, visit);
}

// ---------------------------------------------------------------- host: layout ---
struct GridLayout {
  RingLists rings;
  size_t keys, pts, cell_start, temp, gene, total;                   // gene: only with_gene
  size_t temp_bytes;
  int key_bits;
};

// with n_points, n_polygons and n_cells below 2^31 every term is below 2^36 bytes: nothing here can overflow
inline GridLayout grid_layout(int64_t N, int64_t P, int64_t n_cells, bool with_gene) {
  GridLayout l;
  l.key_bits = 32 + bit_length((unsigned long long)(n_cells > 1 ? n_cells - 1 : 1));
  const size_t n = (size_t)(N > 0 ? N : 1);
  Carver c;
  l.rings = take_ring_lists(c, P);
  l.keys = c.take(n * 8);                                            // sorted keys: cell << 32 | point id
  l.pts = c.take(n * 16);                                            // cell-ordered points; before that, the unsorted keys
  l.cell_start = c.take((size_t)(n_cells + 1) * 4);
  size_t t = 0;
  unsigned long long* k64 = nullptr;
  (void)rocprim::radix_sort_keys<NoScratchSortConfig>(nullptr, t, k64, k64, n, 0, (unsigned)l.key_bits, (hipStream_t)0);
  l.temp_bytes = t;
  l.temp = c.take(t > 0 ? t : 1);
  l.gene = with_gene ? c.take(n * 4) : 0;                            // cell-ordered genes, behind the join's layout
  l.total = c.total();
  return l;
}

// ---------------------------------------------------------------- host: checks ---
inline int grid_check_sizes(const char* who, int64_t N, int64_t P, int32_t nx, int32_t ny) {
  SEGGER_REQUIRE(N >= 0 && P >= 0, "%s: negative n_points or n_polygons", who);
  SEGGER_REQUIRE(N < 0x7fffffffLL && P < 0x7fffffffLL, "%s: 2^31 - 1 points or polygons, or more", who);
  SEGGER_REQUIRE(nx >= 1 && ny >= 1 && (int64_t)nx * ny < 0x7fffffffLL, "%s: bad grid: nx, ny >= 1 and nx * ny < 2^31 - 1", who);
  return SEGGER_OK;
}

// what the units' entry points receive; offsets = pair_offsets / indptr, names8 how the 8-byte message lists them
struct GridCall {
  const double* points; int64_t N; const int64_t* ring_offsets; const double* xy; int64_t P, V; const double* buffer;
  int32_t predicate; double x0, y0, cell; int32_t nx, ny; const int64_t* offsets; void* workspace; int64_t workspace_bytes;
  bool with_gene; const int32_t* gene; const char* names8;
};

// the values in the order of the entry points' parameters; a unit with genes says so and passes them
inline GridCall grid_call(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy, int64_t n_polygons,
                          int64_t n_vertices, const double* buffer, int32_t predicate, double x0, double y0, double cell, int32_t nx,
                          int32_t ny, const int64_t* offsets, void* workspace, int64_t workspace_bytes, const char* names8,
                          bool with_gene = false, const int32_t* gene = nullptr) {
  return GridCall{points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                  offsets, workspace, workspace_bytes, with_gene, gene, names8};
}

// everything the entry points reject after the sizes (grid_check_sizes, and a unit's own, come first);
// *empty = nothing to do (no pointer was looked at)
inline int grid_check(const char* who, const GridCall& c, bool* empty) {
  *empty = false;
  SEGGER_REQUIRE(c.V >= 0, "%s: negative n_vertices", who);
  SEGGER_REQUIRE(c.workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(c.predicate == SEGGER_PJOIN_CONTAINS || c.predicate == SEGGER_PJOIN_INTERSECTS,
                 "%s: predicate %d is neither SEGGER_PJOIN_CONTAINS nor SEGGER_PJOIN_INTERSECTS", who, (int)c.predicate);
  SEGGER_REQUIRE(c.cell > 0.0 && c.cell < INFINITY && c.x0 - c.x0 == 0.0 && c.y0 - c.y0 == 0.0,
                 "%s: bad grid: the origin must be finite and the cell side positive and finite", who);
  if (c.N == 0 || c.P == 0) { *empty = true; return SEGGER_OK; }
  const size_t need = grid_layout(c.N, c.P, (int64_t)c.nx * c.ny, c.with_gene).total;
  const int rc = check_ring_call(who, c.ring_offsets, c.xy, c.V, c.workspace, c.workspace_bytes, need,
                                 OtherPointers{c.points && c.offsets && (c.gene || !c.with_gene),
                                               is_aligned(c.offsets, 8) && is_aligned(c.buffer, 8), is_aligned(c.points, 16), c.names8,
                                               "points and xy"});
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(is_aligned(c.gene, 4), "%s: gene must be 4-byte aligned", who);
  return SEGGER_OK;
}

// what a _fill entry point adds after its unit's checks: no capacity is nothing to do as well
inline int grid_check_capacity(const char* who, int64_t capacity, bool* empty) {
  SEGGER_REQUIRE(capacity >= 0, "%s: negative capacity", who);
  if (capacity == 0) *empty = true;
  return SEGGER_OK;
}

// ---------------------------------------------------------------- host: arguments and launches ---
inline WalkCommon walk_common(const GridCall& c, const GridLayout& l) {
  return WalkCommon{c.ring_offsets, c.xy, c.buffer, c.predicate, UniformGrid{c.x0, c.y0, 1.0 / c.cell, c.nx, c.ny},
                    at<int32_t>(c.workspace, l.cell_start), at<double2>(c.workspace, l.pts),
                    at<unsigned long long>(c.workspace, l.keys), at<int32_t>(c.workspace, l.rings.words)};
}

// A unit's wrappers of the three bodies above, under one signature each (a wrapper ignores what its body does not take:
// gene / sorted_gene without genes, sizes / zeroed where the unit zeroes its own), and their names in a launch error.
struct FrontKernels {
  void (*keys)(const double*, int64_t, UniformGrid, unsigned long long*);
  void (*cells)(const unsigned long long*, const double*, const int32_t*, int64_t, int64_t, int32_t*, double2*, int32_t*);
  void (*bin)(const int64_t*, const double*, const double*, int64_t, int64_t, int64_t*, int64_t*, int32_t*, int32_t*, int32_t*);
  const char *keys_name, *cells_name, *bin_name;
};

// The front of a _count entry point, on the stream: the words zeroed, the keys, their sort, the cells, the binning of the
// polygons (sizes, zeroed: bin_rings_body's).  Grid-stride factors: 32 workgroups a CU over the points, 8 over the polygons.
inline int grid_front(const FrontKernels& k, const GridCall& c, const GridLayout& l, int64_t* sizes, int64_t* zeroed, hipStream_t stream) {
  const WalkCommon w = walk_common(c, l);
  const int64_t n_cells = (int64_t)c.nx * c.ny;
  unsigned long long* keys_in = at<unsigned long long>(c.workspace, l.pts);      // dead once sorted: the points go there
  unsigned long long* keys = at<unsigned long long>(c.workspace, l.keys);
  const int cus = cu_count_or_default();
  const dim3 point_blocks(grid_stride_blocks(c.N, kGridThreads, (int64_t)cus * 32));
  SEGGER_HIP(hipMemsetAsync(w.words, 0, kRingWordsBytes, stream));
  hipLaunchKernelGGL(k.keys, point_blocks, dim3(kGridThreads), 0, stream, c.points, c.N, w.g, keys_in);
  SEGGER_LAUNCH_CHECK(k.keys_name);
  size_t temp_bytes = l.temp_bytes;
  SEGGER_HIP(rocprim::radix_sort_keys<NoScratchSortConfig>(at<char>(c.workspace, l.temp), temp_bytes, keys_in, keys, (size_t)c.N, 0,
                                                           (unsigned)l.key_bits, stream));
  hipLaunchKernelGGL(k.cells, point_blocks, dim3(kGridThreads), 0, stream, (const unsigned long long*)keys, c.points, c.gene, c.N,
                     n_cells, at<int32_t>(c.workspace, l.cell_start), at<double2>(c.workspace, l.pts),
                     c.with_gene ? at<int32_t>(c.workspace, l.gene) : (int32_t*)nullptr);
  SEGGER_LAUNCH_CHECK(k.cells_name);
  hipLaunchKernelGGL(k.bin, dim3(grid_stride_blocks(c.P, kGridThreads, (int64_t)cus * 8)), dim3(kGridThreads), 0, stream,
                     c.ring_offsets, c.xy, c.buffer, c.P, c.V, sizes, zeroed, w.words, at<int32_t>(c.workspace, l.rings.list_short),
                     at<int32_t>(c.workspace, l.rings.list_long));
  SEGGER_LAUNCH_CHECK(k.bin_name);
  return SEGGER_OK;
}

// A unit's two polygon kernels (rings.h's loops around its body) for one of count / fill: the short one with `short_waves`
// waves a workgroup, the long one with one; each at most `..._per_cu` workgroups a CU.  Args embeds a WalkCommon.
template <class Args>
struct RingKernels {
  void (*short_kernel)(Args, const int32_t*);
  const char* short_name;
  int short_waves, short_per_cu;
  void (*long_kernel)(Args, const int32_t*);
  const char* long_name;
  int long_per_cu;
};

template <class Args>
int launch_ring_kernels(const RingKernels<Args>& k, const GridCall& c, const GridLayout& l, const Args& a, hipStream_t stream) {
  const int cus = cu_count_or_default();
  hipLaunchKernelGGL(k.short_kernel, dim3(grid_stride_blocks(c.P, k.short_waves, (int64_t)cus * k.short_per_cu)),
                     dim3(k.short_waves * kWave), 0, stream, a, (const int32_t*)at<int32_t>(c.workspace, l.rings.list_short));
  SEGGER_LAUNCH_CHECK(k.short_name);
  hipLaunchKernelGGL(k.long_kernel, dim3(grid_stride_blocks(c.P, 1, (int64_t)cus * k.long_per_cu)), dim3(kWave), 0, stream, a,
                     (const int32_t*)at<int32_t>(c.workspace, l.rings.list_long));
  SEGGER_LAUNCH_CHECK(k.long_name);
  return SEGGER_OK;
}

// the tail of a _count entry point: sizes[1 .. n] -> offsets, in place; *total (may be NULL) = the last of them
// (static: the scan kernel is the including unit's own instance)
static int launch_offsets_scan(int64_t* sizes, int64_t n, int64_t* total, hipStream_t stream) {
  hipLaunchKernelGGL((counts_to_offsets_kernel<int64_t>), dim3(1), dim3(kScanThreads), 0, stream, sizes, n, total);
  SEGGER_LAUNCH_CHECK("counts_to_offsets_kernel");
  return SEGGER_OK;
}

}  // namespace segger
