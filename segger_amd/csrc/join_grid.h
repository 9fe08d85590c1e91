// The front half of the units that walk points against grown rings (polygon_join.hip, buffered_counts.hip,
// nearest_boundaries.hip; included after rings.h and sort_config.h): the points binned into the uniform grid (keys, cell
// starts, cell-ordered points and -- for the counts -- their genes), the polygons binned by route, the layout of the workspace and the host checks of an
// entry point.  "The join's grid" is one definition: the key format, the cell-start writing and the layout are fixed here
// and nowhere else.  Each unit keeps thin __global__ wrappers of its own around the bodies below (its kernels keep their
// names in its assembly), as with post_common.h's scan.
#pragma once
#include <math.h>

#include "post_common.h"
#include "rings.h"
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

// what both units' entry points receive; offsets = pair_offsets / indptr, names8 how the 8-byte message lists them
struct GridCall {
  const double* points; int64_t N; const int64_t* ring_offsets; const double* xy; int64_t P, V; const double* buffer;
  int32_t predicate; double x0, y0, cell; int32_t nx, ny; const int64_t* offsets; void* workspace; int64_t workspace_bytes;
  bool with_gene; const int32_t* gene; const char* names8;
};

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

}  // namespace segger
