// segger_buffered_counts_count / _fill: the polygon x gene count matrix of boundaries grown by a per-polygon distance d,
// as a CSR -- the reference's get_buffered_counts -> buffer_polygons -> get_expression_matrix
// (src/segger/metrics/segment.py:66-122, three cuSpatial calls), the nucleus-expansion baseline.  include/segger_amd.h has
// the contract.  The join of polygon_join.hip and the histogram of expression.hip fused: the pair list [2, E], its int64
// sort and the (cell, gene) sort of the composition are never made.
//
// Kernels, one stream, no host synchronisation inside an entry point:
//   bcount_keys_kernel    one thread per point: key = cell << 32 | point id, the join's grid;
//   (rocprim keys sort)
//   bcount_cells_kernel   one thread per sorted position: cell_start[], the cell-ordered points and their genes;
//   bcount_bin_kernel     one thread per polygon: checks its ring and its distance, zeroes its row size and cell_count,
//                         appends a ring of 3 or more vertices to the list of its route;
//                         (these three are wrappers around join_grid.h's bodies, which polygon_join.hip wraps as well: one
//                         key format, one cell-start rule, one workspace layout, one set of host checks and one front --
//                         grid_front -- for the units)
//   bcount_short_kernel   n <= 64: one wave per polygon, the ring in registers.  Small tier: four waves a workgroup, each
//                         with its own hist[SEGGER_BCOUNT_SMALL_GENES] and touched list; large tier: one wave a workgroup,
//                         hist[SEGGER_BCOUNT_MAX_GENES];
//   bcount_long_kernel    64 < n <= SEGGER_MORPH_MAX_VERTS: one single-wave workgroup per polygon, the ring in LDS (64 KB)
//                         beside the histogram of its tier;
//   counts_to_offsets_kernel<int64>  one workgroup: row sizes -> indptr, in place, and nnz.
// The polygon kernels are templates on count / fill and on the tier: their LDS, rings.h's loops (short_ring_loop,
// long_ring_loop) and ONE body (count_body), a sink of the join's walk (ring_predicate.h: walk_grown_ring; the arguments
// and the launches are join_grid.h's): per hit an LDS atomic add on hist[gene]; the lane that sees the old
// value 0 appends the gene to the touched list at a ballot-derived slot.  After the walk the list is sorted (wave_sort.h),
// the row is written from it and exactly those entries of hist are zeroed again.  More distinct genes than the list holds:
// one ordered scan of hist writes the row and zeroes all of it.
//
// Why the bytes do not depend on scheduling: the atomics are integer adds on a wave-private array, the order in which the
// lanes win their slots in the touched list is erased by the sort, and the overflow scan is in gene order by construction.
//
// LDS (static, hipcc -Rpass-analysis=kernel-resource-usage): hist 4 G + list 2048 B per wave, G = 2048 or 24064 --
// short/small 4 x 10240 = 40960 B, short/large 98304 B, long/small 75776 B, long/large 163840 B (all of a CU: one
// workgroup, one wave; the price of a 4096-vertex ring on a whole-transcriptome panel).  No scratch.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "ring_predicate.h"
#include "sort_config.h"
#include "join_grid.h"
#include "wave_sort.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

static_assert(SEGGER_BCOUNT_ERR_OFFSETS == SEGGER_PJOIN_ERR_OFFSETS && SEGGER_BCOUNT_ERR_CAP == SEGGER_PJOIN_ERR_CAP &&
              SEGGER_BCOUNT_ERR_BUFFER == SEGGER_PJOIN_ERR_BUFFER && SEGGER_BCOUNT_ERR_FILL == SEGGER_PJOIN_ERR_FILL,
              "the error bits mirror the join's");
static_assert(SEGGER_BCOUNT_LDS_BYTES == 160 * 1024, "what a CDNA4 workgroup can address");
static_assert(SEGGER_BCOUNT_MAX_GENES * 4 + SEGGER_BCOUNT_TOUCHED * 4 + SEGGER_MORPH_MAX_VERTS * 16 == SEGGER_BCOUNT_LDS_BYTES,
              "the large tier of the long-ring route fills the LDS exactly");
static_assert((SEGGER_BCOUNT_TOUCHED & (SEGGER_BCOUNT_TOUCHED - 1)) == 0 && SEGGER_BCOUNT_TOUCHED >= kWave, "the sort pads to a power of two");

constexpr int kBcThreads = kGridThreads;
constexpr int kBcWaves = kBcThreads / kWave;
constexpr int kTouched = SEGGER_BCOUNT_TOUCHED;
constexpr int kCtrPairs = 0, kCtrNnz = 1, kCtrBad = 2, kCtrOverflow = 3, kCtrLarge = 4;

constexpr int tier_genes(bool large) { return large ? SEGGER_BCOUNT_MAX_GENES : SEGGER_BCOUNT_SMALL_GENES; }

// ---------------------------------------------------------------- the points, the polygons: join_grid.h ---
__global__ __launch_bounds__(kBcThreads) void bcount_keys_kernel(const double* __restrict__ pts, int64_t n, UniformGrid g,
                                                                 unsigned long long* __restrict__ keys) {
  grid_keys_body(pts, n, g, keys);
}

__global__ __launch_bounds__(kBcThreads) void bcount_cells_kernel(const unsigned long long* __restrict__ keys_sorted,
                                                                  const double* __restrict__ pts, const int32_t* __restrict__ gene,
                                                                  int64_t n, int64_t n_cells, int32_t* __restrict__ cell_start,
                                                                  double2* __restrict__ sorted_pts, int32_t* __restrict__ sorted_gene) {
  grid_cells_body<true>(keys_sorted, pts, gene, n, n_cells, cell_start, sorted_pts, sorted_gene);
}

__global__ __launch_bounds__(kBcThreads) void bcount_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                                const double* __restrict__ buffer, int64_t P, int64_t V,
                                                                int64_t* __restrict__ indptr, int64_t* __restrict__ cell_count,
                                                                int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                                int32_t* __restrict__ list_long) {
  bin_rings_body(off, xy, buffer, P, V, indptr, cell_count, words, list_short, list_long);
}

constexpr FrontKernels kBcFront{bcount_keys_kernel, bcount_cells_kernel, bcount_bin_kernel,
                                "bcount_keys_kernel", "bcount_cells_kernel", "bcount_bin_kernel"};

struct CountArgs {
  WalkCommon c;                                                      // join_grid.h
  int n_genes;
  const int32_t* gene;                                               // cell-ordered
  int64_t* indptr;                                                   // count: [p + 1] is written; fill: read
  int64_t* cell_count;                                               // count: written; fill: read
  int32_t* indices;                                                  // fill
  int32_t* counts;                                                   // fill
  int64_t capacity;
  unsigned long long* counters;                                      // count
};

// what a wave adds to the counters once, after its last polygon
struct WaveTotals { unsigned long long pairs = 0, bad = 0, overflow = 0, large = 0; };

// One polygon, one wave, every lane active: r is what rings.h's loops hand over.  hist[0 .. n_genes) is zero on entry and
// on return; `touched` is the wave's list.  kSync orders the wave's LDS traffic (wave_sort.h).
template <bool kFill, class Sync, class Ring>
__device__ __forceinline__ void count_body(const ListedRing<Ring>& r, const CountArgs& a, int32_t* hist, int32_t* touched,
                                           WaveTotals& tot, Sync sync) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = r.p;
  int64_t n_hit = 0, n_good = 0;
  int distinct = 0;                                                  // the same in every lane
  walk_polygon(a.c, r, [&](bool hit, int s, const RingDistance&) {
    const int g = hit ? a.gene[s] : -1;
    const bool good = hit && (unsigned)g < (unsigned)a.n_genes;      // any other gene is never an index
    n_hit += (int64_t)__popcll(__ballot(hit));
    n_good += (int64_t)__popcll(__ballot(good));
    bool fresh = false;
    if (good) fresh = atomicAdd(&hist[g], 1) == 0;                   // two lanes on one gene: one of them sees 0
    const unsigned long long m = __ballot(fresh);
    if (fresh) {
      const int pos = distinct + (int)__popcll(m & ((1ull << lane) - 1));
      if (pos < kTouched) touched[pos] = g;
    }
    distinct += (int)__popcll(m);
  });
  sync();                                                            // hist and the list are complete
  const bool overflow = distinct > kTouched;
  tot.pairs += (unsigned long long)n_hit;
  tot.bad += (unsigned long long)(n_hit - n_good);
  tot.overflow += overflow ? 1u : 0u;
  if (!kFill) {
    if (lane == 0) {
      a.indptr[p + 1] = distinct;
      a.cell_count[p] = n_good;
    }
    if (!overflow) {
      for (int k = lane; k < distinct; k += kWave) hist[touched[k]] = 0;
    } else {
      for (int k = lane; k < a.n_genes; k += kWave) hist[k] = 0;
    }
    sync();
    return;
  }
  const int64_t begin = a.indptr[p];
  int64_t end = a.indptr[p + 1];
  if (end > a.capacity) end = a.capacity;                            // nothing is ever written at or beyond either
  if (!overflow) {
    int padded = 2;
    while (padded < distinct) padded <<= 1;                          // <= kTouched
    for (int k = distinct + lane; k < padded; k += kWave) touched[k] = 0x7fffffff;
    sync();
    wave_bitonic_sort(touched, padded, [](int32_t x, int32_t y) { return x < y; }, sync);
    for (int k = lane; k < distinct; k += kWave) {
      const int g = touched[k];                                      // < n_genes: only in-range genes were appended
      const int64_t slot = begin + k;
      if (slot >= 0 && slot < end) {
        a.indices[slot] = g;
        a.counts[slot] = hist[g];
      }
      hist[g] = 0;
    }
  } else {
    int64_t found = 0;
    for (int base = 0; base < a.n_genes; base += kWave) {            // the ordered scan: gene order by construction
      const int g = base + lane;
      const int c = g < a.n_genes ? hist[g] : 0;
      hit_slot<true>(c > 0, begin, end, found, [&](int64_t slot) { a.indices[slot] = g; a.counts[slot] = c; });
      if (c > 0) hist[g] = 0;
    }
  }
  sync();
  if (lane == 0 && (begin + distinct != a.indptr[p + 1] || begin + distinct > a.capacity || a.cell_count[p] != n_good))
    atomicOr(&a.c.words[kWordFlag], SEGGER_BCOUNT_ERR_FILL);
}

template <bool kFill>
__device__ __forceinline__ void add_totals(const CountArgs& a, const WaveTotals& tot) {
  if (kFill || (threadIdx.x & (kWave - 1)) != 0) return;
  if (tot.pairs) atomicAdd(&a.counters[kCtrPairs], tot.pairs);
  if (tot.bad) atomicAdd(&a.counters[kCtrBad], tot.bad);
  if (tot.overflow) atomicAdd(&a.counters[kCtrOverflow], tot.overflow);
  if (tot.large) atomicAdd(&a.counters[kCtrLarge], tot.large);
}

template <class Sync>
__device__ __forceinline__ void zero_hist(int32_t* hist, int n_genes, Sync sync) {
  for (int k = threadIdx.x & (kWave - 1); k < n_genes; k += kWave) hist[k] = 0;
  sync();
}

template <bool kFill, bool kLarge>
__global__ __launch_bounds__(kLarge ? kWave : kBcThreads) void bcount_short_kernel(CountArgs a, const int32_t* __restrict__ list) {
  constexpr int kWaves = kLarge ? 1 : kBcWaves;
  __shared__ int32_t hist[kWaves][tier_genes(kLarge)];
  __shared__ int32_t touched[kWaves][kTouched];
  const int wave = (int)(threadIdx.x >> 6);
  WaveTotals tot;
  zero_hist(hist[wave], a.n_genes, WaveSync{});
  short_ring_loop(a.c.off, a.c.xy, a.c.words, list, kWaves, [&](const auto& r) {
    count_body<kFill>(r, a, hist[wave], touched[wave], tot, WaveSync{});
    tot.large += kLarge ? 1u : 0u;
  });
  add_totals<kFill>(a, tot);
}

template <bool kFill, bool kLarge>
__global__ __launch_bounds__(kWave) void bcount_long_kernel(CountArgs a, const int32_t* __restrict__ list) {
  __shared__ double2 pts[SEGGER_MORPH_MAX_VERTS];
  __shared__ int32_t hist[tier_genes(kLarge)];
  __shared__ int32_t touched[kTouched];
  WaveTotals tot;
  zero_hist(hist, a.n_genes, BlockSync{});
  long_ring_loop(a.c.off, a.c.xy, a.c.words, list, pts, [&](const auto& r) {
    count_body<kFill>(r, a, hist, touched, tot, BlockSync{});
    tot.large += kLarge ? 1u : 0u;
  });
  add_totals<kFill>(a, tot);
}

// ---------------------------------------------------------------- host ---
using BcLayout = GridLayout;                                         // join_grid.h: the join's layout and, behind it, the genes
using BcCall = GridCall;
constexpr const char* kBcNames8 = "ring_offsets, indptr and buffer";

BcLayout bc_layout(int64_t N, int64_t P, int64_t n_cells) { return grid_layout(N, P, n_cells, true); }

int bc_check_sizes(const char* who, int64_t N, int64_t P, int64_t G, int32_t nx, int32_t ny) {
  const int rc = grid_check_sizes(who, N, P, nx, ny);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(G >= 1 && G <= SEGGER_BCOUNT_MAX_GENES, "%s: n_genes %lld outside 1 .. SEGGER_BCOUNT_MAX_GENES = %d", who, (long long)G,
                 SEGGER_BCOUNT_MAX_GENES);
  return SEGGER_OK;
}

// everything both entry points reject; *empty = nothing to do (no pointer was looked at)
int bc_check(const char* who, const BcCall& c, int64_t G, bool* empty) {
  *empty = false;
  const int rc = bc_check_sizes(who, c.N, c.P, G, c.nx, c.ny);
  return rc != SEGGER_OK ? rc : grid_check(who, c, empty);
}

CountArgs count_args(const BcCall& c, int64_t G, const BcLayout& l) {
  CountArgs a{};
  a.c = walk_common(c, l);
  a.n_genes = (int)G;
  a.gene = at<int32_t>(c.workspace, l.gene);
  a.indptr = const_cast<int64_t*>(c.offsets);
  return a;
}

// the tier's kernels: the small one runs four waves a workgroup on the short route, the large one one
template <bool kFill, bool kLarge>
constexpr RingKernels<CountArgs> kBcRings{bcount_short_kernel<kFill, kLarge>, "bcount_short_kernel", kLarge ? 1 : kBcWaves, kLarge ? 1 : 4,
                                          bcount_long_kernel<kFill, kLarge>, "bcount_long_kernel", kLarge ? 1 : 2};

template <bool kFill>
int launch_polygons(const BcCall& c, const BcLayout& l, const CountArgs& a, hipStream_t stream) {
  return launch_ring_kernels(a.n_genes > SEGGER_BCOUNT_SMALL_GENES ? kBcRings<kFill, true> : kBcRings<kFill, false>, c, l, a, stream);
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_buffered_counts_workspace_bytes(int64_t n_points, int64_t n_polygons, int64_t n_genes, int32_t nx, int32_t ny) {
  const int rc = bc_check_sizes("segger_buffered_counts_workspace_bytes", n_points, n_polygons, n_genes, nx, ny);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)bc_layout(n_points, n_polygons, (int64_t)nx * ny).total;
}

extern "C" int segger_buffered_counts_count(const double* points, int64_t n_points, const int32_t* gene, int64_t n_genes,
                                            const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                            const double* buffer, int32_t predicate, double x0, double y0, double cell, int32_t nx,
                                            int32_t ny, int64_t* indptr, int64_t* cell_count, int64_t* counters, void* workspace,
                                            int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_buffered_counts_count";
  hipStream_t stream = (hipStream_t)stream_;
  const BcCall c = grid_call(points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                             indptr, workspace, workspace_bytes, kBcNames8, true, gene);
  bool empty = false;
  int rc = bc_check(who, c, n_genes, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  SEGGER_REQUIRE(cell_count && counters, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(cell_count, 8) && is_aligned(counters, 8), "%s: cell_count and counters must be 8-byte aligned", who);
  const BcLayout l = bc_layout(n_points, n_polygons, (int64_t)nx * ny);
  CountArgs a = count_args(c, n_genes, l);
  a.cell_count = cell_count;
  a.counters = reinterpret_cast<unsigned long long*>(counters);
  SEGGER_HIP(hipMemsetAsync(counters, 0, SEGGER_BCOUNT_COUNTERS * sizeof(int64_t), stream));
  rc = grid_front(kBcFront, c, l, indptr, cell_count, stream);
  if (rc == SEGGER_OK) rc = launch_polygons<false>(c, l, a, stream);
  return rc != SEGGER_OK ? rc : launch_offsets_scan(indptr, n_polygons, counters + kCtrNnz, stream);
}

extern "C" int segger_buffered_counts_fill(const double* points, int64_t n_points, const int32_t* gene, int64_t n_genes,
                                           const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                           const double* buffer, int32_t predicate, double x0, double y0, double cell, int32_t nx,
                                           int32_t ny, const int64_t* indptr, const int64_t* cell_count, int32_t* indices,
                                           int32_t* counts, int64_t capacity, void* workspace, int64_t workspace_bytes,
                                           segger_stream_t stream_) {
  const char* who = "segger_buffered_counts_fill";
  hipStream_t stream = (hipStream_t)stream_;
  const BcCall c = grid_call(points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                             indptr, workspace, workspace_bytes, kBcNames8, true, gene);
  bool empty = false;
  int rc = bc_check(who, c, n_genes, &empty);
  if (rc == SEGGER_OK) rc = grid_check_capacity(who, capacity, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  SEGGER_REQUIRE(cell_count && indices && counts, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(cell_count, 8), "%s: cell_count must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(indices, 4) && is_aligned(counts, 4), "%s: indices and counts must be 4-byte aligned", who);
  const BcLayout l = bc_layout(n_points, n_polygons, (int64_t)nx * ny);
  CountArgs a = count_args(c, n_genes, l);
  a.cell_count = const_cast<int64_t*>(cell_count);
  a.indices = indices;
  a.counts = counts;
  a.capacity = capacity;
  return launch_polygons<true>(c, l, a, stream);
}
