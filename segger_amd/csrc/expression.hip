// segger_expression_build: the cell x gene count matrix of a segmentation (include/segger_amd.h has the contract).
// A filtered group-by-and-reduce over the deduplicated rows: one 64-bit key per kept row, one stable radix sort with the
// row position as value, a compaction of the run heads, and two segmented reductions over the sorted order (per
// (cell, gene) pair, per cell).  Counts use integer atomics only; every floating-point sum is taken in float64 in an
// order that is a function of the run alone (its rows in ascending row position, its length), never of the launch
// geometry: no floating-point atomics anywhere.
// Per row: 20 bytes streamed in, 12 bytes of key + position through the sort, one 4-byte (similarity) and one 8-byte
// (xy) gather through the sort permutation -- the gathers are the cost to watch; positions ascend inside a run.
#include "common.h"
#include "post_common.h"
#include "sort_config.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace segger {
namespace {

constexpr int kExprThreads = 256;
constexpr int64_t kExprMaxBlocks = 1024;        // grid-stride above 262 144 items: four blocks per CU of the MI355X
constexpr int kExprWaves = kExprThreads / kWave;

// counters block of segger_expression_build
enum { kKept = 0, kNnz = 1, kCellsPresent = 2, kGenesPresent = 3, kBad = 4, kExprCounters = 5 };

// key = (cell << gene_bits) | gene, gene_bits = bit length of n_genes - 1: cell and gene come back with a shift and a
// mask instead of a 64-bit division per row.  The sentinel n_cells << gene_bits is above every real key.
struct ExprKeying {
  int gene_bits;
  unsigned long long sentinel;
};

ExprKeying expr_keying(int64_t n_cells, int64_t n_genes) {
  ExprKeying k;
  k.gene_bits = bit_length((unsigned long long)(n_genes - 1));
  k.sentinel = (unsigned long long)n_cells << k.gene_bits;       // n_cells, n_genes < 2^31: below 2^62
  return k;
}

// One key per row; the rows that are not kept take the sentinel and sort behind every kept row.  A kept row whose cell
// or gene is out of range is counted and never used as an index.
__global__ __launch_bounds__(kExprThreads) void expression_keys_kernel(
    const int32_t* __restrict__ cell, const int32_t* __restrict__ gene, const float* __restrict__ sim,
    const double* __restrict__ thr, int64_t n, int64_t n_cells, int64_t n_genes, ExprKeying kg,
    uint64_t* __restrict__ keys, int32_t* __restrict__ pos, int32_t* __restrict__ cell_present,
    int32_t* __restrict__ gene_present, unsigned long long* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kExprThreads;
  int n_kept = 0, n_bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kExprThreads + threadIdx.x; i < n; i += stride) {
    const int32_t c = cell[i];
    const int32_t g = gene[i];
    const bool kept = c >= 0 && (double)sim[i] >= thr[i];        // false when either side is NaN
    const bool in_range = (int64_t)c < n_cells && g >= 0 && (int64_t)g < n_genes;
    unsigned long long key = kg.sentinel;
    if (kept && in_range) {
      key = ((unsigned long long)(uint32_t)c << kg.gene_bits) | (unsigned long long)(uint32_t)g;
      cell_present[c] = 1;                                       // every writer stores the same value
      gene_present[g] = 1;
      ++n_kept;
    }
    n_bad += (kept && !in_range) ? 1 : 0;
    keys[i] = key;
    pos[i] = (int32_t)i;
  }
  n_kept = wave_sum_i32(n_kept);                            // at most 2^31 / (1024 * 256) + 1 rows per thread
  n_bad = wave_sum_i32(n_bad);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (n_kept) atomicAdd(counters + kKept, (unsigned long long)n_kept);
    if (n_bad) atomicAdd(counters + kBad, (unsigned long long)n_bad);
  }
}

// position p of the sorted order starts a run: a real key that differs from its predecessor's
struct ExprRunHead {
  const uint64_t* keys;
  uint64_t sentinel;
  __host__ __device__ bool operator()(const int32_t& p) const {
    const uint64_t k = keys[p];
    return k < sentinel && (p == 0 || keys[p - 1] != k);
  }
};

// cell_pos / gene_pos are the exclusive scans of the present flags: the compacted id lists and their sizes
__global__ __launch_bounds__(kExprThreads) void expression_ids_kernel(
    const int32_t* __restrict__ cell_present, const int32_t* __restrict__ cell_pos, int64_t n_cells,
    const int32_t* __restrict__ gene_present, const int32_t* __restrict__ gene_pos, int64_t n_genes,
    int32_t* __restrict__ cell_ids, int32_t* __restrict__ gene_ids, unsigned long long* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kExprThreads;
  const int64_t n = n_cells > n_genes ? n_cells : n_genes;
  for (int64_t i = (int64_t)blockIdx.x * kExprThreads + threadIdx.x; i < n; i += stride) {
    if (i < n_cells) {
      if (cell_present[i]) cell_ids[cell_pos[i]] = (int32_t)i;
      if (i == n_cells - 1) counters[kCellsPresent] = (unsigned long long)(cell_pos[i] + cell_present[i]);
    }
    if (i < n_genes) {
      if (gene_present[i]) gene_ids[gene_pos[i]] = (int32_t)i;
      if (i == n_genes - 1) counters[kGenesPresent] = (unsigned long long)(gene_pos[i] + gene_present[i]);
    }
  }
}

// Sum of src[pos[p]] (NC floats per row) over p in [beg, beg + len) of the sorted order, by one whole wave, in float64.
// Lane l adds the elements beg + l, beg + l + 64, ... in that order and the 64 partial sums are added in a fixed
// butterfly: the shape of the sum depends on len alone.  Every lane returns the total.
template <int NC>
__device__ __forceinline__ void expr_wave_run_sum(const float* __restrict__ src, const int32_t* __restrict__ pos,
                                                  int32_t beg, int32_t len, int lane, double (&acc)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  const int64_t end = (int64_t)beg + len;
#pragma unroll 4
  for (int64_t p = (int64_t)beg + lane; p < end; p += kWave) {
    const int64_t row = (int64_t)pos[p];
    if constexpr (NC == 2) {
      const float2 v = reinterpret_cast<const float2*>(src)[row];
      acc[0] += (double)v.x;
      acc[1] += (double)v.y;
    } else {
      acc[0] += (double)src[row];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += __shfl_xor(acc[c], m, kWave);
  }
}

// the same sum by one lane, first row to last: runs of at most a wave's width
template <int NC>
__device__ __forceinline__ void expr_lane_run_sum(const float* __restrict__ src, const int32_t* __restrict__ pos,
                                                  int32_t beg, int32_t len, double (&acc)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  for (int32_t j = 0; j < len; ++j) {
    const int64_t row = (int64_t)pos[(int64_t)beg + j];
    if constexpr (NC == 2) {
      const float2 v = reinterpret_cast<const float2*>(src)[row];
      acc[0] += (double)v.x;
      acc[1] += (double)v.y;
    } else {
      acc[0] += (double)src[row];
    }
  }
}

// Segments [seg_beg(s), seg_beg(s + 1)) of the sorted order, 64 consecutive segments per wave: every lane sums its own
// segment when it is short (len <= 64), then the wave takes the long ones of its 64 one after the other.  The lane that
// owns segment s calls emit(s, len, sums) exactly once.  Which path a segment takes depends on its length alone.
template <int NC, typename SegBeg, typename Emit>
__device__ __forceinline__ void expr_segmented_sum(const float* __restrict__ src, const int32_t* __restrict__ pos,
                                                   int64_t n_seg, SegBeg seg_beg, Emit emit) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * kExprWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kExprWaves;
  for (int64_t base = wave * kWave; base < n_seg; base += n_waves * kWave) {        // wave-uniform bounds
    const int64_t s = base + lane;
    int32_t beg = 0, len = 0;
    if (s < n_seg) {
      beg = seg_beg(s);
      len = seg_beg(s + 1) - beg;
    }
    double acc[NC];
    const bool is_long = len > kWave;
    if (s < n_seg && !is_long) {
      if (src) expr_lane_run_sum<NC>(src, pos, beg, len, acc);
      emit(s, len, acc);
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
      const int owner = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t b = __shfl(beg, owner, kWave);
      const int32_t l = __shfl(len, owner, kWave);
      if (src) expr_wave_run_sum<NC>(src, pos, b, l, lane, acc);
      if (lane == owner) emit(s, len, acc);
    }
  }
}

// One run = one (cell, gene) pair = one stored entry of the matrix: its column, its count, its mean similarity; the
// first run of a cell sets the cell's row pointer.  run_start [nnz] comes from the compaction; the last run ends at n_kept.
__global__ __launch_bounds__(kExprThreads) void expression_pairs_kernel(
    const uint64_t* __restrict__ keys, const int32_t* __restrict__ pos, const int32_t* __restrict__ run_start,
    const float* __restrict__ sim, const int32_t* __restrict__ cell_pos, const int32_t* __restrict__ gene_pos,
    ExprKeying kg, const unsigned long long* __restrict__ counters, int64_t* __restrict__ indptr,
    int32_t* __restrict__ indices, int32_t* __restrict__ counts, double* __restrict__ mean_similarity) {
  const int64_t nnz = (int64_t)counters[kNnz];
  const int32_t n_kept = (int32_t)counters[kKept];
  if (blockIdx.x == 0 && threadIdx.x == 0) indptr[counters[kCellsPresent]] = nnz;   // also indptr[0] = 0 of an empty matrix
  const uint64_t gene_mask = ((uint64_t)1 << kg.gene_bits) - 1;
  expr_segmented_sum<1>(
      sim, pos, nnz, [&](int64_t r) { return r < nnz ? run_start[r] : n_kept; },
      [&](int64_t r, int32_t len, const double (&sum)[1]) {
        const uint64_t key = keys[run_start[r]];
        const uint64_t c = key >> kg.gene_bits;
        indices[r] = gene_pos[key & gene_mask];
        counts[r] = len;
        mean_similarity[r] = sum[0] / (double)len;
        if (r == 0 || (keys[run_start[r - 1]] >> kg.gene_bits) != c) indptr[cell_pos[c]] = r;
      });
}

// One segment = the runs of one present cell = rows [run_start[indptr[j]], run_start[indptr[j + 1]]) of the sorted order
// (gene by gene, ascending row position inside a gene): the cell's row count and, when xy is given, its mean position.
__global__ __launch_bounds__(kExprThreads) void expression_cells_kernel(
    const int32_t* __restrict__ pos, const int32_t* __restrict__ run_start, const int64_t* __restrict__ indptr,
    const float* __restrict__ xy, const unsigned long long* __restrict__ counters, int64_t* __restrict__ cell_count,
    double* __restrict__ centroid) {
  const int64_t nnz = (int64_t)counters[kNnz];
  const int32_t n_kept = (int32_t)counters[kKept];
  const int64_t n_present = (int64_t)counters[kCellsPresent];
  expr_segmented_sum<2>(
      xy, pos, n_present,
      [&](int64_t j) {
        const int64_t r = indptr[j];
        return r < nnz ? run_start[r] : n_kept;
      },
      [&](int64_t j, int32_t len, const double (&sum)[2]) {
        cell_count[j] = (int64_t)len;
        if (xy) {
          centroid[2 * j] = sum[0] / (double)len;
          centroid[2 * j + 1] = sum[1] / (double)len;
        }
      });
}

unsigned expr_grid(int64_t n_items) { return grid_stride_blocks(n_items, kExprThreads, kExprMaxBlocks); }

int expr_check_sizes(const char* who, int64_t n_rows, int64_t n_cells, int64_t n_genes) {
  SEGGER_REQUIRE(n_rows >= 0, "%s: negative n_rows", who);
  SEGGER_REQUIRE(n_rows <= 0x7fffffffLL, "%s: 2^31 rows or more", who);
  SEGGER_REQUIRE(n_cells >= 1, "%s: n_cells must be at least 1", who);
  SEGGER_REQUIRE(n_genes >= 1, "%s: n_genes must be at least 1", who);
  SEGGER_REQUIRE(n_cells <= INT64_MAX / n_genes, "%s: n_cells * n_genes overflows 63 bits", who);
  SEGGER_REQUIRE(n_cells <= 0x7fffffffLL && n_genes <= 0x7fffffffLL, "%s: cell and gene ids are int32: n_cells and n_genes "
                 "must be below 2^31", who);
  return SEGGER_OK;
}

struct ExprLayout {
  size_t keys_a, keys_b, pos_a, pos_b, run_start, cell_present, cell_pos, gene_present, gene_pos, temp, total;
  size_t temp_bytes;
  int key_bits;
};

ExprLayout expr_layout(int64_t n_rows, int64_t n_cells, int64_t n_genes) {
  ExprLayout L;
  const ExprKeying kg = expr_keying(n_cells, n_genes);
  L.key_bits = bit_length(kg.sentinel);
  const size_t n = (size_t)(n_rows > 0 ? n_rows : 1);
  Carver ws;
  L.keys_a = ws.take(n * 8);
  L.keys_b = ws.take(n * 8);
  L.pos_a = ws.take(n * 4);
  L.pos_b = ws.take(n * 4);
  L.run_start = ws.take(n * 4);
  L.cell_present = ws.take((size_t)n_cells * 4);
  L.cell_pos = ws.take((size_t)n_cells * 4);
  L.gene_present = ws.take((size_t)n_genes * 4);
  L.gene_pos = ws.take((size_t)n_genes * 4);
  size_t a = 0, b = 0, c = 0, d = 0;
  uint64_t* k64 = nullptr;
  int32_t* v32 = nullptr;
  int32_t* i32 = nullptr;
  size_t* cnt = nullptr;
  (void)rocprim::radix_sort_pairs<NoScratchSortConfig>(nullptr, a, k64, k64, v32, v32, n, 0, (unsigned)L.key_bits, (hipStream_t)0);
  (void)rocprim::select(nullptr, b, rocprim::counting_iterator<int32_t>(0), i32, cnt, n, ExprRunHead{nullptr, 0}, (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, c, i32, i32, (int32_t)0, (size_t)n_cells, rocprim::plus<int32_t>(), (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, d, i32, i32, (int32_t)0, (size_t)n_genes, rocprim::plus<int32_t>(), (hipStream_t)0);
  L.temp_bytes = a;
  if (b > L.temp_bytes) L.temp_bytes = b;
  if (c > L.temp_bytes) L.temp_bytes = c;
  if (d > L.temp_bytes) L.temp_bytes = d;
  L.temp = ws.take(L.temp_bytes > 0 ? L.temp_bytes : 1);
  L.total = ws.total();
  return L;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_expression_workspace_bytes(int64_t n_rows, int64_t n_cells, int64_t n_genes) {
  const int rc = expr_check_sizes("segger_expression_workspace_bytes", n_rows, n_cells, n_genes);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)expr_layout(n_rows, n_cells, n_genes).total;
}

extern "C" int segger_expression_build(const int32_t* cell, const int32_t* gene, const float* similarity,
                                       const double* threshold, const float* xy, int64_t n_rows, int64_t n_cells,
                                       int64_t n_genes, int32_t* cell_ids, int32_t* gene_ids, int64_t* indptr,
                                       int32_t* indices, int32_t* counts, double* mean_similarity, int64_t* cell_count,
                                       double* centroid, uint64_t* counters, void* workspace, size_t workspace_bytes,
                                       segger_stream_t stream_) {
  const char* who = "segger_expression_build";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = expr_check_sizes(who, n_rows, n_cells, n_genes);
  if (rc != SEGGER_OK) return rc;
  if (n_rows == 0) {                               // nothing launched: the caller's zeroed counters and indptr[0] stand
    SEGGER_REQUIRE(counters && indptr, "%s: NULL pointer", who);
    return SEGGER_OK;
  }
  SEGGER_REQUIRE(cell && gene && similarity && threshold && cell_ids && gene_ids && indptr && indices && counts &&
                     mean_similarity && cell_count && counters && workspace, "%s: NULL pointer", who);
  SEGGER_REQUIRE((xy == nullptr) == (centroid == nullptr), "%s: xy and centroid are given together or not at all", who);
  SEGGER_REQUIRE(is_aligned(threshold, 8) && is_aligned(xy, 8) && is_aligned(indptr, 8) &&
                     is_aligned(mean_similarity, 8) && is_aligned(cell_count, 8) && is_aligned(centroid, 8) &&
                     is_aligned(counters, 8),
                 "%s: threshold, xy, indptr, mean_similarity, cell_count, centroid and counters must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(cell, 4) && is_aligned(gene, 4) && is_aligned(similarity, 4) && is_aligned(cell_ids, 4) &&
                     is_aligned(gene_ids, 4) && is_aligned(indices, 4) && is_aligned(counts, 4),
                 "%s: cell, gene, similarity, cell_ids, gene_ids, indices and counts must be 4-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  const ExprLayout L = expr_layout(n_rows, n_cells, n_genes);
  if (workspace_bytes < L.total) return workspace_too_small(who, workspace_bytes, L.total);

  uint64_t* keys_a = at<uint64_t>(workspace, L.keys_a);     // uint64 keys, int32 values: the pair quadtree.hip sorts
  uint64_t* keys_b = at<uint64_t>(workspace, L.keys_b);
  int32_t* pos_a = at<int32_t>(workspace, L.pos_a);
  int32_t* pos_b = at<int32_t>(workspace, L.pos_b);
  int32_t* run_start = at<int32_t>(workspace, L.run_start);
  int32_t* cell_present = at<int32_t>(workspace, L.cell_present);
  int32_t* cell_pos = at<int32_t>(workspace, L.cell_pos);
  int32_t* gene_present = at<int32_t>(workspace, L.gene_present);
  int32_t* gene_pos = at<int32_t>(workspace, L.gene_pos);
  void* temp = at<char>(workspace, L.temp);
  size_t temp_bytes = L.temp_bytes;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  const ExprKeying kg = expr_keying(n_cells, n_genes);

  SEGGER_HIP(hipMemsetAsync(cnt, 0, kExprCounters * sizeof(unsigned long long), stream));
  SEGGER_HIP(hipMemsetAsync(cell_present, 0, (size_t)n_cells * 4, stream));
  SEGGER_HIP(hipMemsetAsync(gene_present, 0, (size_t)n_genes * 4, stream));
  hipLaunchKernelGGL(expression_keys_kernel, dim3(expr_grid(n_rows)), dim3(kExprThreads), 0, stream, cell, gene, similarity,
                     threshold, n_rows, n_cells, n_genes, kg, keys_a, pos_a, cell_present, gene_present, cnt);
  SEGGER_LAUNCH_CHECK("expression_keys_kernel");
  SEGGER_HIP(rocprim::radix_sort_pairs<NoScratchSortConfig>(temp, temp_bytes, keys_a, keys_b, pos_a, pos_b, (size_t)n_rows, 0,
                                                       (unsigned)L.key_bits, stream));
  temp_bytes = L.temp_bytes;
  SEGGER_HIP(rocprim::select(temp, temp_bytes, rocprim::counting_iterator<int32_t>(0), run_start,
                             reinterpret_cast<size_t*>(cnt + kNnz), (size_t)n_rows, ExprRunHead{keys_b, kg.sentinel}, stream));
  temp_bytes = L.temp_bytes;
  SEGGER_HIP(rocprim::exclusive_scan(temp, temp_bytes, cell_present, cell_pos, (int32_t)0, (size_t)n_cells,
                                     rocprim::plus<int32_t>(), stream));
  temp_bytes = L.temp_bytes;
  SEGGER_HIP(rocprim::exclusive_scan(temp, temp_bytes, gene_present, gene_pos, (int32_t)0, (size_t)n_genes,
                                     rocprim::plus<int32_t>(), stream));
  const int64_t n_ids = n_cells > n_genes ? n_cells : n_genes;
  hipLaunchKernelGGL(expression_ids_kernel, dim3(expr_grid(n_ids)), dim3(kExprThreads), 0, stream,
                     (const int32_t*)cell_present, (const int32_t*)cell_pos, n_cells, (const int32_t*)gene_present,
                     (const int32_t*)gene_pos, n_genes, cell_ids, gene_ids, cnt);
  SEGGER_LAUNCH_CHECK("expression_ids_kernel");
  // one lane per run / per present cell; the device-side counts decide which lanes work
  hipLaunchKernelGGL(expression_pairs_kernel, dim3(expr_grid(n_rows)), dim3(kExprThreads), 0, stream,
                     (const uint64_t*)keys_b, (const int32_t*)pos_b, (const int32_t*)run_start, similarity,
                     (const int32_t*)cell_pos, (const int32_t*)gene_pos, kg, (const unsigned long long*)cnt, indptr, indices,
                     counts, mean_similarity);
  SEGGER_LAUNCH_CHECK("expression_pairs_kernel");
  const int64_t cell_cap = n_rows < n_cells ? n_rows : n_cells;
  hipLaunchKernelGGL(expression_cells_kernel, dim3(expr_grid(cell_cap)), dim3(kExprThreads), 0, stream,
                     (const int32_t*)pos_b, (const int32_t*)run_start, (const int64_t*)indptr, xy,
                     (const unsigned long long*)cnt, cell_count, centroid);
  SEGGER_LAUNCH_CHECK("expression_cells_kernel");
  return SEGGER_OK;
}
