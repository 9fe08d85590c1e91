// segger_thresholds_build: the per-gene similarity thresholds min(Yen, Li) over the assigned rows of a segmentation
// (include/segger_amd.h has the contract; postprocess.per_gene_thresholds is the torch form of the same algorithms).
// One 64-bit key per row, (gene << 32) | ord(similarity), and one keys-only radix sort: the sorted key array is the data
// (gene in the high word, the value back from the low word), so there is no value array, no permutation, and the result
// is a function of the multiset of rows -- the same bits for any order of the input.  Every floating-point sum is
// float64 in an order fixed by the sorted positions (chunks of kThrChunk positions, a fixed tree inside a chunk, a
// sequential prefix over a gene's chunks); the only atomics are integer (counters, the minimum gap as a bit pattern).
// Per row: 12 bytes streamed in, 8 bytes of key through the sort, two streaming reads of the sorted keys; per gene one
// workgroup: 255 binary searches for Yen's histogram, and per Li iteration one binary search plus a sum of < kThrChunk rows.
#include "common.h"
#include "post_common.h"
#include "sort_config.h"

// numpy rounds every product before it adds: a fused multiply-add would move a bin edge by an ulp past a value that sits on it
#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kThrThreads = 256;
constexpr int kThrWaves = kThrThreads / kWave;
constexpr int64_t kThrMaxBlocks = 1024;         // grid-stride above 262 144 items: four blocks per CU of the MI355X
constexpr int64_t kThrChunk = SEGGER_THRESHOLDS_CHUNK;
constexpr int kThrBins = 256;
constexpr uint32_t kThrNoGene = 0xffffffffu;    // high word of the sentinel key: above every gene id (ids are < 2^31)
constexpr unsigned long long kThrSentinel = ~0ull;
constexpr unsigned long long kThrInfBits = 0x7ff0000000000000ull;

// counters block of segger_thresholds_build
enum { kThrAssigned = 0, kThrGenesPresent = 1, kThrBad = 2, kThrNan = 3, kThrCounters = 4 };

// similarity bits -> unsigned order: the same mapping as ordered_bits (post_common.h) -- -0.0 sorts just below +0.0 as a
// key of its own, and a NaN never gets here -- written as one xor.  It stays a function of this file because the
// compiler turns the two spellings into different code: with ordered_bits the row loop of thresholds_keys_kernel gains
// a branch and four SGPRs.
__device__ __forceinline__ uint32_t thr_ord(float s) {
  const uint32_t b = __float_as_uint(s);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ double thr_value(unsigned long long key) {
  const uint32_t ord = (uint32_t)key;
  return (double)__uint_as_float((ord >> 31) ? (ord ^ 0x80000000u) : ~ord);
}

__device__ __forceinline__ uint32_t thr_gene(unsigned long long key) { return (uint32_t)(key >> 32); }

// One key per row; unassigned and rejected rows take the sentinel and sort behind every real key.  An assigned row with a
// gene outside [0, n_genes) or a NaN similarity is counted and never used as an index.  The same grid initialises the
// per-gene segment table: beg = end = 0 (absent), gap = +inf.
__global__ __launch_bounds__(kThrThreads) void thresholds_keys_kernel(
    const float* __restrict__ sim, const int32_t* __restrict__ gene, const int32_t* __restrict__ cell, int64_t n,
    int64_t n_genes, unsigned long long* __restrict__ keys, int32_t* __restrict__ beg, int32_t* __restrict__ end,
    unsigned long long* __restrict__ gap, unsigned long long* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kThrThreads;
  const int64_t first = (int64_t)blockIdx.x * kThrThreads + threadIdx.x;
  for (int64_t g = first; g < n_genes; g += stride) {
    beg[g] = 0;
    end[g] = 0;
    gap[g] = kThrInfBits;
  }
  int n_ok = 0, n_bad = 0, n_nan = 0;
  for (int64_t i = first; i < n; i += stride) {
    const int32_t g = gene[i];
    const float s = sim[i];
    const bool assigned = cell[i] >= 0;
    const bool in_range = g >= 0 && (int64_t)g < n_genes;
    const bool is_nan = s != s;
    const bool ok = assigned && in_range && !is_nan;
    keys[i] = ok ? (((unsigned long long)(uint32_t)g << 32) | (unsigned long long)thr_ord(s)) : kThrSentinel;
    n_ok += ok ? 1 : 0;
    n_bad += (assigned && !in_range) ? 1 : 0;
    n_nan += (assigned && in_range && is_nan) ? 1 : 0;
  }
  n_ok = wave_sum_i32(n_ok);                                 // at most 2^31 / (1024 * 256) + 1 rows per thread
  n_bad = wave_sum_i32(n_bad);
  n_nan = wave_sum_i32(n_nan);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (n_ok) atomicAdd(counters + kThrAssigned, (unsigned long long)n_ok);
    if (n_bad) atomicAdd(counters + kThrBad, (unsigned long long)n_bad);
    if (n_nan) atomicAdd(counters + kThrNan, (unsigned long long)n_nan);
  }
}

// beg[g] / end[g] of every present gene from adjacent high words of the sorted keys: one writer per slot
__global__ __launch_bounds__(kThrThreads) void thresholds_segments_kernel(
    const unsigned long long* __restrict__ keys, int64_t n, int32_t* __restrict__ beg, int32_t* __restrict__ end,
    unsigned long long* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kThrThreads;
  int n_present = 0;
  for (int64_t p = (int64_t)blockIdx.x * kThrThreads + threadIdx.x; p < n; p += stride) {
    const uint32_t g = thr_gene(keys[p]);
    if (g == kThrNoGene) continue;
    if (p == 0 || thr_gene(keys[p - 1]) != g) {
      beg[g] = (int32_t)p;
      ++n_present;
    }
    if (p == n - 1 || thr_gene(keys[p + 1]) != g) end[g] = (int32_t)(p + 1);
  }
  n_present = wave_sum_i32(n_present);
  if ((threadIdx.x & (kWave - 1)) == 0 && n_present) atomicAdd(counters + kThrGenesPresent, (unsigned long long)n_present);
}

// Sum of value - vmin over the sorted positions [lo, hi), float64, by one whole workgroup: thread t adds the positions
// lo + t, lo + t + 256, ... in that order, the 64 lanes of a wave meet in a fixed butterfly and the four wave sums are
// added first to last.  The shape of the sum depends on (lo, hi) alone; every thread returns the total.
__device__ __forceinline__ double thr_block_range_sum(const unsigned long long* __restrict__ keys, int64_t lo, int64_t hi,
                                                      double vmin, double* red) {
  double acc = 0.0;
  for (int64_t p = lo + threadIdx.x; p < hi; p += kThrThreads) acc += thr_value(keys[p]) - vmin;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < kThrWaves; ++w) s += red[w];
  __syncthreads();                                               // red is free for the next call
  return s;
}

// One workgroup per chunk of kThrChunk sorted positions.  Every position with a predecessor of the same gene and a
// different key offers its gap (of the values shifted by the gene's minimum, as Li sees them) to the gene's minimum: an
// integer min over the bit patterns of positive doubles, whose result no order of arrival changes.  A chunk that lies
// inside one gene leaves its sum; the partial chunks at a gene's ends are summed by the gene's own workgroup.
__global__ __launch_bounds__(kThrThreads) void thresholds_chunks_kernel(
    const unsigned long long* __restrict__ keys, int64_t n, const int32_t* __restrict__ beg,
    unsigned long long* __restrict__ gap, double* __restrict__ chunk_sum) {
  __shared__ double red[kThrWaves];
  const int64_t n_chunks = (n + kThrChunk - 1) / kThrChunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t lo = c * kThrChunk;
    const int64_t hi = lo + kThrChunk < n ? lo + kThrChunk : n;
    for (int64_t p = lo + threadIdx.x; p < hi; p += kThrThreads) {
      const unsigned long long k = keys[p];
      const uint32_t g = thr_gene(k);
      if (g == kThrNoGene || p == 0) continue;
      const unsigned long long kp = keys[p - 1];
      if (thr_gene(kp) != g || kp == k) continue;
      const double vmin = thr_value(keys[beg[g]]);
      const double d = (thr_value(k) - vmin) - (thr_value(kp) - vmin);
      if (d > 0.0) {                                             // -0.0 and +0.0 are two keys with no gap between them
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
        // a stale read is only ever too large: the atomic is skipped when it could not lower the minimum anyway
        if (bits < __hip_atomic_load(gap + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(gap + g, bits);
      }
    }
    const uint32_t g0 = thr_gene(keys[lo]);
    if (hi - lo == kThrChunk && g0 != kThrNoGene && thr_gene(keys[hi - 1]) == g0) {       // the same for every thread
      const double s = thr_block_range_sum(keys, lo, hi, thr_value(keys[beg[g0]]), red);
      if (threadIdx.x == 0) chunk_sum[c] = s;
    }
  }
}

// numpy.linspace(lo, hi, 257)[i]
__device__ __forceinline__ double thr_edge(int i, double lo, double hi, double step) {
  return i == kThrBins ? hi : lo + (double)i * step;
}

// One workgroup per gene, every gene in one launch.  All 256 threads follow the same control flow on the same values
// (they read the same keys and the same shared sums), so every branch below is uniform.
__global__ __launch_bounds__(kThrThreads) void thresholds_genes_kernel(
    const unsigned long long* __restrict__ keys, const int32_t* __restrict__ beg, const int32_t* __restrict__ end,
    const unsigned long long* __restrict__ gap, double* __restrict__ chunk_sum, int64_t n_genes, int32_t max_iter,
    double* __restrict__ threshold, double* __restrict__ yen_out, double* __restrict__ li_out, int64_t* __restrict__ count,
    uint8_t* __restrict__ converged) {
  __shared__ int32_t below[kThrBins + 1];          // below[i]: values of the gene under edge i
  __shared__ double p1[kThrBins], p1_sq[kThrBins], p2_sq[kThrBins], crit[kThrBins];
  __shared__ double red[kThrWaves];
  __shared__ double mid_total;
  const int tid = threadIdx.x;
  for (int64_t g = blockIdx.x; g < n_genes; g += gridDim.x) {
    const int64_t b = beg[g], e = end[g];
    const int64_t n = e - b;
    if (n == 0) {                                  // no assigned row
      if (tid == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        threshold[g] = nan;
        yen_out[g] = nan;
        li_out[g] = nan;
        count[g] = 0;
        converged[g] = 1;
      }
      continue;
    }
    const double vmin = thr_value(keys[b]), vmax = thr_value(keys[e - 1]);
    const bool flat = vmin == vmax;

    // ---- Yen: 256 bins over [lo, hi]; value v is in bin i iff edge_i <= v < edge_{i+1}, the last bin closed, so the
    // counts are differences of the positions of the edges in the sorted segment
    const double lo = flat ? vmin - 0.5 : vmin, hi = flat ? vmax + 0.5 : vmax;
    const double step = (hi - lo) / (double)kThrBins;
    if (tid == 0) {
      below[0] = 0;
      below[kThrBins] = (int32_t)n;
    } else {
      const double edge = lo + (double)tid * step;
      int64_t l = b, r = e;                        // first position whose value is >= edge
      while (l < r) {
        const int64_t m = l + ((r - l) >> 1);
        if (thr_value(keys[m]) < edge) l = m + 1; else r = m;
      }
      below[tid] = (int32_t)(l - b);
    }
    __syncthreads();
    if (tid == 0) {                                // the running sums of numpy.cumsum, first bin to last ...
      double run = 0.0, run_sq = 0.0;
      for (int i = 0; i < kThrBins; ++i) {
        const double pmf = (double)(below[i + 1] - below[i]) / (double)n;
        run += pmf;
        run_sq += pmf * pmf;
        p1[i] = run;
        p1_sq[i] = run_sq;
      }
    } else if (tid == kWave) {                     // ... and last bin to first, by a lane of another wave
      double run_sq = 0.0;
      for (int i = kThrBins - 1; i >= 0; --i) {
        const double pmf = (double)(below[i + 1] - below[i]) / (double)n;
        run_sq += pmf * pmf;
        p2_sq[i] = run_sq;
      }
    }
    __syncthreads();
    if (tid < kThrBins - 1) {
      const double q = p1[tid] * (1.0 - p1[tid]);
      crit[tid] = log((1.0 / (p1_sq[tid] * p2_sq[tid + 1])) * (q * q));
    }
    __syncthreads();
    int k = 0;                                     // numpy.argmax: the first NaN, else the first maximum
    {
      double best = crit[0];
      for (int i = 1; i < kThrBins - 1 && best == best; ++i) {
        const double c = crit[i];
        if (c != c || c > best) {
          best = c;
          k = i;
        }
      }
    }
    const double yen = (thr_edge(k, lo, hi, step) + thr_edge(k + 1, lo, hi, step)) / 2.0;

    // ---- Li on the values shifted by vmin: t <- (mean_back - mean_fore) / (log mean_back - log mean_fore)
    double li = vmin;
    bool failed = false;
    if (!flat) {
      const int64_t c0 = (b + kThrChunk - 1) / kThrChunk, c1 = e / kThrChunk;       // whole chunks of the gene: [c0, c1)
      const bool interior = c0 < c1;
      double head = 0.0;
      if (interior) {
        if (tid == 0) {                            // chunk sums -> exclusive prefix, first chunk to last
          double run = 0.0;
          for (int64_t c = c0; c < c1; ++c) {
            const double s = chunk_sum[c];
            chunk_sum[c] = run;
            run += s;
          }
          mid_total = run;
        }
        __syncthreads();
        head = thr_block_range_sum(keys, b, c0 * kThrChunk, vmin, red);
      }
      auto sum_below = [&](int64_t pos) -> double {                                  // sum over [b, pos)
        if (!interior || pos <= c0 * kThrChunk) return thr_block_range_sum(keys, b, pos, vmin, red);
        if (pos >= c1 * kThrChunk) return (head + mid_total) + thr_block_range_sum(keys, c1 * kThrChunk, pos, vmin, red);
        const int64_t c = pos / kThrChunk;
        return (head + chunk_sum[c]) + thr_block_range_sum(keys, c * kThrChunk, pos, vmin, red);
      };
      const double total = sum_below(e);
      const double tol = __longlong_as_double((long long)gap[g]) / 2.0;
      double t_next = total / (double)n, t_curr = -2.0 * tol;
      int32_t calls = 1;
      while (fabs(t_next - t_curr) > tol) {
        t_curr = t_next;
        int64_t l = b, r = e;                      // first position whose shifted value is > t_curr
        while (l < r) {
          const int64_t m = l + ((r - l) >> 1);
          if (thr_value(keys[m]) - vmin <= t_curr) l = m + 1; else r = m;
        }
        const double n_back = (double)(l - b);
        const double below_sum = sum_below(l);
        const double mean_back = below_sum / n_back;
        const double mean_fore = (total - below_sum) / ((double)n - n_back);
        if (mean_back == 0.0) break;
        t_next = (mean_back - mean_fore) / (log(mean_back) - log(mean_fore));
        if (++calls > max_iter) {
          failed = true;
          break;
        }
      }
      li = t_next + vmin;
    }
    if (tid == 0) {
      threshold[g] = li < yen ? li : yen;
      yen_out[g] = yen;
      li_out[g] = li;
      count[g] = n;
      converged[g] = failed ? 0 : 1;
    }
    __syncthreads();                               // the shared tables are free for the next gene
  }
}

// n_rows == 0: every gene is absent
__global__ __launch_bounds__(kThrThreads) void thresholds_absent_kernel(int64_t n_genes, double* __restrict__ threshold,
                                                                        double* __restrict__ yen, double* __restrict__ li,
                                                                        int64_t* __restrict__ count,
                                                                        uint8_t* __restrict__ converged) {
  const int64_t stride = (int64_t)gridDim.x * kThrThreads;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t g = (int64_t)blockIdx.x * kThrThreads + threadIdx.x; g < n_genes; g += stride) {
    threshold[g] = nan;
    yen[g] = nan;
    li[g] = nan;
    count[g] = 0;
    converged[g] = 1;
  }
}

unsigned thr_grid(int64_t n_items) { return grid_stride_blocks(n_items, kThrThreads, kThrMaxBlocks); }

int thr_check_sizes(const char* who, int64_t n_rows, int64_t n_genes) {
  SEGGER_REQUIRE(n_rows >= 0, "%s: negative n_rows", who);
  SEGGER_REQUIRE(n_rows <= 0x7fffffffLL, "%s: 2^31 rows or more", who);
  SEGGER_REQUIRE(n_genes >= 1, "%s: n_genes must be at least 1", who);
  SEGGER_REQUIRE(n_genes <= 0x7fffffffLL, "%s: gene ids are int32: n_genes must be below 2^31", who);
  return SEGGER_OK;
}

struct ThrLayout {
  size_t keys_a, keys_b, beg, end, gap, chunk_sum, temp, total;
  size_t temp_bytes;
  int key_bits;
};

// with n_rows and n_genes below 2^31 every term is below 2^36 bytes: nothing here can overflow
ThrLayout thr_layout(int64_t n_rows, int64_t n_genes) {
  ThrLayout L;
  L.key_bits = 32 + bit_length((unsigned long long)n_genes);   // the sentinel is all ones in these bits, above every gene
  const size_t n = (size_t)(n_rows > 0 ? n_rows : 1);
  Carver ws;
  L.keys_a = ws.take(n * 8);
  L.keys_b = ws.take(n * 8);
  L.beg = ws.take((size_t)n_genes * 4);
  L.end = ws.take((size_t)n_genes * 4);
  L.gap = ws.take((size_t)n_genes * 8);
  L.chunk_sum = ws.take((n + (size_t)kThrChunk - 1) / (size_t)kThrChunk * 8);
  size_t a = 0;
  unsigned long long* k64 = nullptr;
  (void)rocprim::radix_sort_keys<NoScratchSortConfig>(nullptr, a, k64, k64, n, 0, (unsigned)L.key_bits, (hipStream_t)0);
  L.temp_bytes = a;
  L.temp = ws.take(a > 0 ? a : 1);
  L.total = ws.total();
  return L;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_thresholds_workspace_bytes(int64_t n_rows, int64_t n_genes) {
  const int rc = thr_check_sizes("segger_thresholds_workspace_bytes", n_rows, n_genes);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)thr_layout(n_rows, n_genes).total;
}

extern "C" int segger_thresholds_build(const float* similarity, const int32_t* gene, const int32_t* cell, int64_t n_rows,
                                       int64_t n_genes, int32_t max_iter, double* threshold, double* yen, double* li,
                                       int64_t* count, uint8_t* converged, int64_t* counters, void* workspace,
                                       int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_thresholds_build";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = thr_check_sizes(who, n_rows, n_genes);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(max_iter >= 1, "%s: max_iter must be at least 1", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace size", who);
  SEGGER_REQUIRE(threshold && yen && li && count && converged && counters, "%s: NULL pointer", who);
  SEGGER_REQUIRE(n_rows == 0 || (similarity && gene && cell && workspace), "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(threshold, 8) && is_aligned(yen, 8) && is_aligned(li, 8) && is_aligned(count, 8) &&
                     is_aligned(counters, 8),
                 "%s: threshold, yen, li, count and counters must be 8-byte aligned", who);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (n_rows == 0) {                               // no row pointer and no workspace is looked at
    SEGGER_HIP(hipMemsetAsync(cnt, 0, kThrCounters * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(thresholds_absent_kernel, dim3(thr_grid(n_genes)), dim3(kThrThreads), 0, stream, n_genes, threshold,
                       yen, li, count, converged);
    SEGGER_LAUNCH_CHECK("thresholds_absent_kernel");
    return SEGGER_OK;
  }
  SEGGER_REQUIRE(is_aligned(similarity, 4) && is_aligned(gene, 4) && is_aligned(cell, 4),
                 "%s: similarity, gene and cell must be 4-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  const ThrLayout L = thr_layout(n_rows, n_genes);
  if ((size_t)workspace_bytes < L.total) return workspace_too_small(who, (size_t)workspace_bytes, L.total);

  unsigned long long* keys_a = at<unsigned long long>(workspace, L.keys_a);
  unsigned long long* keys_b = at<unsigned long long>(workspace, L.keys_b);
  int32_t* beg = at<int32_t>(workspace, L.beg);
  int32_t* end = at<int32_t>(workspace, L.end);
  unsigned long long* gap = at<unsigned long long>(workspace, L.gap);
  double* chunk_sum = at<double>(workspace, L.chunk_sum);
  size_t temp_bytes = L.temp_bytes;

  SEGGER_HIP(hipMemsetAsync(cnt, 0, kThrCounters * sizeof(unsigned long long), stream));
  const int64_t n_items = n_rows > n_genes ? n_rows : n_genes;
  hipLaunchKernelGGL(thresholds_keys_kernel, dim3(thr_grid(n_items)), dim3(kThrThreads), 0, stream, similarity, gene, cell,
                     n_rows, n_genes, keys_a, beg, end, gap, cnt);
  SEGGER_LAUNCH_CHECK("thresholds_keys_kernel");
  SEGGER_HIP(rocprim::radix_sort_keys<NoScratchSortConfig>(at<char>(workspace, L.temp), temp_bytes, keys_a, keys_b, (size_t)n_rows, 0,
                                                     (unsigned)L.key_bits, stream));
  hipLaunchKernelGGL(thresholds_segments_kernel, dim3(thr_grid(n_rows)), dim3(kThrThreads), 0, stream,
                     (const unsigned long long*)keys_b, n_rows, beg, end, cnt);
  SEGGER_LAUNCH_CHECK("thresholds_segments_kernel");
  const int64_t n_chunks = (n_rows + kThrChunk - 1) / kThrChunk;
  hipLaunchKernelGGL(thresholds_chunks_kernel, dim3((unsigned)(n_chunks < 65536 ? n_chunks : 65536)), dim3(kThrThreads), 0,
                     stream, (const unsigned long long*)keys_b, n_rows, (const int32_t*)beg, gap, chunk_sum);
  SEGGER_LAUNCH_CHECK("thresholds_chunks_kernel");
  hipLaunchKernelGGL(thresholds_genes_kernel, dim3((unsigned)(n_genes < 65536 ? n_genes : 65536)), dim3(kThrThreads), 0,
                     stream, (const unsigned long long*)keys_b, (const int32_t*)beg, (const int32_t*)end,
                     (const unsigned long long*)gap, chunk_sum, n_genes, max_iter, threshold, yen, li, count, converged);
  SEGGER_LAUNCH_CHECK("thresholds_genes_kernel");
  return SEGGER_OK;
}
