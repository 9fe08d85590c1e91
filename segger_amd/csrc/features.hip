// segger_sparse_gram / segger_sparse_project: the two kernels behind the boundary and gene features of a count matrix
// (include/segger_amd.h has the contract; segger_amd/features.py is the caller).
//
// Gram: S = sum_r w_r^2 x_r x_r^T and s = sum_r w_r x_r over the rows of a CSR matrix, float64, nothing dense in HBM.
// One workgroup per pair of 64-gene tiles (ti <= tj) and per slab of rows.  A block of 32 rows is densified into two
// zero-filled LDS tiles (its entries inside the two gene ranges, times w_r; the range start by binary search in the
// sorted row) and multiplied with v_mfma_f64_16x16x4_f64: wave v owns genes 16 v .. 16 v + 15 of tile ti against the four
// 16-gene blocks of tile tj.  The accumulators of a workgroup leave as one 64 x 64 partial per (slab, pair); a second
// kernel adds the partials in slab order, writes the upper triangle and mirrors it.  The slab count depends on the
// shapes alone and every sum has a fixed order: no floating-point atomics, the same bits from call to call.
//
// Project: out[r, :] = w_r * sum_j x_rj V[j, :] - offset, one wave per row, the entries in CSR order, lane l owning the
// columns l, l + 64, l + 128, l + 192 in float64.
#include "common.h"
#include "post_common.h"

namespace segger {
namespace {

constexpr int kFeatThreads = 256;
constexpr int kFeatWaves = kFeatThreads / kWave;
constexpr int kTile = SEGGER_FEATURES_TILE;             // genes per tile: four waves x 16 rows of the MFMA
constexpr int kRowBlock = 32;                           // CSR rows densified at a time: eight K = 4 steps
constexpr int kLd = kTile + 16;                         // LDS row stride in doubles: rows k and k + 1 of an operand read
                                                        // (lanes 0-15 / 16-31) fall into different halves of the banks
constexpr int kSubLanes = kFeatThreads / kRowBlock;     // threads that share one row of the block when it is scattered
constexpr int64_t kTileElems = (int64_t)kTile * kTile;
constexpr int64_t kProjMaxBlocks = 4096;

typedef double f64x4 __attribute__((ext_vector_type(4)));

static_assert(kTile == 64 && kFeatWaves * 16 == kTile, "one wave per 16 genes of the first tile");
static_assert(kRowBlock % 4 == 0 && kFeatThreads % kRowBlock == 0, "row block: whole MFMA steps, whole thread groups");
static_assert(SEGGER_FEATURES_SLAB_ROWS % kRowBlock == 0, "a slab is a whole number of row blocks");

struct GramPlan {
  int64_t n_tiles, n_pairs, n_slabs, slab_rows;
  size_t partial, colsum, total;                        // byte offsets into the workspace
};

// Slabs: as many as keep ~SEGGER_FEATURES_TARGET_GROUPS workgroups busy, never more than SEGGER_FEATURES_MAX_SLABS, never
// shorter than SEGGER_FEATURES_SLAB_ROWS rows -- a function of (n_rows, n_cols) only.
GramPlan gram_plan(int64_t n_rows, int64_t n_cols) {
  GramPlan p;
  p.n_tiles = ceil_div(n_cols, kTile);
  p.n_pairs = p.n_tiles * (p.n_tiles + 1) / 2;
  int64_t slabs = ceil_div(n_rows, SEGGER_FEATURES_SLAB_ROWS);
  const int64_t by_groups = ceil_div(SEGGER_FEATURES_TARGET_GROUPS, p.n_pairs);
  if (slabs > by_groups) slabs = by_groups;
  if (slabs > SEGGER_FEATURES_MAX_SLABS) slabs = SEGGER_FEATURES_MAX_SLABS;
  if (slabs < 1) slabs = 1;
  p.n_slabs = slabs;
  p.slab_rows = ceil_div(ceil_div(n_rows > 0 ? n_rows : 1, slabs), kRowBlock) * kRowBlock;
  Carver ws;                                            // both regions are whole multiples of 512 bytes: nothing is padded
  p.partial = ws.take((size_t)(p.n_slabs * p.n_pairs * kTileElems) * sizeof(double));
  p.colsum = ws.take((size_t)(p.n_slabs * p.n_tiles * kTile) * sizeof(double));
  p.total = ws.total();
  return p;
}

// first position in [lo, hi) whose column is >= col (the row is strictly ascending)
__device__ __forceinline__ int64_t feat_lower_bound(const int32_t* __restrict__ indices, int64_t lo, int64_t hi, int32_t col) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (indices[mid] < col) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the entries of row [beg, end) inside columns [c0, c0 + kTile), times w, into one zero-filled LDS row; `sub` of
// kSubLanes threads take every kSubLanes-th entry.  Ascending columns: no two entries share a slot.
__device__ __forceinline__ void feat_scatter_row(const int32_t* __restrict__ indices, const int32_t* __restrict__ values,
                                                 int64_t beg, int64_t end, int32_t c0, double w, int sub, double* row) {
  const int32_t c1 = c0 + kTile;
  for (int64_t e = feat_lower_bound(indices, beg, end, c0) + sub; e < end; e += kSubLanes) {
    const int32_t c = indices[e];
    if (c >= c1) break;
    if (c >= c0) row[c - c0] = w * (double)values[e];
  }
}

__global__ __launch_bounds__(kFeatThreads) void features_gram_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const int32_t* __restrict__ values,
    const double* __restrict__ row_weight, int64_t n_rows, int64_t nnz, int64_t n_tiles, int64_t n_pairs, int64_t slab_rows,
    double* __restrict__ partial, double* __restrict__ colsum) {
  __shared__ double tiles[2 * kRowBlock * kLd];
  double* tile_a = tiles;
  double* tile_b = tiles + kRowBlock * kLd;
  // pair index -> (ti, tj), ti <= tj, row-major over the upper triangle
  int64_t p = blockIdx.x, ti = 0;
  while (p >= n_tiles - ti) { p -= n_tiles - ti; ++ti; }
  const int64_t tj = ti + p;
  const bool diag = ti == tj;
  const double* tb = tiles + (diag ? 0 : kRowBlock * kLd);      // a diagonal pair multiplies its one tile with itself
  const int64_t slab = blockIdx.y;
  const int64_t row_beg = slab * slab_rows;
  const int64_t row_end = row_beg + slab_rows < n_rows ? row_beg + slab_rows : n_rows;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const int lk = lane >> 4, lc = lane & 15;
  const int srow = tid / kSubLanes, sub = tid % kSubLanes;

  f64x4 acc[4];
#pragma unroll
  for (int nj = 0; nj < 4; ++nj) acc[nj] = f64x4{0.0, 0.0, 0.0, 0.0};
  double col_acc = 0.0;                                  // threads 0..63 of a diagonal pair: s of column ti * 64 + tid

  for (int64_t r0 = row_beg; r0 < row_end; r0 += kRowBlock) {
    for (int i = tid; i < kRowBlock * kLd; i += kFeatThreads) {
      tile_a[i] = 0.0;
      if (!diag) tile_b[i] = 0.0;
    }
    __syncthreads();
    const int64_t r = r0 + srow;
    if (r < row_end) {
      const double w = row_weight[r];
      if (w != 0.0) {                                    // weight 0: the row takes no part
        int64_t beg = indptr[r], end = indptr[r + 1];
        beg = beg < 0 ? 0 : beg;
        end = end > nnz ? nnz : end;                     // never past the arrays, whatever indptr holds
        feat_scatter_row(indices, values, beg, end, (int32_t)(ti * kTile), w, sub, tile_a + srow * kLd);
        if (!diag) feat_scatter_row(indices, values, beg, end, (int32_t)(tj * kTile), w, sub, tile_b + srow * kLd);
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kRowBlock / 4; ++ks) {
      // A[i][k] = tile_a[row k][gene i], B[k][j] = tile_b[row k][gene j]: D[i][j] += sum_k A[i][k] B[k][j]
      const double a = tile_a[(ks * 4 + lk) * kLd + wave * 16 + lc];
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) {
        if (diag && nj < wave) continue;                 // below the diagonal of a diagonal pair: never read back
        const double b = tb[(ks * 4 + lk) * kLd + nj * 16 + lc];
        acc[nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nj], 0, 0, 0);
      }
    }
    if (diag && tid < kTile) {
#pragma unroll 8
      for (int k = 0; k < kRowBlock; ++k) col_acc += tile_a[k * kLd + tid];
    }
    __syncthreads();
  }

  // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = partial + (slab * n_pairs + (int64_t)blockIdx.x) * kTileElems;
#pragma unroll
  for (int nj = 0; nj < 4; ++nj) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(wave * 16 + lk + 4 * reg) * kTile + nj * 16 + lc] = acc[nj][reg];
  }
  if (diag && tid < kTile) colsum[(slab * n_tiles + ti) * kTile + tid] = col_acc;
}

// S and s from the partials, slabs first to last.  One thread per element of a pair's tile; the lower triangle of a
// diagonal pair is skipped, every other element is written to S[i, j] and S[j, i].
__global__ __launch_bounds__(kFeatThreads) void features_gram_reduce_kernel(
    const double* __restrict__ partial, const double* __restrict__ colsum, int64_t n_cols, int64_t n_tiles, int64_t n_pairs,
    int64_t n_slabs, double* __restrict__ S, double* __restrict__ s) {
  constexpr int kBlocksPerPair = (int)(kTileElems / kFeatThreads);
  const int64_t pair = blockIdx.x / kBlocksPerPair;
  int64_t p = pair, ti = 0;
  while (p >= n_tiles - ti) { p -= n_tiles - ti; ++ti; }
  const int64_t tj = ti + p;
  const int elem = (int)(blockIdx.x % kBlocksPerPair) * kFeatThreads + threadIdx.x;
  const int a = elem / kTile, b = elem % kTile;
  const int64_t gi = ti * kTile + a, gj = tj * kTile + b;
  if (gi < n_cols && gj < n_cols && gi <= gj) {
    double v = 0.0;
    for (int64_t sl = 0; sl < n_slabs; ++sl) v += partial[(sl * n_pairs + pair) * kTileElems + elem];
    S[gi * n_cols + gj] = v;
    S[gj * n_cols + gi] = v;
  }
  if (ti == tj && elem < kTile && ti * kTile + elem < n_cols) {
    double v = 0.0;
    for (int64_t sl = 0; sl < n_slabs; ++sl) v += colsum[(sl * n_tiles + ti) * kTile + elem];
    s[ti * kTile + elem] = v;
  }
}

// KC = ceil(k / 64) column chunks per lane
template <int KC, typename Out>
__global__ __launch_bounds__(kFeatThreads) void features_project_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const int32_t* __restrict__ values,
    const double* __restrict__ row_weight, int64_t n_rows, int64_t n_cols, int64_t nnz, const double* __restrict__ V,
    const double* __restrict__ offset, int k, Out* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n_waves = (int64_t)gridDim.x * kFeatWaves;
  double off[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) off[c] = lane + c * kWave < k ? offset[lane + c * kWave] : 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kFeatWaves + (threadIdx.x >> 6); r < n_rows; r += n_waves) {   // wave-uniform
    double acc[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[c] = 0.0;
    const double w = row_weight[r];
    if (w != 0.0) {
      int64_t beg = indptr[r], end = indptr[r + 1];
      beg = beg < 0 ? 0 : beg;
      end = end > nnz ? nnz : end;
#pragma unroll 4
      for (int64_t e = beg; e < end; ++e) {
        const int32_t j = indices[e];
        if ((uint32_t)j >= (uint32_t)n_cols) continue;   // a column outside V is never used as an index
        const double x = (double)values[e];
        const double* v = V + (int64_t)j * k + lane;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          if (lane + c * kWave < k) acc[c] = fma(x, v[c * kWave], acc[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      if (lane + c * kWave < k) out[r * k + lane + c * kWave] = (Out)(w != 0.0 ? fma(w, acc[c], -off[c]) : -off[c]);
    }
  }
}

template <typename Out>
int project_launch(const int64_t* indptr, const int32_t* indices, const int32_t* values, const double* row_weight,
                   int64_t n_rows, int64_t n_cols, int64_t nnz, const double* V, const double* offset, int k, Out* out,
                   hipStream_t stream) {
  int64_t blocks = ceil_div(n_rows, kFeatWaves);
  if (blocks > kProjMaxBlocks) blocks = kProjMaxBlocks;
  const dim3 grid((unsigned)blocks), block(kFeatThreads);
  switch ((k + kWave - 1) / kWave) {
    case 1: hipLaunchKernelGGL((features_project_kernel<1, Out>), grid, block, 0, stream, indptr, indices, values, row_weight,
                               n_rows, n_cols, nnz, V, offset, k, out); break;
    case 2: hipLaunchKernelGGL((features_project_kernel<2, Out>), grid, block, 0, stream, indptr, indices, values, row_weight,
                               n_rows, n_cols, nnz, V, offset, k, out); break;
    case 3: hipLaunchKernelGGL((features_project_kernel<3, Out>), grid, block, 0, stream, indptr, indices, values, row_weight,
                               n_rows, n_cols, nnz, V, offset, k, out); break;
    default: hipLaunchKernelGGL((features_project_kernel<4, Out>), grid, block, 0, stream, indptr, indices, values, row_weight,
                                n_rows, n_cols, nnz, V, offset, k, out); break;
  }
  SEGGER_LAUNCH_CHECK("features_project_kernel");
  return SEGGER_OK;
}

int feat_check_sizes(const char* who, int64_t n_rows, int64_t n_cols) {
  SEGGER_REQUIRE(n_rows >= 0, "%s: negative n_rows", who);
  SEGGER_REQUIRE(n_rows <= 0x7fffffffLL, "%s: 2^31 rows or more", who);
  SEGGER_REQUIRE(n_cols >= 1, "%s: n_cols must be at least 1", who);
  SEGGER_REQUIRE(n_cols <= SEGGER_FEATURES_MAX_COLS, "%s: n_cols above %d", who, SEGGER_FEATURES_MAX_COLS);
  return SEGGER_OK;
}

int feat_check_csr(const char* who, const int64_t* indptr, const int32_t* indices, const int32_t* values,
                   const double* row_weight, int64_t nnz) {
  SEGGER_REQUIRE(nnz >= 0, "%s: negative nnz", who);
  SEGGER_REQUIRE(indptr && row_weight && (nnz == 0 || (indices && values)), "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(indptr, 8) && is_aligned(row_weight, 8), "%s: indptr and row_weight must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(indices, 4) && is_aligned(values, 4), "%s: indices and values must be 4-byte aligned", who);
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_features_gram_slabs(int64_t n_rows, int64_t n_cols) {
  const int rc = feat_check_sizes("segger_features_gram_slabs", n_rows, n_cols);
  if (rc != SEGGER_OK) return rc;
  return gram_plan(n_rows, n_cols).n_slabs;
}

extern "C" int64_t segger_features_workspace_bytes(int64_t n_rows, int64_t n_cols) {
  const int rc = feat_check_sizes("segger_features_workspace_bytes", n_rows, n_cols);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)gram_plan(n_rows, n_cols).total;
}

extern "C" int segger_sparse_gram(const int64_t* indptr, const int32_t* indices, const int32_t* values,
                                  const double* row_weight, int64_t n_rows, int64_t n_cols, int64_t nnz, double* S, double* s,
                                  void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_sparse_gram";
  hipStream_t stream = (hipStream_t)stream_;
  int rc = feat_check_sizes(who, n_rows, n_cols);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(S && s, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(S, 8) && is_aligned(s, 8), "%s: S and s must be 8-byte aligned", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  if (n_rows == 0) {                                     // an empty matrix: zeros, no kernel
    SEGGER_HIP(hipMemsetAsync(S, 0, (size_t)(n_cols * n_cols) * sizeof(double), stream));
    SEGGER_HIP(hipMemsetAsync(s, 0, (size_t)n_cols * sizeof(double), stream));
    return SEGGER_OK;
  }
  rc = feat_check_csr(who, indptr, indices, values, row_weight, nnz);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(workspace, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  const GramPlan plan = gram_plan(n_rows, n_cols);
  if ((size_t)workspace_bytes < plan.total) return workspace_too_small(who, (size_t)workspace_bytes, plan.total);
  double* partial = at<double>(workspace, plan.partial);
  double* colsum = at<double>(workspace, plan.colsum);
  hipLaunchKernelGGL(features_gram_kernel, dim3((unsigned)plan.n_pairs, (unsigned)plan.n_slabs), dim3(kFeatThreads), 0, stream,
                     indptr, indices, values, row_weight, n_rows, nnz, plan.n_tiles, plan.n_pairs, plan.slab_rows, partial,
                     colsum);
  SEGGER_LAUNCH_CHECK("features_gram_kernel");
  hipLaunchKernelGGL(features_gram_reduce_kernel, dim3((unsigned)(plan.n_pairs * (kTileElems / kFeatThreads))),
                     dim3(kFeatThreads), 0, stream, (const double*)partial, (const double*)colsum, n_cols, plan.n_tiles,
                     plan.n_pairs, plan.n_slabs, S, s);
  SEGGER_LAUNCH_CHECK("features_gram_reduce_kernel");
  return SEGGER_OK;
}

extern "C" int segger_sparse_project(const int64_t* indptr, const int32_t* indices, const int32_t* values,
                                     const double* row_weight, int64_t n_rows, int64_t n_cols, int64_t nnz, const double* V,
                                     const double* offset, int32_t k, void* out, int32_t out_f64, segger_stream_t stream_) {
  const char* who = "segger_sparse_project";
  hipStream_t stream = (hipStream_t)stream_;
  int rc = feat_check_sizes(who, n_rows, n_cols);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(k >= 1 && k <= SEGGER_FEATURES_MAX_K, "%s: k = %d outside 1 .. %d", who, (int)k, SEGGER_FEATURES_MAX_K);
  SEGGER_REQUIRE(out_f64 == 0 || out_f64 == 1, "%s: out_f64 must be 0 (float32) or 1 (float64)", who);
  if (n_rows == 0) return SEGGER_OK;
  rc = feat_check_csr(who, indptr, indices, values, row_weight, nnz);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(V && offset && out, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(V, 8) && is_aligned(offset, 8) && is_aligned(out, out_f64 ? 8 : 4),
                 "%s: V, offset and out must be aligned to their element size", who);
  if (out_f64)
    return project_launch<double>(indptr, indices, values, row_weight, n_rows, n_cols, nnz, V, offset, (int)k,
                                  static_cast<double*>(out), stream);
  return project_launch<float>(indptr, indices, values, row_weight, n_rows, n_cols, nnz, V, offset, (int)k,
                               static_cast<float*>(out), stream);
}
