// segger_assign_update / segger_assign_finalize: the best row per transcript over a stream of prediction batches
// (include/segger_amd.h has the contract).  The dedup of postprocess.best_assignment is a per-transcript arg-max; a
// 64-bit atomic max over a packed (similarity, arrival order) key computes it without a sort, and -- max being
// order-independent and the keys unique -- with the same bits whatever order the rows arrive in.
// Per row: 25 bytes streamed in, one 8-byte atomic, one 8-byte read back; per winner two 4-byte stores.
#include "common.h"
#include "post_common.h"

namespace segger {
namespace {

constexpr int kAssignThreads = 256;
constexpr int64_t kAssignMaxBlocks = 1024;      // grid-stride above 262 144 rows: four blocks per CU of the MI355X
constexpr uint32_t kCanonicalNan = 0x7fc00000u;
constexpr unsigned long long kSeqLimit = 0x100000000ull;

// similarity bits -> unsigned order: larger = higher similarity, NaN above +inf (torch.sort's order), -0.0 == +0.0
__device__ __forceinline__ uint32_t assign_ord(float s) {
  uint32_t b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;                                  // bits(s + 0.0f) without touching denormals
  if ((b & 0x7fffffffu) > 0x7f800000u) b = kCanonicalNan;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float assign_similarity(uint32_t ord) {
  return __uint_as_float((ord >> 31) ? (ord ^ 0x80000000u) : ~ord);
}

// key of row i, or 0 (no real key) for a row that takes no part: masked out, or dropped (dropped = true)
__device__ __forceinline__ unsigned long long assign_key(const int64_t* __restrict__ tx_index, const float* __restrict__ sim,
                                                         const uint8_t* __restrict__ mask, int64_t i, unsigned long long base,
                                                         int64_t n_tx, int64_t& tx, bool& dropped) {
  dropped = false;
  if (mask && !mask[i]) return 0ull;
  tx = tx_index[i];
  const unsigned long long q = base + (unsigned long long)i;
  if (tx < 0 || tx >= n_tx || q >= kSeqLimit) {                  // never written; the caller reads the count
    dropped = true;
    return 0ull;
  }
  return ((unsigned long long)assign_ord(sim[i]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)q);
}

__global__ __launch_bounds__(kAssignThreads) void assign_max_kernel(const int64_t* __restrict__ tx_index,
                                                                    const float* __restrict__ sim,
                                                                    const uint8_t* __restrict__ mask, int64_t n,
                                                                    unsigned long long* __restrict__ best_key,
                                                                    unsigned long long* __restrict__ counters, int64_t n_tx) {
  const unsigned long long base = counters[0];                   // advanced by assign_advance_kernel, behind both passes
  const int64_t stride = (int64_t)gridDim.x * kAssignThreads;
  unsigned long long n_dropped = 0;
  for (int64_t i = (int64_t)blockIdx.x * kAssignThreads + threadIdx.x; i < n; i += stride) {
    int64_t tx;
    bool dropped;
    const unsigned long long key = assign_key(tx_index, sim, mask, i, base, n_tx, tx, dropped);
    n_dropped += dropped ? 1ull : 0ull;
    if (key) atomicMax(best_key + tx, key);
  }
  if (n_dropped) atomicAdd(counters + 1, n_dropped);
}

// sequence numbers are unique, so exactly one row of a transcript carries its best key: no two threads write one slot
__global__ __launch_bounds__(kAssignThreads) void assign_write_kernel(const int64_t* __restrict__ tx_index,
                                                                      const int64_t* __restrict__ seg,
                                                                      const float* __restrict__ sim,
                                                                      const int32_t* __restrict__ gene,
                                                                      const uint8_t* __restrict__ mask, int64_t n,
                                                                      const unsigned long long* __restrict__ best_key,
                                                                      int32_t* __restrict__ cell, int32_t* __restrict__ gene_out,
                                                                      const unsigned long long* __restrict__ counters,
                                                                      int64_t n_tx) {
  const unsigned long long base = counters[0];
  const int64_t stride = (int64_t)gridDim.x * kAssignThreads;
  for (int64_t i = (int64_t)blockIdx.x * kAssignThreads + threadIdx.x; i < n; i += stride) {
    int64_t tx;
    bool dropped;
    const unsigned long long key = assign_key(tx_index, sim, mask, i, base, n_tx, tx, dropped);
    if (key && best_key[tx] == key) {
      cell[tx] = (int32_t)seg[i];
      gene_out[tx] = gene[i];
    }
  }
}

// a launch of its own: in stream order behind every block of the two passes above, so none of them sees the new base
__global__ void assign_advance_kernel(unsigned long long* __restrict__ counters, unsigned long long n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) counters[0] += n;
}

__global__ __launch_bounds__(kAssignThreads) void assign_finalize_kernel(const unsigned long long* __restrict__ best_key,
                                                                         int64_t n_tx, float* __restrict__ similarity,
                                                                         uint8_t* __restrict__ seen) {
  const int64_t stride = (int64_t)gridDim.x * kAssignThreads;
  for (int64_t t = (int64_t)blockIdx.x * kAssignThreads + threadIdx.x; t < n_tx; t += stride) {
    const unsigned long long k = best_key[t];
    similarity[t] = k ? assign_similarity((uint32_t)(k >> 32)) : 0.0f;
    seen[t] = k ? 1 : 0;
  }
}

unsigned assign_grid(int64_t n) {
  const int64_t blocks = (n + kAssignThreads - 1) / kAssignThreads;
  return (unsigned)(blocks < kAssignMaxBlocks ? blocks : kAssignMaxBlocks);
}

int assign_check_n_tx(const char* who, int64_t n_tx) {
  SEGGER_REQUIRE(n_tx >= 1, "%s: n_tx must be at least 1", who);
  SEGGER_REQUIRE(n_tx <= 0x7fffffffLL, "%s: 2^31 transcripts or more", who);
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int segger_assign_update(const int64_t* tx_index, const int64_t* seg, const float* sim, const int32_t* gene,
                                    const uint8_t* mask, int64_t n, uint64_t* best_key, int32_t* cell, int32_t* gene_out,
                                    uint64_t* counters, int64_t n_tx, segger_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n >= 0, "segger_assign_update: negative size");
  SEGGER_REQUIRE(n <= 0xffffffffLL, "segger_assign_update: 2^32 rows or more in one call");
  const int rc = assign_check_n_tx("segger_assign_update", n_tx);
  if (rc != SEGGER_OK) return rc;
  if (n == 0) return SEGGER_OK;
  SEGGER_REQUIRE(tx_index && seg && sim && gene && best_key && cell && gene_out && counters,
                 "segger_assign_update: NULL pointer");
  SEGGER_REQUIRE(is_aligned(tx_index, 8) && is_aligned(seg, 8) && is_aligned(best_key, 8) &&
                     is_aligned(counters, 8),
                 "segger_assign_update: tx_index, seg, best_key and counters must be 8-byte aligned");
  SEGGER_REQUIRE(is_aligned(sim, 4) && is_aligned(gene, 4) && is_aligned(cell, 4) && is_aligned(gene_out, 4),
                 "segger_assign_update: sim, gene, cell and gene_out must be 4-byte aligned");
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(best_key);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  const unsigned grid = assign_grid(n);
  hipLaunchKernelGGL(assign_max_kernel, dim3(grid), dim3(kAssignThreads), 0, stream, tx_index, sim, mask, n, keys, cnt, n_tx);
  SEGGER_LAUNCH_CHECK("assign_max_kernel");
  hipLaunchKernelGGL(assign_write_kernel, dim3(grid), dim3(kAssignThreads), 0, stream, tx_index, seg, sim, gene, mask, n,
                     (const unsigned long long*)keys, cell, gene_out, (const unsigned long long*)cnt, n_tx);
  SEGGER_LAUNCH_CHECK("assign_write_kernel");
  hipLaunchKernelGGL(assign_advance_kernel, dim3(1), dim3(1), 0, stream, cnt, (unsigned long long)n);
  SEGGER_LAUNCH_CHECK("assign_advance_kernel");
  return SEGGER_OK;
}

extern "C" int segger_assign_finalize(const uint64_t* best_key, int64_t n_tx, float* similarity_out, uint8_t* seen_out,
                                      segger_stream_t stream) {
  const int rc = assign_check_n_tx("segger_assign_finalize", n_tx);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(best_key && similarity_out && seen_out, "segger_assign_finalize: NULL pointer");
  SEGGER_REQUIRE(is_aligned(best_key, 8), "segger_assign_finalize: best_key must be 8-byte aligned");
  SEGGER_REQUIRE(is_aligned(similarity_out, 4), "segger_assign_finalize: similarity_out must be 4-byte aligned");
  hipLaunchKernelGGL(assign_finalize_kernel, dim3(assign_grid(n_tx)), dim3(kAssignThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(best_key), n_tx, similarity_out, seen_out);
  SEGGER_LAUNCH_CHECK("assign_finalize_kernel");
  return SEGGER_OK;
}
