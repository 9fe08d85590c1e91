// Phenograph clustering on the device (include/segger_amd.h has the contract; segger_amd/phenograph.py is the caller):
// the exact k nearest rows of a [N, d] matrix, the Jaccard weights of the neighbour graph, and the kernels of a
// deterministic synchronous Louvain.
//
// kNN.  Scores are the expanded form (|a|^2 + |b|^2) - 2 a.b; the inner products run on v_mfma_f32_16x16x4_f32.  A
// workgroup of eight waves owns 128 query rows (wave w the rows 16 w .. 16 w + 15, their fragments of A resident in
// registers for the whole kernel) and walks its slab of candidate rows 64 at a time through one LDS tile.  The 128 x 64
// scores of a tile go through LDS to the wave that owns the row: lane l takes candidate l, and a row whose running k-th
// best is beaten by any of them sorts the 64 candidates (bitonic, in the wave) and merges them with its list.  Lists are
// ordered by the 64-bit key (score bits in float order, candidate index), so the selected set is independent of the tile
// and slab order; the merge is skipped -- a wave-uniform branch, not a loop -- when no candidate passes.  Every slab
// leaves its k keys per row; the finish kernel merges the slabs, recomputes the k distances as sum (a - b)^2 in
// ascending dimension order and sorts by (distance, index).  No score matrix is written to memory.
//
// Nothing here is contracted by the compiler: every fused multiply-add is an explicit fma()/fmaf().
#include "common.h"
#include "post_common.h"
#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kKnnWaves = 8;
constexpr int kKnnThreads = kKnnWaves * kWave;
constexpr int kQTile = kKnnWaves * 16;                  // query rows per workgroup: one 16-row MFMA block per wave
constexpr int kCTile = 64;                              // candidate rows per LDS tile: one per lane at selection
constexpr int kScoreLd = kCTile + 1;
constexpr uint64_t kKeyNone = ~0ull;                    // sorts after every real (score, index)
constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / kWave;
constexpr int kQThreads = 256;                          // the single workgroup of the modularity sum

static_assert(kCTile == kWave, "selection: one candidate of the tile per lane");
static_assert(SEGGER_KNN_BF_MAX_K <= kWave, "a row's list is one key per lane");

struct KnnPlan {
  int64_t q_tiles, n_slabs, slab_len;
  size_t norm, partial, total;                          // byte offsets into the workspace
};

// Slabs of candidate rows: enough that ~SEGGER_KNN_BF_TARGET_GROUPS workgroups exist, never shorter than two tiles,
// never more than SEGGER_KNN_BF_MAX_SLABS -- a function of n alone (d and k only size the workspace).
KnnPlan knn_plan(int64_t n, int64_t d, int64_t k) {
  KnnPlan p;
  p.q_tiles = ceil_div(n > 0 ? n : 1, kQTile);
  int64_t slabs = ceil_div(SEGGER_KNN_BF_TARGET_GROUPS, p.q_tiles);
  const int64_t by_len = n / (2 * kCTile);
  if (slabs > by_len) slabs = by_len;
  if (slabs > SEGGER_KNN_BF_MAX_SLABS) slabs = SEGGER_KNN_BF_MAX_SLABS;
  if (slabs < 1) slabs = 1;
  p.n_slabs = slabs;
  p.slab_len = ceil_div(ceil_div(n > 0 ? n : 1, slabs), kCTile) * kCTile;
  p.n_slabs = ceil_div(n > 0 ? n : 1, p.slab_len);       // no empty slab at the end
  const size_t partial_bytes = (size_t)p.n_slabs * (size_t)n * (size_t)k * sizeof(uint64_t);
  Carver ws;
  p.norm = ws.take((size_t)n * sizeof(float));
  p.partial = ws.take(partial_bytes);
  p.total = p.partial + partial_bytes;                  // the last region is not rounded up
  return p;
}

// ---------------------------------------------------------------- wave-wide 64-bit helpers ---
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a < b ? b : a; }

// the 64 keys of a wave in ascending lane order (bitonic network, 21 exchanges)
__device__ __forceinline__ uint64_t wave_sort(uint64_t key, int lane) {
#pragma unroll
  for (int size = 2; size <= kWave; size <<= 1) {
#pragma unroll
    for (int j = size >> 1; j > 0; j >>= 1) {
      const uint64_t other = shfl_xor64(key, j);
      const bool up = (lane & size) == 0, low = (lane & j) == 0;
      key = (up == low) ? umin64(key, other) : umax64(key, other);
    }
  }
  return key;
}
// two ascending lists -> the 64 smallest of their 128 keys, ascending
__device__ __forceinline__ uint64_t wave_merge(uint64_t a, uint64_t b, int lane) {
  uint64_t key = umin64(a, shfl64(b, kWave - 1 - lane));  // bitonic, and it holds the 64 smallest
#pragma unroll
  for (int j = kWave >> 1; j > 0; j >>= 1) {
    const uint64_t other = shfl_xor64(key, j);
    key = (lane & j) == 0 ? umin64(key, other) : umax64(key, other);
  }
  return key;
}

// scores in float order (a cancelled score may be slightly negative)
__device__ __forceinline__ uint64_t score_key(float s, uint32_t index) { return ((uint64_t)ordered_bits(s) << 32) | index; }

// ---------------------------------------------------------------- kNN ---
__global__ __launch_bounds__(kRowThreads) void knn_norm_kernel(const float* __restrict__ X, int64_t n, int d,
                                                               float* __restrict__ norm) {
  const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (r >= n) return;
  const float* x = X + r * d;
  float acc = 0.0f;
  for (int j = 0; j < d; ++j) acc = fmaf(x[j], x[j], acc);
  norm[r] = acc;
}

// DP = d rounded up to 32, 64, 128 or 256: the padding dimensions are zeros on both sides
template <int DP>
__global__ __launch_bounds__(kKnnThreads) void knn_select_kernel(const float* __restrict__ X, const float* __restrict__ norm,
                                                                 int64_t n, int d, int k, int64_t slab_len,
                                                                 uint64_t* __restrict__ partial) {
  constexpr int kLd = DP + 4;                           // floats per LDS row: 16-byte rows, 16 lanes on 16 distinct bank groups
  __shared__ __attribute__((aligned(16))) float tile_b[kCTile * kLd];
  __shared__ float score[kQTile * kScoreLd];
  __shared__ float norm_b[kCTile];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int h = lane >> 4, lc = lane & 15;
  const int64_t q0 = (int64_t)blockIdx.x * kQTile + wave * 16;
  const int64_t c_beg = (int64_t)blockIdx.y * slab_len;
  const int64_t c_end = c_beg + slab_len < n ? c_beg + slab_len : n;

  // A[row lc][k = h] of step 4 s + j is dimension 16 s + 4 h + j: the same permutation of the dimensions as B below
  float a[DP / 4];
  {
    const int64_t row = q0 + lc;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int dim = 16 * s + 4 * h + j;
        a[4 * s + j] = (row < n && dim < d) ? X[row * d + dim] : 0.0f;
      }
    }
  }
  float norm_a[4];                                      // C/D rows of this lane: 4 h + reg
#pragma unroll
  for (int r = 0; r < 4; ++r) norm_a[r] = q0 + 4 * h + r < n ? norm[q0 + 4 * h + r] : 0.0f;
  uint64_t top[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) top[r] = kKeyNone;

  for (int64_t c0 = c_beg; c0 < c_end; c0 += kCTile) {
    __syncthreads();                                    // the previous tile has been read
    for (int e = tid; e < kCTile * DP; e += kKnnThreads) {
      const int cand = e / DP, dim = e % DP;
      const int64_t c = c0 + cand;
      tile_b[cand * kLd + dim] = (c < c_end && dim < d) ? X[c * d + dim] : 0.0f;
    }
    if (tid < kCTile) norm_b[tid] = c0 + tid < c_end ? norm[c0 + tid] : 0.0f;
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) acc[nj] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(&tile_b[(nj * 16 + lc) * kLd + 16 * s + 4 * h]);
        acc[nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 0], b.x, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 1], b.y, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 2], b.z, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s + 3], b.w, acc[nj], 0, 0, 0);
      }
    }
    // C/D: column (candidate) = lane & 15, row (query) = 4 (lane >> 4) + reg
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const float nb = norm_b[nj * 16 + lc];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        score[(wave * 16 + 4 * h + r) * kScoreLd + nj * 16 + lc] = fmaf(-2.0f, acc[nj][r], norm_a[r] + nb);
    }
    __syncthreads();
    const int64_t c = c0 + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint64_t key = c < c_end ? score_key(score[(wave * 16 + r) * kScoreLd + lane], (uint32_t)c) : kKeyNone;
      const uint64_t kth = shfl64(top[r], k - 1);
      if (__any(key < kth)) {                            // wave-uniform
        const uint64_t merged = wave_merge(top[r], wave_sort(key, lane), lane);
        top[r] = lane < k ? merged : kKeyNone;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = q0 + r;
    if (row < n && lane < k) partial[((int64_t)blockIdx.y * n + row) * k + lane] = top[r];
  }
}

// one wave per row: the slabs' lists merged, the k distances recomputed directly, the row sorted by (distance, index)
__global__ __launch_bounds__(kRowThreads) void knn_finish_kernel(const float* __restrict__ X, int64_t n, int d, int k,
                                                                 int64_t n_slabs, const uint64_t* __restrict__ partial,
                                                                 int32_t* __restrict__ idx, float* __restrict__ dist2) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (row >= n) return;                                 // the whole wave
  uint64_t top = lane < k ? partial[row * k + lane] : kKeyNone;
  for (int64_t sl = 1; sl < n_slabs; ++sl) {
    const uint64_t other = lane < k ? partial[(sl * n + row) * k + lane] : kKeyNone;
    top = wave_merge(top, other, lane);
  }
  const uint32_t j = (uint32_t)top;
  const bool valid = lane < k && (int64_t)j < n;        // k <= n: every one of the first k keys is a real row
  uint64_t key = kKeyNone;
  if (valid) {
    const float* xa = X + row * d;
    const float* xb = X + (int64_t)j * d;
    float acc = 0.0f;
    for (int t = 0; t < d; ++t) {
      const float diff = xa[t] - xb[t];
      acc = fmaf(diff, diff, acc);
    }
    key = ((uint64_t)__float_as_uint(acc) << 32) | j;   // acc >= 0: its bits are ordered as they are
  }
  key = wave_sort(key, lane);
  if (lane < k) {
    idx[row * k + lane] = (int32_t)(uint32_t)key;
    dist2[row * k + lane] = __uint_as_float((uint32_t)(key >> 32));
  }
}

template <int DP>
int knn_select_launch(const float* X, const float* norm, int64_t n, int d, int k, const KnnPlan& plan, uint64_t* partial,
                      hipStream_t stream) {
  hipLaunchKernelGGL((knn_select_kernel<DP>), dim3((unsigned)plan.q_tiles, (unsigned)plan.n_slabs), dim3(kKnnThreads), 0,
                     stream, X, norm, n, d, k, plan.slab_len, partial);
  SEGGER_LAUNCH_CHECK("knn_select_kernel");
  return SEGGER_OK;
}

// ---------------------------------------------------------------- Jaccard ---
// One thread per stored edge (u, v): the two ascending adjacency lists are merged; with the closed neighbourhoods
// N[x] = adj[x] + {x} an edge has |N[u] & N[v]| = common + 2 and |N[u] | N[v]| = deg u + deg v + 2 - that.
__global__ __launch_bounds__(kRowThreads) void jaccard_kernel(const int64_t* __restrict__ indptr,
                                                              const int32_t* __restrict__ indices, int64_t n, int64_t nnz,
                                                              double* __restrict__ weight) {
  const int64_t e = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (e >= nnz) return;
  int64_t lo = 0, hi = n;                                // the last row whose start is <= e
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (indptr[mid] <= e) lo = mid; else hi = mid;
  }
  const int64_t v = indices[e];
  if (v < 0 || v >= n) { weight[e] = 0.0; return; }
  int64_t i = indptr[lo], ie = indptr[lo + 1], j = indptr[v], je = indptr[v + 1];
  i = i < 0 ? 0 : i; j = j < 0 ? 0 : j;
  ie = ie > nnz ? nnz : ie; je = je > nnz ? nnz : je;   // never past the arrays, whatever indptr holds
  const int64_t deg_u = ie > i ? ie - i : 0, deg_v = je > j ? je - j : 0;
  int64_t common = 0;
  while (i < ie && j < je) {
    const int32_t a = indices[i], b = indices[j];
    common += a == b;
    i += a <= b;
    j += b <= a;
  }
  const int64_t inter = common + 2;
  weight[e] = (double)inter / (double)(deg_u + deg_v + 2 - inter);
}

// ---------------------------------------------------------------- Louvain ---
// One wave per vertex of the sub-round.  For the community of every neighbour the wave's lane sums the vertex's edge
// weight into it by a pass over the row (quadratic in the degree, exact in 64-bit fixed point, correct for any degree,
// no list of a fixed size) and evaluates g(c) = k_vc - (gamma k_v) tot_c / 2m in float64; the best gain wins, the lowest
// community id on a tie, and the move is proposed only if it beats staying.  Everything is read from the state at the
// start of the sub-round: the proposals go to their own array.
__global__ __launch_bounds__(kRowThreads) void louvain_move_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const int64_t* __restrict__ w,
    const int64_t* __restrict__ kdeg, const int32_t* __restrict__ comm, const int64_t* __restrict__ tot,
    const int32_t* __restrict__ size, int64_t n, int64_t nnz, int sub, int n_sub, double gamma, double two_m,
    int32_t* __restrict__ proposal) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t v = sub + (int64_t)n_sub * ((int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6));
  if (v >= n) return;                                   // the whole wave
  int64_t beg = indptr[v], end = indptr[v + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > nnz ? nnz : end;
  const int32_t a = comm[v];
  if ((uint32_t)a >= (uint32_t)n) {                      // never an index: the vertex stays where it is
    if (lane == 0) proposal[v] = a;
    return;
  }
  const int64_t kv = kdeg[v];
  const double gk = gamma * (double)kv;
  const bool alone = size[a] == 1;
  int64_t kva = 0;
  for (int64_t e = beg + lane; e < end; e += kWave) {
    const int32_t u = indices[e];
    if ((uint32_t)u < (uint32_t)n && comm[u] == a) kva += w[e];
  }
  kva = wave_sum_i64(kva);
  const double g_stay = (double)kva - (gk * (double)(tot[a] - kv)) / two_m;
  double best_g = -__builtin_huge_val();
  int32_t best_c = 0x7fffffff;
  for (int64_t e = beg + lane; e < end; e += kWave) {
    const int32_t u = indices[e];
    if ((uint32_t)u >= (uint32_t)n) continue;
    const int32_t c = comm[u];
    if (c == a || (uint32_t)c >= (uint32_t)n) continue;
    if (alone && c > a && size[c] == 1) continue;       // two singletons never swap: only towards the lower id
    int64_t kvc = 0;
    for (int64_t f = beg; f < end; ++f) {
      const int32_t x = indices[f];
      if ((uint32_t)x < (uint32_t)n && comm[x] == c) kvc += w[f];
    }
    const double g = (double)kvc - (gk * (double)tot[c]) / two_m;
    if (g > best_g || (g == best_g && c < best_c)) { best_g = g; best_c = c; }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double og = __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(best_g), m));
    const int32_t oc = __shfl_xor(best_c, m, kWave);
    if (og > best_g || (og == best_g && oc < best_c)) { best_g = og; best_c = oc; }
  }
  if (lane == 0) proposal[v] = (best_c != 0x7fffffff && best_g > g_stay) ? best_c : a;
}

// the proposals of the sub-round applied: integer atomics only, exact in any order
__global__ __launch_bounds__(kRowThreads) void louvain_apply_kernel(const int32_t* __restrict__ proposal,
                                                                    const int64_t* __restrict__ kdeg, int64_t n, int sub,
                                                                    int n_sub, int32_t* __restrict__ comm,
                                                                    int64_t* __restrict__ tot, int32_t* __restrict__ size) {
  const int64_t v = sub + (int64_t)n_sub * ((int64_t)blockIdx.x * kRowThreads + threadIdx.x);
  if (v >= n) return;
  const int32_t a = comm[v], b = proposal[v];
  if (a == b || (uint32_t)b >= (uint32_t)n || (uint32_t)a >= (uint32_t)n) return;
  const unsigned long long kv = (unsigned long long)kdeg[v];
  comm[v] = b;
  atomicAdd(reinterpret_cast<unsigned long long*>(tot + b), kv);
  atomicAdd(reinterpret_cast<unsigned long long*>(tot + a), 0ull - kv);
  atomicAdd(size + b, 1);
  atomicAdd(size + a, -1);
}

// in_c: the self weight of every vertex plus its edges that stay inside its community (both directions are stored)
__global__ __launch_bounds__(kRowThreads) void louvain_internal_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const int64_t* __restrict__ w,
    const int64_t* __restrict__ self_w, const int32_t* __restrict__ comm, int64_t n, int64_t nnz, int64_t* __restrict__ in_c) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t v = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (v >= n) return;
  int64_t beg = indptr[v], end = indptr[v + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > nnz ? nnz : end;
  const int32_t a = comm[v];
  int64_t s = 0;
  for (int64_t e = beg + lane; e < end; e += kWave) {
    const int32_t u = indices[e];
    if ((uint32_t)u < (uint32_t)n && comm[u] == a) s += w[e];
  }
  s = wave_sum_i64(s);
  if (lane == 0 && (uint32_t)a < (uint32_t)n)
    atomicAdd(reinterpret_cast<unsigned long long*>(in_c + a), (unsigned long long)(s + self_w[v]));
}

// Q = sum_c in_c / 2m - (gamma tot_c / 2m) tot_c / 2m in ONE workgroup and a fixed order: thread t adds the terms
// t, t + 256, ... in turn, then the 256 sums fold in halves.
__global__ __launch_bounds__(kQThreads) void louvain_modularity_kernel(const int64_t* __restrict__ in_c,
                                                                       const int64_t* __restrict__ tot, int64_t n, double gamma,
                                                                       double two_m, double* __restrict__ q) {
  __shared__ double part[kQThreads];
  double acc = 0.0;
  for (int64_t c = threadIdx.x; c < n; c += kQThreads) {
    const double x = (double)tot[c] / two_m;
    acc += (double)in_c[c] / two_m - (gamma * x) * x;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kQThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) q[0] = part[0];
}

int knn_check_sizes(const char* who, int64_t n, int64_t d, int64_t k) {
  SEGGER_REQUIRE(n >= 1, "%s: n must be at least 1", who);
  SEGGER_REQUIRE(n <= 0x7fffffffLL, "%s: 2^31 rows or more", who);
  SEGGER_REQUIRE(d >= 1 && d <= SEGGER_KNN_BF_MAX_D, "%s: d = %lld outside 1 .. %d", who, (long long)d, SEGGER_KNN_BF_MAX_D);
  SEGGER_REQUIRE(k >= 1 && k <= SEGGER_KNN_BF_MAX_K, "%s: k = %lld outside 1 .. %d", who, (long long)k, SEGGER_KNN_BF_MAX_K);
  SEGGER_REQUIRE(k <= n, "%s: k = %lld above n = %lld", who, (long long)k, (long long)n);
  return SEGGER_OK;
}

int graph_check(const char* who, const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz) {
  SEGGER_REQUIRE(n >= 0, "%s: negative n", who);
  SEGGER_REQUIRE(n <= 0x7fffffffLL, "%s: 2^31 vertices or more", who);
  SEGGER_REQUIRE(nnz >= 0, "%s: negative nnz", who);
  SEGGER_REQUIRE(indptr && (nnz == 0 || indices), "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(indptr, 8) && is_aligned(indices, 4), "%s: indptr must be 8-byte and indices 4-byte aligned", who);
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_knn_bruteforce_slabs(int64_t n, int32_t d, int32_t k) {
  const int rc = knn_check_sizes("segger_knn_bruteforce_slabs", n, d, k);
  if (rc != SEGGER_OK) return rc;
  return knn_plan(n, d, k).n_slabs;
}

extern "C" int64_t segger_knn_bruteforce_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  const int rc = knn_check_sizes("segger_knn_bruteforce_workspace_bytes", n, d, k);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)knn_plan(n, d, k).total;
}

extern "C" int segger_knn_bruteforce(const float* X, int64_t n, int32_t d, int32_t k, int32_t* idx, float* dist2,
                                     void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_knn_bruteforce";
  hipStream_t stream = (hipStream_t)stream_;
  int rc = knn_check_sizes(who, n, d, k);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(X && idx && dist2 && workspace, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(X, 4) && is_aligned(idx, 4) && is_aligned(dist2, 4), "%s: X, idx and dist2 must be 4-byte aligned",
                 who);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  const KnnPlan plan = knn_plan(n, d, k);
  if ((size_t)workspace_bytes < plan.total) return workspace_too_small(who, (size_t)workspace_bytes, plan.total);
  float* norm = at<float>(workspace, plan.norm);
  uint64_t* partial = at<uint64_t>(workspace, plan.partial);
  hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)ceil_div(n, kRowThreads)), dim3(kRowThreads), 0, stream, X, n, (int)d, norm);
  SEGGER_LAUNCH_CHECK("knn_norm_kernel");
  if (d <= 32) rc = knn_select_launch<32>(X, norm, n, d, k, plan, partial, stream);
  else if (d <= 64) rc = knn_select_launch<64>(X, norm, n, d, k, plan, partial, stream);
  else if (d <= 128) rc = knn_select_launch<128>(X, norm, n, d, k, plan, partial, stream);
  else rc = knn_select_launch<256>(X, norm, n, d, k, plan, partial, stream);
  if (rc != SEGGER_OK) return rc;
  hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)ceil_div(n, kRowWaves)), dim3(kRowThreads), 0, stream, X, n, (int)d,
                     (int)k, plan.n_slabs, (const uint64_t*)partial, idx, dist2);
  SEGGER_LAUNCH_CHECK("knn_finish_kernel");
  return SEGGER_OK;
}

extern "C" int segger_jaccard_weights(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, double* weight,
                                      segger_stream_t stream_) {
  const char* who = "segger_jaccard_weights";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = graph_check(who, indptr, indices, n, nnz);
  if (rc != SEGGER_OK) return rc;
  if (n == 0 || nnz == 0) return SEGGER_OK;
  SEGGER_REQUIRE(weight, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(weight, 8), "%s: weight must be 8-byte aligned", who);
  hipLaunchKernelGGL(jaccard_kernel, dim3((unsigned)ceil_div(nnz, kRowThreads)), dim3(kRowThreads), 0, stream, indptr, indices, n,
                     nnz, weight);
  SEGGER_LAUNCH_CHECK("jaccard_kernel");
  return SEGGER_OK;
}

extern "C" int segger_louvain_move(const int64_t* indptr, const int32_t* indices, const int64_t* weight, const int64_t* kdeg,
                                   int64_t n, int64_t nnz, int32_t sub, int32_t n_sub, double gamma, double two_m,
                                   int32_t* comm, int64_t* tot, int32_t* size, int32_t* proposal, segger_stream_t stream_) {
  const char* who = "segger_louvain_move";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = graph_check(who, indptr, indices, n, nnz);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(n_sub >= 1 && n_sub <= SEGGER_LOUVAIN_MAX_SUBROUNDS && sub >= 0 && sub < n_sub,
                 "%s: sub = %d outside 0 .. n_sub - 1, n_sub = %d outside 1 .. %d", who, (int)sub, (int)n_sub,
                 SEGGER_LOUVAIN_MAX_SUBROUNDS);
  SEGGER_REQUIRE(two_m > 0.0 && gamma >= 0.0, "%s: two_m must be positive and gamma not negative", who);
  if (n == 0) return SEGGER_OK;
  SEGGER_REQUIRE(kdeg && comm && tot && size && proposal && (nnz == 0 || weight), "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(weight, 8) && is_aligned(kdeg, 8) && is_aligned(tot, 8) && is_aligned(comm, 4) &&
                     is_aligned(size, 4) && is_aligned(proposal, 4),
                 "%s: weight, kdeg and tot must be 8-byte, comm, size and proposal 4-byte aligned", who);
  const int64_t active = ceil_div(n - sub > 0 ? n - sub : 0, n_sub);
  if (active == 0) return SEGGER_OK;
  hipLaunchKernelGGL(louvain_move_kernel, dim3((unsigned)ceil_div(active, kRowWaves)), dim3(kRowThreads), 0, stream, indptr,
                     indices, weight, kdeg, (const int32_t*)comm, (const int64_t*)tot, (const int32_t*)size, n, nnz, (int)sub,
                     (int)n_sub, gamma, two_m, proposal);
  SEGGER_LAUNCH_CHECK("louvain_move_kernel");
  hipLaunchKernelGGL(louvain_apply_kernel, dim3((unsigned)ceil_div(active, kRowThreads)), dim3(kRowThreads), 0, stream,
                     (const int32_t*)proposal, kdeg, n, (int)sub, (int)n_sub, comm, tot, size);
  SEGGER_LAUNCH_CHECK("louvain_apply_kernel");
  return SEGGER_OK;
}

extern "C" int segger_louvain_modularity(const int64_t* indptr, const int32_t* indices, const int64_t* weight,
                                         const int64_t* self_weight, const int32_t* comm, const int64_t* tot, int64_t n,
                                         int64_t nnz, double gamma, double two_m, int64_t* in_c, double* q,
                                         segger_stream_t stream_) {
  const char* who = "segger_louvain_modularity";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = graph_check(who, indptr, indices, n, nnz);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(two_m > 0.0 && gamma >= 0.0, "%s: two_m must be positive and gamma not negative", who);
  SEGGER_REQUIRE(q && (n == 0 || (self_weight && comm && tot && in_c)) && (nnz == 0 || weight), "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(weight, 8) && is_aligned(self_weight, 8) && is_aligned(tot, 8) && is_aligned(in_c, 8) &&
                     is_aligned(q, 8) && is_aligned(comm, 4),
                 "%s: weight, self_weight, tot, in_c and q must be 8-byte, comm 4-byte aligned", who);
  if (n > 0) {
    SEGGER_HIP(hipMemsetAsync(in_c, 0, (size_t)n * sizeof(int64_t), stream));
    hipLaunchKernelGGL(louvain_internal_kernel, dim3((unsigned)ceil_div(n, kRowWaves)), dim3(kRowThreads), 0, stream, indptr,
                       indices, weight, self_weight, comm, n, nnz, in_c);
    SEGGER_LAUNCH_CHECK("louvain_internal_kernel");
  }
  hipLaunchKernelGGL(louvain_modularity_kernel, dim3(1), dim3(kQThreads), 0, stream, (const int64_t*)in_c, tot, n, gamma, two_m, q);
  SEGGER_LAUNCH_CHECK("louvain_modularity_kernel");
  return SEGGER_OK;
}
