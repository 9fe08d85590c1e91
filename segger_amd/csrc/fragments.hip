// segger_fragments_update / segger_fragments_finalize: the kernels behind segger_amd.fragments (include/segger_amd.h has
// the contract, DESIGN 3.5p the reasoning).  Unassigned transcripts that are neighbours in the transcript graph and whose
// embeddings agree are grouped into connected components; components of min_size or more become extra cells.
//
// Update, one launch per batch, 64 edges per wave step:
//   A  one lane per edge reads the two local ids, the source's mask, the two global ids and their `unassigned` bytes.  An id
//      outside its range is counted and never used as an address.
//   B  the live edges of the step are compacted by ballot into a wave-private LDS strip (16 bytes an edge); groups of W lanes
//      then take one live edge each, gather the two rows and reduce dot, |a|^2 and |b|^2 by xor shuffles.  W is the number of
//      16-byte pieces of a row rounded up to a power of two (elements, for rows that are not 16-byte multiples), so a row is
//      one load instruction of its group and no lane of the group idles; dead edges cost no gather.
//   C  the group's first lane compares the cosine with min_similarity and unites the endpoints in `parent`.
// The union hooks the larger root under the smaller with an agent-scope compare-and-swap and retries from the value the CAS
// returns; parent[x] <= x always, so a component's final root is its smallest id.  Every value ever stored in parent[x] is
// an ancestor of x (or x), and the ancestors of a node only grow: a read served from another XCD's stale L2 line walks an
// older, still valid chain -- it can make a CAS fail (a retry) and cannot join what is not joined.  Loads and path-halving
// stores of `parent` are relaxed agent-scope atomics.  Integer atomics only; nothing here adds floats.
//
// Finalize: compress every candidate's chain to its root and count members per root (integer atomics), flag the roots with min_size
// members or more, rank the flagged roots in index order (a count per 2048-index chunk, the one-workgroup scan over the
// chunks, a scan inside each chunk), write root / size per fragment and first_id + rank per member.
#include <math.h>

#include "common.h"
#include "post_common.h"

#pragma clang fp contract(off)       // the cosine's multiply and divide are rounded on their own

namespace segger {
namespace {

constexpr int kFragThreads = 256;
constexpr int kFragWaves = kFragThreads / kWave;
constexpr int kFragChunk = SEGGER_FRAGMENTS_CHUNK;               // indices per rank chunk
constexpr int kFragPerThread = kFragChunk / kFragThreads;
static_assert(kFragChunk % kFragThreads == 0, "a chunk is whole steps of the workgroup");

// counters: the words of SEGGER_FRAGMENTS_COUNTERS
enum { kCntEdges = 0, kCntLive, kCntKept, kCntBad, kCntCandidates, kCntComponents, kCntFragments, kCntBadParent };

__device__ __forceinline__ int32_t parent_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void parent_store(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root the chain from x reaches, halving the path on the way.  A value outside [0, x] is no parent (it cannot come from
// these kernels): the walk stops there and never follows it.
__device__ __forceinline__ int32_t find_root(int32_t* __restrict__ parent, int32_t x, bool* bad = nullptr) {
  int32_t p = parent_load(parent + x);
  while (p != x) {
    if ((uint32_t)p > (uint32_t)x) { if (bad) *bad = true; return x; }
    const int32_t gp = parent_load(parent + p);
    if ((uint32_t)gp > (uint32_t)p) { if (bad) *bad = true; return p; }
    if (gp != p) parent_store(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    int32_t expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    if ((uint32_t)expected >= (uint32_t)hi) return;      // no parent these kernels wrote: never followed
    a = expected;                    // hi had a parent already: go on from it (it is below hi, so this ends)
    b = lo;
  }
}

template <typename T> __device__ __forceinline__ float elem_f32(const T* p);
template <> __device__ __forceinline__ float elem_f32<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float elem_f32<bf16_t>(const bf16_t* p) { return __uint_as_float((uint32_t)p->v << 16); }
template <> __device__ __forceinline__ float elem_f32<f16_t>(const f16_t* p) { return (float)__builtin_bit_cast(_Float16, p->v); }

template <typename T> struct Piece;                                  // 16 bytes of a row as fp32
template <> struct Piece<float> {
  static constexpr int kElems = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  }
};
template <> struct Piece<bf16_t> {
  static constexpr int kElems = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) { Vec8<bf16_t>::load(p, f); }
};
template <> struct Piece<f16_t> {
  static constexpr int kElems = 8;
  static __device__ __forceinline__ void load(const f16_t* p, float (&f)[8]) { Vec8<f16_t>::load(p, f); }
};

struct UpdateArgs {
  const void* z; int64_t ld_z; int channels; int log_w;
  const float* similarity; const uint8_t* edge_keep;
  const int64_t* src; const int64_t* dst; int64_t n_edges;
  const int64_t* tx_index; const uint8_t* mask; int64_t n_nodes;
  const uint8_t* unassigned; int64_t n_transcripts; float min_similarity;
  int32_t* parent; int64_t* counters;
};

// torch.cosine_similarity's form, every operation correctly rounded fp32
__device__ __forceinline__ float cosine(float dot, float aa, float bb) {
  const float eps = 1e-8f;
  const float na = fmaxf(sqrtf(aa), eps), nb = fmaxf(sqrtf(bb), eps);
  return dot / (na * nb);
}

// kMode 0: the cosine of the gathered rows | 1: similarity[e] | 2: every live edge.  kVec: rows are whole, aligned 16-byte pieces.
template <typename T, int kMode, bool kVec>
__global__ __launch_bounds__(kFragThreads) void fragments_update_kernel(const UpdateArgs a) {
  __shared__ int32_t strip[kFragWaves][kWave][4];                    // live edges of the step: local s, local d, global s, global d
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * kFragWaves;
  const int64_t n_steps = (a.n_edges + kWave - 1) / kWave;
  const int W = 1 << a.log_w, groups = kWave >> a.log_w;
  const int sub = lane & (W - 1), grp = lane >> a.log_w;
  const T* z = static_cast<const T*>(a.z);
  int n_live = 0, n_kept = 0, n_bad = 0;
  for (int64_t step = (int64_t)blockIdx.x * kFragWaves + wave; step < n_steps; step += n_waves) {        // wave-uniform
    const int64_t e = step * kWave + lane;
    bool live = false;
    int32_t ls = 0, ld = 0, gs = 0, gd = 0;
    if (e < a.n_edges) {
      const int64_t s = a.src[e], d = a.dst[e];
      if ((uint64_t)s >= (uint64_t)a.n_nodes || (uint64_t)d >= (uint64_t)a.n_nodes) {
        ++n_bad;
      } else if (!a.mask || a.mask[s]) {
        const int64_t ts = a.tx_index ? a.tx_index[s] : s, td = a.tx_index ? a.tx_index[d] : d;
        if ((uint64_t)ts >= (uint64_t)a.n_transcripts || (uint64_t)td >= (uint64_t)a.n_transcripts) {
          ++n_bad;
        } else if (ts != td && a.unassigned[ts] && a.unassigned[td]) {
          live = !a.edge_keep || a.edge_keep[e];
          ls = (int32_t)s; ld = (int32_t)d; gs = (int32_t)ts; gd = (int32_t)td;
        }
      }
    }
    n_live += live;
    if (kMode != 0) {
      if (live && (kMode == 2 || a.similarity[e] >= a.min_similarity)) {
        ++n_kept;
        unite(a.parent, gs, gd);
      }
      continue;
    }
    const unsigned long long m = __ballot(live);
    const int L = __popcll(m);
    if (L == 0) continue;
    __builtin_amdgcn_wave_barrier();                                 // the strip is wave-private: one wave's LDS ops stay in order
    if (live) {
      const int slot = __popcll(m & ((1ull << lane) - 1));
      strip[wave][slot][0] = ls; strip[wave][slot][1] = ld; strip[wave][slot][2] = gs; strip[wave][slot][3] = gd;
    }
    __builtin_amdgcn_wave_barrier();
    for (int base = 0; base < L; base += groups) {                   // wave-uniform
      const int idx = base + grp;
      const bool have = idx < L;
      float dot = 0.0f, aa = 0.0f, bb = 0.0f;
      int32_t es = 0, ed = 0;
      if (have) {
        const int32_t rs = strip[wave][idx][0], rd = strip[wave][idx][1];
        es = strip[wave][idx][2]; ed = strip[wave][idx][3];
        const T* pa = z + (int64_t)rs * a.ld_z;
        const T* pb = z + (int64_t)rd * a.ld_z;
        if (kVec) {
          constexpr int kE = Piece<T>::kElems;
          const int pieces = a.channels / kE;
          for (int c = sub; c < pieces; c += W) {
            float fa[8], fb[8];
            Piece<T>::load(pa + c * kE, fa);
            Piece<T>::load(pb + c * kE, fb);
#pragma unroll
            for (int j = 0; j < kE; ++j) {
              dot = fmaf(fa[j], fb[j], dot);
              aa = fmaf(fa[j], fa[j], aa);
              bb = fmaf(fb[j], fb[j], bb);
            }
          }
        } else {
          for (int c = sub; c < a.channels; c += W) {
            const float fa = elem_f32<T>(pa + c), fb = elem_f32<T>(pb + c);
            dot = fmaf(fa, fb, dot);
            aa = fmaf(fa, fa, aa);
            bb = fmaf(fb, fb, bb);
          }
        }
      }
      for (int w = W >> 1; w >= 1; w >>= 1) {                        // every lane of the wave takes part
        dot += __shfl_xor(dot, w, kWave);
        aa += __shfl_xor(aa, w, kWave);
        bb += __shfl_xor(bb, w, kWave);
      }
      if (have && sub == 0 && cosine(dot, aa, bb) >= a.min_similarity) {
        ++n_kept;
        unite(a.parent, es, ed);
      }
    }
  }
  n_live = wave_sum_i32(n_live);
  n_kept = wave_sum_i32(n_kept);
  n_bad = wave_sum_i32(n_bad);
  if (lane == 0) {                                                   // three adds a wave of the grid, not one an edge
    if (n_live) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + kCntLive), (unsigned long long)n_live);
    if (n_kept) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + kCntKept), (unsigned long long)n_kept);
    if (n_bad) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + kCntBad), (unsigned long long)n_bad);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + kCntEdges), (unsigned long long)a.n_edges);
}

// every candidate's chain compressed towards its root (parent[i] = the root, unless another thread's halving store lands
// later with an ancestor: fragments_label_kernel finishes the job), members counted per root
__global__ __launch_bounds__(kFragThreads) void fragments_flatten_kernel(int32_t* __restrict__ parent, const uint8_t* __restrict__ unassigned,
                                                                         int64_t n, int32_t* __restrict__ count,
                                                                         int64_t* __restrict__ counters) {
  const int lane = threadIdx.x & (kWave - 1);
  int n_cand = 0, n_comp = 0, n_bad = 0;
  const int64_t stride = (int64_t)gridDim.x * kFragThreads;
  for (int64_t i = (int64_t)blockIdx.x * kFragThreads + threadIdx.x; i < n; i += stride) {
    if (!unassigned[i]) continue;
    bool bad = false;
    const int32_t r = find_root(parent, (int32_t)i, &bad);
    if (r != (int32_t)i) parent_store(parent + i, r);
    atomicAdd(count + r, 1);
    ++n_cand;
    n_comp += r == (int32_t)i;
    n_bad += bad;
  }
  n_cand = wave_sum_i32(n_cand);
  n_comp = wave_sum_i32(n_comp);
  n_bad = wave_sum_i32(n_bad);
  if (lane == 0) {
    if (n_cand) atomicAdd(reinterpret_cast<unsigned long long*>(counters + kCntCandidates), (unsigned long long)n_cand);
    if (n_comp) atomicAdd(reinterpret_cast<unsigned long long*>(counters + kCntComponents), (unsigned long long)n_comp);
    if (n_bad) atomicAdd(reinterpret_cast<unsigned long long*>(counters + kCntBadParent), (unsigned long long)n_bad);
  }
}

__device__ __forceinline__ bool is_fragment_root(const int32_t* parent, const uint8_t* unassigned, const int32_t* count, int64_t i,
                                                 int64_t min_size) {
  return unassigned[i] && parent[i] == (int32_t)i && (int64_t)count[i] >= min_size;
}

// chunk_tot[c + 1] = the fragment roots among the indices of chunk c; one workgroup a chunk
__global__ __launch_bounds__(kFragThreads) void fragments_flag_kernel(const int32_t* __restrict__ parent, const uint8_t* __restrict__ unassigned,
                                                                      const int32_t* __restrict__ count, int64_t n, int64_t min_size,
                                                                      int64_t* __restrict__ chunk_tot) {
  __shared__ int part[kFragWaves];
  const int64_t base = (int64_t)blockIdx.x * kFragChunk;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kFragPerThread; ++k) {
    const int64_t i = base + k * kFragThreads + threadIdx.x;
    if (i < n) mine += is_fragment_root(parent, unassigned, count, i, min_size);
  }
  mine = wave_sum_i32(mine);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kFragWaves; ++w) t += part[w];
    chunk_tot[blockIdx.x + 1] = t;
  }
}

// after the scan of chunk_tot: root / size of every fragment in index order, and count[i] = the rank of a fragment root, -1
// of every other index
__global__ __launch_bounds__(kFragThreads) void fragments_rank_kernel(const int32_t* __restrict__ parent, const uint8_t* __restrict__ unassigned,
                                                                      int32_t* __restrict__ count, int64_t n, int64_t min_size,
                                                                      const int64_t* __restrict__ chunk_tot, int32_t* __restrict__ root,
                                                                      int32_t* __restrict__ size, int64_t capacity) {
  __shared__ int64_t totals[kFragWaves];
  GroupScan<kFragThreads, int64_t> scan{totals, chunk_tot[blockIdx.x]};
  const int64_t base = (int64_t)blockIdx.x * kFragChunk;
  for (int k = 0; k < kFragPerThread; ++k) {                         // uniform: every thread of the workgroup steps
    const int64_t i = base + k * kFragThreads + threadIdx.x;
    const bool flag = i < n && is_fragment_root(parent, unassigned, count, i, min_size);
    const int64_t rank = scan.step(flag ? 1 : 0);
    if (i < n) {
      if (flag && rank < capacity) {
        root[rank] = (int32_t)i;
        size[rank] = count[i];
      }
      count[i] = flag ? (int32_t)rank : -1;
    }
  }
}

// fragment[i] = first_id + the rank of i's root, and parent[i] = that root.  The flatten pass leaves parent[i] at the root or at
// an ancestor (another thread's halving store may land after i's own): the short rest of the chain is walked here, read-only
// but for the thread's own entry, so that afterwards parent[i] is the root of every candidate.
__global__ __launch_bounds__(kFragThreads) void fragments_label_kernel(int32_t* __restrict__ parent, const uint8_t* __restrict__ unassigned,
                                                                       const int32_t* __restrict__ rank, int64_t n, int64_t first_id,
                                                                       int64_t* __restrict__ fragment) {
  const int64_t stride = (int64_t)gridDim.x * kFragThreads;
  for (int64_t i = (int64_t)blockIdx.x * kFragThreads + threadIdx.x; i < n; i += stride) {
    int64_t f = -1;
    if (unassigned[i]) {
      int32_t r = (int32_t)i;
      for (;;) {
        const int32_t p = parent_load(parent + r);
        if (p == r || (uint32_t)p > (uint32_t)r) break;             // the root (or no parent these kernels wrote: never followed)
        r = p;
      }
      if (r != (int32_t)i) parent_store(parent + i, r);
      const int32_t k = rank[r];
      if (k >= 0) f = first_id + k;
    }
    fragment[i] = f;
  }
}

int pow2_log_at_least(int64_t v) {                                   // the smallest l in 0 .. 6 with 2^l >= v (6 beyond 64)
  int l = 0;
  while (l < 6 && ((int64_t)1 << l) < v) ++l;
  return l;
}

template <typename T, int kMode>
int launch_update(const UpdateArgs& a, bool vec, hipStream_t stream) {
  const unsigned grid = grid_stride_blocks(ceil_div(a.n_edges, kWave) * kWave, kFragThreads, (int64_t)cu_count_or_default() * 8);
  if (vec) hipLaunchKernelGGL((fragments_update_kernel<T, kMode, true>), dim3(grid), dim3(kFragThreads), 0, stream, a);
  else hipLaunchKernelGGL((fragments_update_kernel<T, kMode, false>), dim3(grid), dim3(kFragThreads), 0, stream, a);
  SEGGER_LAUNCH_CHECK("fragments_update_kernel");
  return SEGGER_OK;
}

struct FinalizeLayout { size_t count, chunk_tot, total; int64_t n_chunks; };
FinalizeLayout finalize_layout(int64_t n) {
  FinalizeLayout l;
  Carver c;
  l.n_chunks = ceil_div(n, kFragChunk);
  l.count = c.take((size_t)n * sizeof(int32_t));
  l.chunk_tot = c.take((size_t)(l.n_chunks + 1) * sizeof(int64_t));
  l.total = c.total();
  return l;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int segger_fragments_update(const void* z, int64_t ld_z, int32_t channels, int32_t dtype, const float* similarity,
                                       const uint8_t* edge_keep, const int64_t* src, const int64_t* dst, int64_t n_edges,
                                       const int64_t* tx_index, const uint8_t* mask, int64_t n_nodes, const uint8_t* unassigned,
                                       int64_t n_transcripts, float min_similarity, int32_t* parent, int64_t* counters,
                                       segger_stream_t stream_) {
  const char* who = "segger_fragments_update";
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_edges >= 0 && n_nodes >= 0, "%s: negative n_edges or n_nodes", who);
  SEGGER_REQUIRE(n_transcripts >= 1 && n_transcripts < 0x80000000LL, "%s: n_transcripts outside [1, 2^31)", who);
  SEGGER_REQUIRE(n_nodes < 0x80000000LL, "%s: 2^31 nodes or more in a batch", who);
  SEGGER_REQUIRE(!(z && similarity), "%s: both z and similarity given", who);
  SEGGER_REQUIRE(!isnan(min_similarity), "%s: min_similarity is NaN", who);
  if (z) {
    SEGGER_REQUIRE(channels >= 1 && channels <= SEGGER_FRAGMENTS_MAX_CHANNELS, "%s: channels = %d outside 1 .. %d", who,
                   (int)channels, SEGGER_FRAGMENTS_MAX_CHANNELS);
    SEGGER_REQUIRE(dtype == SEGGER_F32 || dtype == SEGGER_BF16 || dtype == SEGGER_F16, "%s: unknown dtype %d", who, (int)dtype);
    SEGGER_REQUIRE(ld_z >= channels, "%s: ld_z < channels", who);
    SEGGER_REQUIRE(is_aligned(z, dtype == SEGGER_F32 ? 4 : 2), "%s: z must be aligned to its element size", who);
  }
  if (n_edges == 0) return SEGGER_OK;
  SEGGER_REQUIRE(src && dst && unassigned && parent && counters, "%s: NULL pointer", who);
  SEGGER_REQUIRE(n_nodes >= 1, "%s: edges but n_nodes = 0", who);
  SEGGER_REQUIRE(is_aligned(src, 8) && is_aligned(dst, 8) && is_aligned(tx_index, 8) && is_aligned(counters, 8),
                 "%s: src, dst, tx_index and counters must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(parent, 4) && is_aligned(similarity, 4), "%s: parent and similarity must be 4-byte aligned", who);
  UpdateArgs a;
  a.z = z; a.ld_z = ld_z; a.channels = (int)channels; a.log_w = 0;
  a.similarity = similarity; a.edge_keep = edge_keep;
  a.src = src; a.dst = dst; a.n_edges = n_edges;
  a.tx_index = tx_index; a.mask = mask; a.n_nodes = n_nodes;
  a.unassigned = unassigned; a.n_transcripts = n_transcripts; a.min_similarity = min_similarity;
  a.parent = parent; a.counters = counters;
  if (!z) return similarity ? launch_update<float, 1>(a, false, stream) : launch_update<float, 2>(a, false, stream);
  return dispatch_dtype(dtype, who, [&](auto t) {
    using T = elem_t<decltype(t)>;
    const size_t row_bytes = (size_t)channels * sizeof(T);
    const bool vec = row_bytes % 16 == 0 && ((size_t)ld_z * sizeof(T)) % 16 == 0 && is_aligned(z, 16);
    a.log_w = pow2_log_at_least(vec ? (int64_t)(row_bytes / 16) : (int64_t)channels);
    return launch_update<T, 0>(a, vec, stream);
  });
}

extern "C" int segger_fragments_finalize(int32_t* parent, const uint8_t* unassigned, int64_t n_transcripts, int64_t min_size,
                                         int64_t first_id, int64_t* fragment, int32_t* root, int32_t* size, int64_t capacity,
                                         int64_t* counters, void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_fragments_finalize";
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = n_transcripts;
  SEGGER_REQUIRE(n >= 1 && n < 0x80000000LL, "%s: n_transcripts outside [1, 2^31)", who);
  SEGGER_REQUIRE(min_size >= 1, "%s: min_size must be >= 1", who);
  SEGGER_REQUIRE(first_id >= 0 && first_id <= INT64_MAX - n, "%s: first_id outside [0, 2^63 - n_transcripts)", who);
  SEGGER_REQUIRE(capacity >= 0, "%s: negative capacity", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(parent && unassigned && fragment && counters && workspace, "%s: NULL pointer", who);
  SEGGER_REQUIRE(capacity == 0 || (root && size), "%s: NULL root or size", who);
  SEGGER_REQUIRE(is_aligned(fragment, 8) && is_aligned(counters, 8), "%s: fragment and counters must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(parent, 4) && is_aligned(root, 4) && is_aligned(size, 4), "%s: parent, root and size must be 4-byte aligned",
                 who);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  const FinalizeLayout l = finalize_layout(n);
  if ((size_t)workspace_bytes < l.total) return workspace_too_small(who, (size_t)workspace_bytes, l.total);
  int32_t* count = at<int32_t>(workspace, l.count);
  int64_t* chunk_tot = at<int64_t>(workspace, l.chunk_tot);
  SEGGER_HIP(hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), stream));
  SEGGER_HIP(hipMemsetAsync(counters + kCntCandidates, 0, 4 * sizeof(int64_t), stream));
  const unsigned grid = grid_stride_blocks(n, kFragThreads, (int64_t)cu_count_or_default() * 8);
  hipLaunchKernelGGL(fragments_flatten_kernel, dim3(grid), dim3(kFragThreads), 0, stream, parent, unassigned, n, count, counters);
  SEGGER_LAUNCH_CHECK("fragments_flatten_kernel");
  hipLaunchKernelGGL(fragments_flag_kernel, dim3((unsigned)l.n_chunks), dim3(kFragThreads), 0, stream, parent, unassigned, count, n,
                     min_size, chunk_tot);
  SEGGER_LAUNCH_CHECK("fragments_flag_kernel");
  hipLaunchKernelGGL((counts_to_offsets_kernel<int64_t>), dim3(1), dim3(kScanThreads), 0, stream, chunk_tot, l.n_chunks,
                     counters + kCntFragments);
  SEGGER_LAUNCH_CHECK("counts_to_offsets_kernel");
  hipLaunchKernelGGL(fragments_rank_kernel, dim3((unsigned)l.n_chunks), dim3(kFragThreads), 0, stream, parent, unassigned, count, n,
                     min_size, chunk_tot, root, size, capacity);
  SEGGER_LAUNCH_CHECK("fragments_rank_kernel");
  hipLaunchKernelGGL(fragments_label_kernel, dim3(grid), dim3(kFragThreads), 0, stream, parent, unassigned, count, n, first_id, fragment);
  SEGGER_LAUNCH_CHECK("fragments_label_kernel");
  return SEGGER_OK;
}
