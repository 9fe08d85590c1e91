// The front end and the back end that the two units writing one ring per cell share (boundaries.hip: the convex hull;
// outlines.hip: the pruned Delaunay outline; included after rings.h and sort_config.h).  Front: the key of a row, the
// position where a cell starts in the sorted keys, the segments.  Back: the scan that keeps the cells with a ring and
// places them, and the emit kernel with its Chaikin stage.  In between each unit runs its own kernels, which write ring
// vertex k of segment j to hull[head[j] + k] and the ring's length to hull_n[j].  The kernels are defined here, in an
// unnamed namespace: every including unit gets its own copies under the same names, and a fix is made once.
#pragma once
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kBndThreads = 256;
constexpr int kBndWaves = kBndThreads / kWave;
constexpr int kBndScanThreads = 1024;

// the head of the counters block of both entry points
enum { kCounted = 0, kPresent = 1, kKept = 2, kVerts = 3, kBadCell = 4, kNonFinite = 5, kRefused = 6, kRefusedCell = 7 };

// ---------------------------------------------------------------- keys ---
__global__ __launch_bounds__(kBndThreads) void bnd_keys_kernel(const double* __restrict__ xy, const int32_t* __restrict__ cell,
                                                               const uint8_t* __restrict__ keep, int64_t n, int64_t n_cells,
                                                               unsigned long long* __restrict__ keys,
                                                               unsigned long long* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kBndThreads;
  const unsigned long long sentinel = (unsigned long long)n_cells << 32;
  int n_counted = 0, n_bad = 0, n_nonfinite = 0;                     // at most 2^31 / (256 * grid) + 1 rows per thread
  for (int64_t i = (int64_t)blockIdx.x * kBndThreads + threadIdx.x; i < n; i += stride) {
    const int32_t c = cell[i];
    unsigned long long key = sentinel;
    if (c >= 0 && (!keep || keep[i])) {
      if ((int64_t)c >= n_cells) ++n_bad;
      else {
        const double2 p = reinterpret_cast<const double2*>(xy)[i];
        if (p.x - p.x == 0.0 && p.y - p.y == 0.0) {                  // finite
          key = ((unsigned long long)(uint32_t)c << 32) | (unsigned long long)i;
          ++n_counted;
        } else ++n_nonfinite;
      }
    }
    keys[i] = key;
  }
  n_counted = wave_sum_i32(n_counted);
  n_bad = wave_sum_i32(n_bad);
  n_nonfinite = wave_sum_i32(n_nonfinite);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (n_counted) atomicAdd(counters + kCounted, (unsigned long long)n_counted);
    if (n_bad) atomicAdd(counters + kBadCell, (unsigned long long)n_bad);
    if (n_nonfinite) atomicAdd(counters + kNonFinite, (unsigned long long)n_nonfinite);
  }
}

// position p of the sorted order starts a cell: a real key whose cell differs from its predecessor's
struct BndCellHead {
  const unsigned long long* keys;
  unsigned long long sentinel;
  __host__ __device__ bool operator()(const int32_t& p) const {
    const unsigned long long k = keys[p];
    return k < sentinel && (p == 0 || (keys[p - 1] >> 32) != (k >> 32));
  }
};

// ---------------------------------------------------------------- segments ---
struct BndSegs {
  const unsigned long long* keys;                                    // sorted
  const int32_t* head;                                               // [present] first sorted position of a present cell
  int32_t* len;                                                      // [present] its counted rows
  int32_t* hull_n;                                                   // [present] its ring's vertices; 0: none, or refused
  double2* hull;                                                     // [n_rows] ring vertex k of segment j at head[j] + k
};

// sorted position s of the keys -> the point of its row, -0.0 as +0.0 (equal points then have equal bits, and which of
// them a cell's kernel meets first cannot show in the output)
__device__ __forceinline__ P2 point_at(const double* __restrict__ xy, const unsigned long long* __restrict__ keys, int64_t s) {
  const double2 p = reinterpret_cast<const double2*>(xy)[keys[s] & 0xffffffffull];
  return P2{p.x + 0.0, p.y + 0.0};
}

// ---------------------------------------------------------------- keep and scan ---
// One workgroup over the present cells in ascending cell id: a cell with h >= 3 is kept; its position among the kept and
// the exclusive sum of h << smoothing before it are its row of the outputs and its ring offset.
__global__ __launch_bounds__(kBndScanThreads) void bnd_scan_kernel(BndSegs s, int smoothing, int32_t* __restrict__ kept_seg,
                                                                   int64_t* __restrict__ ring_offsets, int32_t* __restrict__ cell_ids,
                                                                   int64_t* __restrict__ n_transcripts,
                                                                   unsigned long long* __restrict__ counters) {
  __shared__ int64_t wave_verts[kBndScanThreads / kWave];
  __shared__ int wave_kept[kBndScanThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t present = (int64_t)counters[kPresent];
  int64_t carry_v = 0;                                               // vertices and kept cells before this chunk
  int carry_k = 0;
  for (int64_t base = 0; base < present; base += kBndScanThreads) {
    const int64_t j = base + threadIdx.x;
    const int h = j < present ? s.hull_n[j] : 0;
    const bool kept = h >= 3;
    const int64_t mine = kept ? (int64_t)h << smoothing : 0;
    int64_t v = mine;
    int k = kept ? 1 : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {                            // inclusive scans of the wave
      const int src = lane >= d ? lane - d : lane;
      const int64_t ov = (int64_t)shfl64((uint64_t)v, src);
      const int ok = __shfl(k, src, kWave);
      if (lane >= d) { v += ov; k += ok; }
    }
    if (lane == kWave - 1) { wave_verts[wave] = v; wave_kept[wave] = k; }
    __syncthreads();
    int64_t before_v = carry_v, all_v = carry_v;
    int before_k = carry_k, all_k = carry_k;
    for (int w = 0; w < kBndScanThreads / kWave; ++w) {
      const int64_t tv = wave_verts[w];
      const int tk = wave_kept[w];
      if (w < wave) { before_v += tv; before_k += tk; }
      all_v += tv;
      all_k += tk;
    }
    if (kept) {
      const int q = before_k + k - 1;
      kept_seg[q] = (int32_t)j;
      ring_offsets[q] = before_v + v - mine;
      cell_ids[q] = (int32_t)(s.keys[s.head[j]] >> 32);
      n_transcripts[q] = (int64_t)s.len[j];
    }
    carry_v = all_v;
    carry_k = all_k;
    __syncthreads();                                                 // the totals are rewritten by the next chunk
  }
  if (threadIdx.x == 0) {
    ring_offsets[carry_k] = carry_v;
    counters[kKept] = (unsigned long long)carry_k;
    counters[kVerts] = (unsigned long long)carry_v;
  }
}

// ---------------------------------------------------------------- emit ---
// Vertex j of the ring after S Chaikin iterations of the h-vertex ring.  A vertex of level l (the ring after l
// iterations, 2^l h vertices) with index q comes from the vertices q >> 1 and (q >> 1) + 1 of level l - 1, so vertex j of
// level S depends on S + 1 consecutive (cyclic) ring vertices from j >> S on.  w holds, level after level, the S - l + 1
// consecutive vertices of level l from index j >> (S - l) on; which two entries of the previous level make entry t
// depends on the parity of that index alone: the array indices are compile-time constants and w stays in registers.
// f(int_c<0>{}) .. f(int_c<N - 1>{}): a loop whose counter is a constant expression in its body
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(int_c<N - 1>{});
  }
}

// N + 1 consecutive vertices of a level in w -> the N of the next level that start at an index of parity b, in w
template <int N>
__device__ __forceinline__ void chaikin_level(P2* w, bool b) {
  P2 nw[N];
  static_for<N>([&](auto t_) __attribute__((always_inline)) {
    constexpr int t = decltype(t_)::value;
    // (values first, then the choice: a choice between two elements would be a choice between two addresses)
    const P2 p0 = w[t >> 1], q0 = w[(t >> 1) + 1], p1 = w[(t + 1) >> 1], q1 = w[((t + 1) >> 1) + 1];
    const double px = b ? p1.x : p0.x, py = b ? p1.y : p0.y, qx = b ? q1.x : q0.x, qy = b ? q1.y : q0.y;
    const bool odd = b != ((t & 1) != 0);
    const double wp = odd ? 0.25 : 0.75, wq = odd ? 0.75 : 0.25;
    nw[t] = P2{wp * px + wq * qx, wp * py + wq * qy};
  });
  static_for<N>([&](auto t_) __attribute__((always_inline)) { w[decltype(t_)::value] = nw[decltype(t_)::value]; });
}

template <int S>
__device__ __forceinline__ P2 chaikin_vertex(const double2* __restrict__ hull, int h, int j) {
  P2 w[S + 1];
  const int first = j >> S;
  static_for<S + 1>([&](auto t_) __attribute__((always_inline)) {
    constexpr int t = decltype(t_)::value;
    const double2 p = hull[(first + t) % h];
    w[t] = P2{p.x, p.y};
  });
  static_for<S>([&](auto l_) __attribute__((always_inline)) {
    constexpr int l = decltype(l_)::value + 1;
    // entries 0 .. S - l of level l from entries 0 .. S - l + 1 of level l - 1; the parity of this level's first index
    chaikin_level<S - l + 1>(w, ((j >> (S - l)) & 1) != 0);
  });
  return w[0];
}

template <int S>
__global__ __launch_bounds__(kBndThreads) void bnd_emit_kernel(BndSegs s, const int32_t* __restrict__ kept_seg,
                                                               const int64_t* __restrict__ ring_offsets,
                                                               const unsigned long long* __restrict__ counters,
                                                               double2* __restrict__ xy_out, int64_t capacity) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t K = (int64_t)counters[kKept];
  const int64_t n_waves = (int64_t)gridDim.x * kBndWaves;
  for (int64_t q = (int64_t)blockIdx.x * kBndWaves + (threadIdx.x >> 6); q < K; q += n_waves) {                 // wave-uniform
    const int j = kept_seg[q];
    const int h = s.hull_n[j];
    const double2* hull = s.hull + s.head[j];
    const int64_t at0 = ring_offsets[q];
    const int total = h << S;
    for (int v = lane; v < total; v += kWave) {
      const P2 p = chaikin_vertex<S>(hull, h, v);
      if (at0 + v < capacity) xy_out[at0 + v] = double2{p.x, p.y};
    }
  }
}

// ---------------------------------------------------------------- host ---
int bnd_check_sizes(const char* who, int64_t n_rows, int64_t n_cells) {
  SEGGER_REQUIRE(n_rows >= 0, "%s: negative n_rows", who);
  SEGGER_REQUIRE(n_rows < 0x7fffffffLL, "%s: 2^31 - 1 rows or more", who);
  SEGGER_REQUIRE(n_cells >= 1 && n_cells <= 0x7fffffffLL, "%s: n_cells = %lld outside 1 .. 2^31 - 1", who, (long long)n_cells);
  return SEGGER_OK;
}

template <int S>
void launch_emit(unsigned grid, hipStream_t stream, const BndSegs& s, const int32_t* kept_seg, const int64_t* ring_offsets,
                 const unsigned long long* counters, double2* xy_out, int64_t capacity) {
  hipLaunchKernelGGL((bnd_emit_kernel<S>), dim3(grid), dim3(kBndThreads), 0, stream, s, kept_seg, ring_offsets, counters, xy_out,
                     capacity);
}

// the emit kernel of `smoothing` (0 .. SEGGER_BOUNDARY_MAX_SMOOTHING, checked by the caller)
void launch_emit_for(int smoothing, unsigned grid, hipStream_t stream, const BndSegs& s, const int32_t* kept_seg,
                     const int64_t* ring_offsets, const unsigned long long* counters, double2* xy_out, int64_t capacity) {
  switch (smoothing) {
    case 0: launch_emit<0>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
    case 1: launch_emit<1>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
    case 2: launch_emit<2>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
    case 3: launch_emit<3>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
    case 4: launch_emit<4>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
    case 5: launch_emit<5>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
    default: launch_emit<6>(grid, stream, s, kept_seg, ring_offsets, counters, xy_out, capacity); break;
  }
}

}  // namespace
}  // namespace segger
