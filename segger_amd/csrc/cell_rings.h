// The front end and the back end that the units writing one ring per cell share (boundaries.hip: the convex hull;
// outlines.hip and outlines_large.hip: the pruned Delaunay outline; included after rings.h and sort_config.h).  Front: the
// key of a row, the position where a cell starts in the sorted keys, the segments.  Back: the scan that keeps the cells with
// a ring and places them (post_common.h's GroupScan over vertices and kept cells at once), and the emit kernel with its
// Chaikin stage.  In between each unit runs its own kernels, which write ring vertex k of segment j to hull[head[j] + k] and
// the ring's length to hull_n[j].  The host half is here as well, once: the head of the workspace layout
// (take_cell_rings), the refusals of a call (bnd_check_sizes, check_cell_rings_call), the views into a workspace
// (cell_rings_views) and the launches of the front and of the back (launch_cell_rings_front / _back); a unit keeps its own
// regions, its own refusals and the launches of its own kernels.  Everything is defined in an unnamed namespace: every
// including unit gets its own copies under the same names, and a fix is made once.
#pragma once
#include <math.h>

#include "common.h"
#include "mma.h"
#include "post_common.h"
#include "rings.h"
#include "sort_config.h"

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

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
  __shared__ ScanPair totals[kBndScanThreads / kWave];
  const int64_t present = (int64_t)counters[kPresent];
  GroupScan<kBndScanThreads, ScanPair> scan{totals, ScanPair{0, 0}}; // vertices and kept cells before
  for (int64_t base = 0; base < present; base += kBndScanThreads) {
    const int64_t j = base + threadIdx.x;
    const int h = j < present ? s.hull_n[j] : 0;
    const bool kept = h >= 3;
    const ScanPair before = scan.step(ScanPair{kept ? (int64_t)h << smoothing : 0, kept ? 1 : 0});
    if (kept) {
      const int q = before.k;
      kept_seg[q] = (int32_t)j;
      ring_offsets[q] = before.v;
      cell_ids[q] = (int32_t)(s.keys[s.head[j]] >> 32);
      n_transcripts[q] = (int64_t)s.len[j];
    }
  }
  if (threadIdx.x == 0) {
    ring_offsets[scan.carry.k] = scan.carry.v;
    counters[kKept] = (unsigned long long)scan.carry.k;
    counters[kVerts] = (unsigned long long)scan.carry.v;
  }
}

// ---------------------------------------------------------------- emit ---
// Vertex j of the ring after S Chaikin iterations of the h-vertex ring.  A vertex of level l (the ring after l
// iterations, 2^l h vertices) with index q comes from the vertices q >> 1 and (q >> 1) + 1 of level l - 1, so vertex j of
// level S depends on S + 1 consecutive (cyclic) ring vertices from j >> S on.  w holds, level after level, the S - l + 1
// consecutive vertices of level l from index j >> (S - l) on; which two entries of the previous level make entry t
// depends on the parity of that index alone: the array indices are compile-time constants (mma.h's static_for) and w
// stays in registers.

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

// The regions every workspace of these units starts with, and what sizes them.  keys: the sorted keys; hull: the rings,
// and before that the unsorted keys (dead once sorted); head, len, hull_n, kept_seg: one int32 per possible cell; temp: the
// larger of the sort's and the select's.  A unit takes its own regions after these.  With n_rows and n_cells below 2^31
// every term is below 2^36 bytes: nothing here can overflow.
struct CellRingsLayout {
  RingLists rings;
  size_t keys, hull, head, len, hull_n, kept_seg, temp;
  size_t temp_bytes;
  int key_bits;
  int64_t cells_cap;
};

CellRingsLayout take_cell_rings(Carver& c, int64_t n_rows, int64_t n_cells) {
  CellRingsLayout l;
  l.key_bits = 32 + bit_length((unsigned long long)n_cells);         // the sentinel n_cells << 32 is the largest key
  const size_t n = (size_t)(n_rows > 0 ? n_rows : 1);
  l.cells_cap = n_rows < n_cells ? (n_rows > 0 ? n_rows : 1) : n_cells;
  const size_t c4 = (size_t)l.cells_cap * 4;
  l.rings = take_ring_lists(c, l.cells_cap);
  l.keys = c.take(n * 8);
  l.hull = c.take(n * 16);
  l.head = c.take(c4);
  l.len = c.take(c4);
  l.hull_n = c.take(c4);
  l.kept_seg = c.take(c4);
  size_t a = 0, b = 0;
  unsigned long long* k64 = nullptr;
  int32_t* i32 = nullptr;
  size_t* cnt = nullptr;
  (void)rocprim::radix_sort_keys<NoScratchSortConfig>(nullptr, a, k64, k64, n, 0, (unsigned)l.key_bits, (hipStream_t)0);
  (void)rocprim::select(nullptr, b, rocprim::counting_iterator<int32_t>(0), i32, cnt, n, BndCellHead{nullptr, 0}, (hipStream_t)0);
  l.temp_bytes = a > b ? a : b;
  l.temp = c.take(l.temp_bytes > 0 ? l.temp_bytes : 1);
  return l;
}

// the arguments the three entry points share
struct CellRingsCall {
  const double* xy; const int32_t* cell; const uint8_t* keep; int64_t n_rows, n_cells; int32_t smoothing;
  int64_t* ring_offsets; double* xy_out; int64_t xy_capacity; int32_t* cell_ids; int64_t* n_transcripts; uint64_t* counters;
  void* workspace; int64_t workspace_bytes;
};

// What all three refuse about a call whose sizes passed (bnd_check_sizes comes first: `need` is a layout's total, and a
// layout is defined for sizes that passed), in one order and one wording.  `unit` holds the unit's own refusals of scalar
// arguments, where they stand: after smoothing.  *empty: n_rows == 0, nothing is launched and the caller's zeroed counters
// and ring_offsets[0] stand.
template <class F>
int check_cell_rings_call(const char* who, const CellRingsCall& a, size_t need, F&& unit, bool* empty) {
  *empty = false;
  SEGGER_REQUIRE(a.smoothing >= 0 && a.smoothing <= SEGGER_BOUNDARY_MAX_SMOOTHING, "%s: smoothing = %d outside 0 .. %d", who,
                 (int)a.smoothing, SEGGER_BOUNDARY_MAX_SMOOTHING);
  const int rc = unit();
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(a.workspace_bytes >= 0 && a.xy_capacity >= 0, "%s: negative workspace_bytes or xy_capacity", who);
  if (a.n_rows == 0) {
    SEGGER_REQUIRE(a.counters && a.ring_offsets, "%s: NULL pointer", who);
    *empty = true;
    return SEGGER_OK;
  }
  SEGGER_REQUIRE(a.xy && a.cell && a.ring_offsets && a.cell_ids && a.n_transcripts && a.counters && a.workspace, "%s: NULL pointer", who);
  SEGGER_REQUIRE(a.xy_out || a.xy_capacity == 0, "%s: NULL xy_out with xy_capacity > 0", who);
  SEGGER_REQUIRE(is_aligned(a.xy, 16) && is_aligned(a.xy_out, 16), "%s: xy and xy_out must be 16-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(a.ring_offsets, 8) && is_aligned(a.n_transcripts, 8) && is_aligned(a.counters, 8),
                 "%s: ring_offsets, n_transcripts and counters must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(a.cell, 4) && is_aligned(a.cell_ids, 4), "%s: cell and cell_ids must be 4-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(a.workspace, 256), "%s: workspace must be 256-byte aligned", who);
  SEGGER_REQUIRE((size_t)a.workspace_bytes >= need, "%s: workspace %lld < %zu bytes", who, (long long)a.workspace_bytes, need);
  return SEGGER_OK;
}

// the shared regions of a workspace as pointers
struct CellRingsViews {
  int32_t *words, *list_short, *list_long, *head, *kept_seg;
  unsigned long long *keys_in, *keys;                                // unsorted, in the hull's region (dead once sorted); sorted
  char* temp;
  unsigned long long* cnt;                                           // the caller's counters
  BndSegs s;
};
CellRingsViews cell_rings_views(const CellRingsCall& a, const CellRingsLayout& l) {
  void* ws = a.workspace;
  return CellRingsViews{at<int32_t>(ws, l.rings.words), at<int32_t>(ws, l.rings.list_short), at<int32_t>(ws, l.rings.list_long),
                        at<int32_t>(ws, l.head), at<int32_t>(ws, l.kept_seg), at<unsigned long long>(ws, l.hull),
                        at<unsigned long long>(ws, l.keys), at<char>(ws, l.temp), reinterpret_cast<unsigned long long*>(a.counters),
                        BndSegs{at<unsigned long long>(ws, l.keys), at<int32_t>(ws, l.head), at<int32_t>(ws, l.len),
                                at<int32_t>(ws, l.hull_n), at<double2>(ws, l.hull)}};
}

// Front: the words and the unit's n_counters counters zeroed, the keys, the keys-only sort, the first sorted position of
// every present cell into head with their number in counters[kPresent].
int launch_cell_rings_front(const CellRingsCall& a, const CellRingsLayout& l, const CellRingsViews& v, int n_counters, int cus,
                            hipStream_t stream) {
  SEGGER_HIP(hipMemsetAsync(v.words, 0, kRingWordsBytes, stream));
  SEGGER_HIP(hipMemsetAsync(v.cnt, 0, n_counters * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(bnd_keys_kernel, dim3(grid_stride_blocks(a.n_rows, kBndThreads, (int64_t)cus * 32)), dim3(kBndThreads), 0, stream,
                     a.xy, a.cell, a.keep, a.n_rows, a.n_cells, v.keys_in, v.cnt);
  SEGGER_LAUNCH_CHECK("bnd_keys_kernel");
  size_t temp_bytes = l.temp_bytes;
  SEGGER_HIP(rocprim::radix_sort_keys<NoScratchSortConfig>(v.temp, temp_bytes, v.keys_in, v.keys, (size_t)a.n_rows, 0,
                                                           (unsigned)l.key_bits, stream));
  temp_bytes = l.temp_bytes;
  SEGGER_HIP(rocprim::select(v.temp, temp_bytes, rocprim::counting_iterator<int32_t>(0), v.head,
                             reinterpret_cast<size_t*>(v.cnt + kPresent), (size_t)a.n_rows,
                             BndCellHead{v.keys, (unsigned long long)a.n_cells << 32}, stream));
  return SEGGER_OK;
}

// Back: the kept cells placed, then their rings emitted after `smoothing` Chaikin iterations.
int launch_cell_rings_back(const CellRingsCall& a, const CellRingsLayout& l, const CellRingsViews& v, int cus, hipStream_t stream) {
  hipLaunchKernelGGL(bnd_scan_kernel, dim3(1), dim3(kBndScanThreads), 0, stream, v.s, (int)a.smoothing, v.kept_seg, a.ring_offsets,
                     a.cell_ids, a.n_transcripts, v.cnt);
  SEGGER_LAUNCH_CHECK("bnd_scan_kernel");
  launch_emit_for((int)a.smoothing, grid_stride_blocks(l.cells_cap, kBndWaves, (int64_t)cus * 8), stream, v.s, v.kept_seg,
                  a.ring_offsets, v.cnt, reinterpret_cast<double2*>(a.xy_out), a.xy_capacity);
  SEGGER_LAUNCH_CHECK("bnd_emit_kernel");
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger
