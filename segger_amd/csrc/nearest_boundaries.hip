// segger_nearest_boundaries_count / _fill / _select: for every point the k best boundaries among the polygons the join
// pairs it with, each with its squared distance to the ring and the crossing parity -- the numbers ring_distance computes
// and ring_decide folds into one bit.  include/segger_amd.h has the contract.  A prediction graph with a bounded degree ("the k nearest
// boundaries within a distance"), the signed distance of a transcript to an outline, and erosion as a mask all read them.
//
// Kernels, one stream, no host synchronisation inside an entry point:
//   near_keys_kernel, (rocprim keys sort), near_cells_kernel, near_bin_kernel   join_grid.h's bodies: the join's grid;
//   near_short_kernel   n <= 64: one wave per polygon, the ring in registers;
//   near_long_kernel    64 < n <= SEGGER_MORPH_MAX_VERTS: one single-wave workgroup per polygon, the ring in LDS (64 KB);
//   counts_to_offsets_kernel<int64>  one workgroup: candidates per point -> pair_offsets, in place;
//   near_select_kernel  one lane per point, or the whole wave for a point with more than SEGGER_NEAREST_LANE_MAX candidates.
// The two polygon kernels are rings.h's loops around walk_body, a template on count / fill and this unit's sink of the
// join's walk (ring_predicate.h: walk_grown_ring -- a candidate is a pair of the join, bit for bit; the arguments and the
// launches are join_grid.h's).  It is the sink that keeps the numbers (RingDistance) of a match.  Count: an integer atomic
// add on pair_offsets[point + 1].  Fill: the slot of a match is pair_offsets[point] + an integer atomic add on the point's
// cursor; it holds s (fp64) and the polygon id with the parity in bit 31.
//
// Why the bytes do not depend on scheduling: the atomics are integer adds, so the counts are sums; the order of a point's
// slots is arbitrary, but the selection reads a segment as a SET: entry j of the output is the smallest (key, id) above
// entry j - 1, a strict total order in which no two candidates of a point are equal (a polygon pairs with a point once).
// The selection is k passes over the segment and keeps nothing but the last pick: no list in registers, none in LDS, no
// sort.  One lane reads its point's segment k times (at most k SEGGER_NEAREST_LANE_MAX loads of 12 bytes); above that the
// 64 lanes stride over the segment and a shuffle reduction picks the minimum.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel of this unit; near_long_kernel
// holds the 65536 B ring stage, counts_to_offsets_kernel its 128 B of wave totals, every other kernel no LDS.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "ring_predicate.h"
#include "sort_config.h"
#include "join_grid.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

static_assert(SEGGER_NEAREST_ERR_OFFSETS == SEGGER_PJOIN_ERR_OFFSETS && SEGGER_NEAREST_ERR_CAP == SEGGER_PJOIN_ERR_CAP &&
              SEGGER_NEAREST_ERR_BUFFER == SEGGER_PJOIN_ERR_BUFFER && SEGGER_NEAREST_ERR_FILL == SEGGER_PJOIN_ERR_FILL,
              "the error bits mirror the join's");
static_assert(SEGGER_NEAREST_MAX_K <= kWave && SEGGER_NEAREST_LANE_MAX >= SEGGER_NEAREST_MAX_K, "a lane can hold every kept candidate");

constexpr int kNbThreads = kGridThreads;
constexpr int kNbWaves = kNbThreads / kWave;
constexpr int kCtrPairs = 0, kCtrKept = 1, kCtrTruncated = 2, kCtrMaxCount = 3;
constexpr uint32_t kParityBit = 0x80000000u, kIdMask = 0x7fffffffu;  // polygon ids are below 2^31 - 1

// ---------------------------------------------------------------- the points, the polygons: join_grid.h ---
__global__ __launch_bounds__(kNbThreads) void near_keys_kernel(const double* __restrict__ pts, int64_t n, UniformGrid g,
                                                               unsigned long long* __restrict__ keys) {
  grid_keys_body(pts, n, g, keys);
}

__global__ __launch_bounds__(kNbThreads) void near_cells_kernel(const unsigned long long* __restrict__ keys_sorted,
                                                                const double* __restrict__ pts, const int32_t*, int64_t n,
                                                                int64_t n_cells, int32_t* __restrict__ cell_start,
                                                                double2* __restrict__ sorted_pts, int32_t*) {
  grid_cells_body<false>(keys_sorted, pts, nullptr, n, n_cells, cell_start, sorted_pts, nullptr);
}

// the sizes of this unit are per point (pair_offsets, zeroed by the entry point): the binning kernel zeroes none
__global__ __launch_bounds__(kNbThreads) void near_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                              const double* __restrict__ buffer, int64_t P, int64_t V, int64_t*,
                                                              int64_t*, int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                              int32_t* __restrict__ list_long) {
  bin_rings_body(off, xy, buffer, P, V, nullptr, nullptr, words, list_short, list_long);
}

constexpr FrontKernels kNbFront{near_keys_kernel, near_cells_kernel, near_bin_kernel,
                                "near_keys_kernel", "near_cells_kernel", "near_bin_kernel"};

struct WalkArgs {
  WalkCommon c;                                                      // join_grid.h
  int64_t* pair_offsets;                                             // count: [point + 1] is added to; fill: read
  int32_t* cursor;                                                   // fill: [point], zero on entry
  double* pair_key;                                                  // fill: s of a candidate
  uint32_t* pair_polygon;                                            // fill: its polygon, the parity in bit 31
  int64_t capacity;
};

// One polygon, one wave, every lane active: r is what rings.h's loops hand over.  This unit's sink of the walk: a match is
// a candidate of its point (the join's pairs, bit for bit).
template <bool kFill, class Ring>
__device__ __forceinline__ void walk_body(const ListedRing<Ring>& r, const WalkArgs& a) {
  const int64_t p = r.p;
  walk_polygon(a.c, r, [&](bool hit, int s, const RingDistance& rd) {
    if (!hit) return;
    const int64_t id = (int64_t)(a.c.keys[s] & 0xffffffffull);       // < n_points: the keys kernel wrote it
    if (!kFill) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&a.pair_offsets[id + 1]), 1ull);
    } else {
      const int64_t begin = a.pair_offsets[id];
      int64_t end = a.pair_offsets[id + 1];
      if (end > a.capacity) end = a.capacity;                        // nothing is ever written at or beyond either
      const int64_t slot = begin + (int64_t)atomicAdd(&a.cursor[id], 1);
      if (begin >= 0 && slot < end) {
        a.pair_key[slot] = rd.best == 0.0 ? 0.0 : (rd.inside ? -rd.best : rd.best);
        a.pair_polygon[slot] = (uint32_t)p | (rd.inside ? kParityBit : 0u);
      } else {
        atomicOr(&a.c.words[kWordFlag], SEGGER_NEAREST_ERR_FILL);
      }
    }
  });
}

template <bool kFill>
__global__ __launch_bounds__(kNbThreads) void near_short_kernel(WalkArgs a, const int32_t* __restrict__ list) {
  short_ring_loop(a.c.off, a.c.xy, a.c.words, list, kNbWaves, [&](const auto& r) { walk_body<kFill>(r, a); });
}

template <bool kFill>
__global__ __launch_bounds__(kWave) void near_long_kernel(WalkArgs a, const int32_t* __restrict__ list) {
  __shared__ double2 pts[SEGGER_MORPH_MAX_VERTS];
  long_ring_loop(a.c.off, a.c.xy, a.c.words, list, pts, [&](const auto& r) { walk_body<kFill>(r, a); });
}

template <bool kFill>
constexpr RingKernels<WalkArgs> kNbRings{near_short_kernel<kFill>, "near_short_kernel", kNbWaves, 8,
                                         near_long_kernel<kFill>, "near_long_kernel", 2};

// ---------------------------------------------------------------- the selection ---
// A candidate as the selection compares it: the bits of s mapped so that their unsigned order is the order of the doubles
// (s is never -0.0: the fill writes +0.0 for dist2 == 0), then the polygon id.  idp carries the parity in bit 31.
struct Pick { uint64_t key; uint32_t idp; };

__device__ __forceinline__ uint64_t ordered_key(double s) {
  const uint64_t u = (uint64_t)__double_as_longlong(s);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t key) {
  return __longlong_as_double((long long)((key >> 63) ? (key ^ 0x8000000000000000ull) : ~key));
}
__device__ __forceinline__ bool pick_before(Pick x, Pick y) {
  return x.key < y.key || (x.key == y.key && (x.idp & kIdMask) < (y.idp & kIdMask));
}
// nothing: what a pass returns when no candidate is left; it compares after every candidate
__device__ __forceinline__ Pick no_pick() { return Pick{~0ull, kIdMask}; }

struct SelectArgs {
  const int64_t* pair_offsets;
  const double* pair_key;
  const uint32_t* pair_polygon;
  int64_t capacity, N;
  int32_t P, k;
  int32_t* polygon;                                                  // [N, k]
  double* dist2;                                                     // [N, k]
  uint8_t* inside;                                                   // [N, k]
  int32_t* count;                                                    // [N]
  unsigned long long* counters;
};

// the smallest candidate of positions begin + first, + first + step, ... < begin + c that comes after `last` (any, if !have)
__device__ __forceinline__ Pick next_pick(const SelectArgs& a, int64_t begin, int c, int first, int step, bool have, Pick last) {
  Pick best = no_pick();
  for (int t = first; t < c; t += step) {
    const Pick x{ordered_key(a.pair_key[begin + t]), a.pair_polygon[begin + t]};
    if ((!have || pick_before(last, x)) && pick_before(x, best)) best = x;
  }
  return best;
}

__device__ __forceinline__ void write_pick(const SelectArgs& a, int64_t point, int j, Pick x) {
  const int64_t o = point * a.k + j;
  const bool none = x.key == no_pick().key && x.idp == no_pick().idp;
  a.polygon[o] = none ? a.P : (int32_t)(x.idp & kIdMask);
  a.dist2[o] = none ? INFINITY : fabs(key_value(x.key));
  a.inside[o] = none ? 0 : (uint8_t)(x.idp >> 31);
}

__global__ __launch_bounds__(kNbThreads) void near_select_kernel(SelectArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kNbThreads;
  unsigned long long kept = 0, truncated = 0, max_count = 0;
  // whole waves iterate together: the wave route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kNbThreads + (threadIdx.x & ~(kWave - 1)); base < a.N; base += stride) {
    const int64_t i = base + lane;
    int64_t begin = 0;
    int c = 0;
    if (i < a.N) {
      begin = a.pair_offsets[i];
      int64_t end = a.pair_offsets[i + 1];
      a.count[i] = (int32_t)(end - begin);                           // before the cap: <= n_polygons
      if (end > a.capacity) end = a.capacity;                        // nothing is ever read at or beyond it
      c = begin >= 0 && end > begin ? (int)(end - begin) : 0;
      kept += (unsigned long long)(c < a.k ? c : a.k);
      truncated += c > a.k ? 1u : 0u;
      max_count = max_count > (unsigned long long)c ? max_count : (unsigned long long)c;
    }
    const bool wide = c > SEGGER_NEAREST_LANE_MAX;
    if (i < a.N && !wide) {                                          // one lane, its own segment
      Pick last = no_pick();
      for (int j = 0; j < a.k; ++j) {
        last = j < c ? next_pick(a, begin, c, 0, 1, j > 0, last) : no_pick();
        write_pick(a, i, j, last);
      }
    }
    for (unsigned long long m = __ballot(wide); m != 0; m &= m - 1) {                // the whole wave, one point at a time
      const int src = (int)__builtin_ctzll(m);
      const int64_t wb = (int64_t)shfl64((uint64_t)begin, src);
      const int wc = __shfl(c, src, kWave);
      Pick last = no_pick();
      for (int j = 0; j < a.k; ++j) {                                // k <= LANE_MAX < wc: a candidate is always left
        Pick x = next_pick(a, wb, wc, lane, kWave, j > 0, last);
#pragma unroll
        for (int s = 1; s < kWave; s <<= 1) {
          const Pick o{shfl_xor64(x.key, s), (uint32_t)__shfl_xor((int)x.idp, s, kWave)};
          if (pick_before(o, x)) x = o;
        }
        last = x;                                                    // the same in every lane: a minimum of a total order
        if (lane == 0) write_pick(a, base + src, j, x);
      }
    }
  }
  kept = (unsigned long long)wave_sum_i64((int64_t)kept);
  truncated = (unsigned long long)wave_sum_i64((int64_t)truncated);
#pragma unroll
  for (int s = 1; s < kWave; s <<= 1) {
    const unsigned long long o = shfl_xor64(max_count, s);
    max_count = o > max_count ? o : max_count;
  }
  if (lane == 0) {
    if (kept) atomicAdd(&a.counters[kCtrKept], kept);
    if (truncated) atomicAdd(&a.counters[kCtrTruncated], truncated);
    if (max_count) atomicMax(&a.counters[kCtrMaxCount], max_count);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.counters[kCtrPairs] = (unsigned long long)a.pair_offsets[a.N];
}

// ---------------------------------------------------------------- host ---
using NbCall = GridCall;
constexpr const char* kNbNames8 = "ring_offsets, pair_offsets and buffer";
struct NbLayout { GridLayout grid; size_t cursor, total; };          // the join's layout and, behind it, a cursor per point

NbLayout nb_layout(int64_t N, int64_t P, int64_t n_cells) {
  NbLayout l;
  l.grid = grid_layout(N, P, n_cells, false);
  l.cursor = l.grid.total;                                           // a multiple of 256
  l.total = l.cursor + align256((size_t)(N > 0 ? N : 1) * 4);
  return l;
}

// everything the count and the fill reject; *empty = nothing to do (no pointer was looked at)
int nb_check(const char* who, const NbCall& c, bool* empty) {
  *empty = false;
  int rc = grid_check_sizes(who, c.N, c.P, c.nx, c.ny);
  if (rc != SEGGER_OK) return rc;
  rc = grid_check(who, c, empty);
  if (rc != SEGGER_OK || *empty) return rc;
  const size_t need = nb_layout(c.N, c.P, (int64_t)c.nx * c.ny).total;
  SEGGER_REQUIRE((size_t)c.workspace_bytes >= need, "%s: workspace %lld < %zu bytes", who, (long long)c.workspace_bytes, need);
  return SEGGER_OK;
}

WalkArgs walk_args(const NbCall& c, const NbLayout& l) {
  WalkArgs a{};
  a.c = walk_common(c, l.grid);
  a.pair_offsets = const_cast<int64_t*>(c.offsets);
  a.cursor = at<int32_t>(c.workspace, l.cursor);
  return a;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_nearest_boundaries_workspace_bytes(int64_t n_points, int64_t n_polygons, int32_t nx, int32_t ny) {
  const int rc = grid_check_sizes("segger_nearest_boundaries_workspace_bytes", n_points, n_polygons, nx, ny);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)nb_layout(n_points, n_polygons, (int64_t)nx * ny).total;
}

extern "C" int segger_nearest_boundaries_count(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                                               int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate,
                                               double x0, double y0, double cell, int32_t nx, int32_t ny, int64_t* pair_offsets,
                                               void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_nearest_boundaries_count";
  hipStream_t stream = (hipStream_t)stream_;
  const NbCall c = grid_call(points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                             pair_offsets, workspace, workspace_bytes, kNbNames8);
  bool empty = false;
  int rc = nb_check(who, c, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  const NbLayout l = nb_layout(n_points, n_polygons, (int64_t)nx * ny);
  SEGGER_HIP(hipMemsetAsync(pair_offsets, 0, (size_t)(n_points + 1) * sizeof(int64_t), stream));
  rc = grid_front(kNbFront, c, l.grid, nullptr, nullptr, stream);
  if (rc == SEGGER_OK) rc = launch_ring_kernels(kNbRings<false>, c, l.grid, walk_args(c, l), stream);
  return rc != SEGGER_OK ? rc : launch_offsets_scan(pair_offsets, n_points, nullptr, stream);
}

extern "C" int segger_nearest_boundaries_fill(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                                              int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate,
                                              double x0, double y0, double cell, int32_t nx, int32_t ny, const int64_t* pair_offsets,
                                              double* pair_key, int32_t* pair_polygon, int64_t capacity, void* workspace,
                                              int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_nearest_boundaries_fill";
  hipStream_t stream = (hipStream_t)stream_;
  const NbCall c = grid_call(points, n_points, ring_offsets, xy, n_polygons, n_vertices, buffer, predicate, x0, y0, cell, nx, ny,
                             pair_offsets, workspace, workspace_bytes, kNbNames8);
  bool empty = false;
  int rc = nb_check(who, c, &empty);
  if (rc == SEGGER_OK) rc = grid_check_capacity(who, capacity, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  SEGGER_REQUIRE(pair_key && pair_polygon, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(pair_key, 8) && is_aligned(pair_polygon, 4), "%s: pair_key must be 8-byte and pair_polygon 4-byte aligned", who);
  const NbLayout l = nb_layout(n_points, n_polygons, (int64_t)nx * ny);
  WalkArgs a = walk_args(c, l);
  a.pair_key = pair_key;
  a.pair_polygon = reinterpret_cast<uint32_t*>(pair_polygon);
  a.capacity = capacity;
  SEGGER_HIP(hipMemsetAsync(a.cursor, 0, (size_t)n_points * sizeof(int32_t), stream));
  return launch_ring_kernels(kNbRings<true>, c, l.grid, a, stream);
}

extern "C" int segger_nearest_boundaries_select(const int64_t* pair_offsets, const double* pair_key, const int32_t* pair_polygon,
                                                int64_t capacity, int64_t n_points, int64_t n_polygons, int32_t k,
                                                int32_t* polygon_out, double* dist2_out, uint8_t* inside_out, int32_t* count_out,
                                                int64_t* counters, segger_stream_t stream_) {
  const char* who = "segger_nearest_boundaries_select";
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_points >= 0 && n_polygons >= 0, "%s: negative n_points or n_polygons", who);
  SEGGER_REQUIRE(n_points < 0x7fffffffLL && n_polygons < 0x7fffffffLL, "%s: 2^31 - 1 points or polygons, or more", who);
  SEGGER_REQUIRE(k >= 1 && k <= SEGGER_NEAREST_MAX_K, "%s: k %d outside 1 .. SEGGER_NEAREST_MAX_K = %d", who, (int)k, SEGGER_NEAREST_MAX_K);
  SEGGER_REQUIRE(capacity >= 0, "%s: negative capacity", who);
  if (n_points == 0) return SEGGER_OK;
  SEGGER_REQUIRE(pair_offsets && polygon_out && dist2_out && inside_out && count_out && counters, "%s: NULL pointer", who);
  SEGGER_REQUIRE((pair_key && pair_polygon) || capacity == 0, "%s: NULL pair_key or pair_polygon with capacity > 0", who);
  SEGGER_REQUIRE(is_aligned(pair_offsets, 8) && is_aligned(pair_key, 8) && is_aligned(dist2_out, 8) && is_aligned(counters, 8),
                 "%s: pair_offsets, pair_key, dist2_out and counters must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(pair_polygon, 4) && is_aligned(polygon_out, 4) && is_aligned(count_out, 4),
                 "%s: pair_polygon, polygon_out and count_out must be 4-byte aligned", who);
  SelectArgs a{};
  a.pair_offsets = pair_offsets;
  a.pair_key = pair_key;
  a.pair_polygon = reinterpret_cast<const uint32_t*>(pair_polygon);
  a.capacity = capacity;
  a.N = n_points;
  a.P = (int32_t)n_polygons;
  a.k = k;
  a.polygon = polygon_out;
  a.dist2 = dist2_out;
  a.inside = inside_out;
  a.count = count_out;
  a.counters = reinterpret_cast<unsigned long long*>(counters);
  SEGGER_HIP(hipMemsetAsync(counters, 0, SEGGER_NEAREST_COUNTERS * sizeof(int64_t), stream));
  hipLaunchKernelGGL(near_select_kernel, dim3(grid_stride_blocks(n_points, kNbThreads, (int64_t)cu_count_or_default() * 32)),
                     dim3(kNbThreads), 0, stream, a);
  SEGGER_LAUNCH_CHECK("near_select_kernel");
  return SEGGER_OK;
}
