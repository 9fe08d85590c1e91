// segger_rings_resort: the repair that the reference's fix_invalid_geometry tries first on an invalid polygon,
// resort_coordinates (src/segger/io/utils.py:83-102) -- the vertices of the closed coordinate sequence re-sorted by angle
// around their mean -- over the project's ring CSR, for the rings a mask selects.  include/segger_amd.h has the contract:
// the centre and the order of its sum, the rounded differences, the exact angular order and its ties.  The buffer(0)
// fallback of the reference is NOT BUILT (GEOS was never run; see the header).
//
// Kernels, one stream, no host synchronisation inside the entry point:
//   rr_copy_kernel    one thread per vertex: xy -> xy_out as it is, vertex_index = the row itself.  What the sort kernel
//                     does not overwrite afterwards (unselected rings, rings of fewer than 3 vertices, rows between rings)
//                     is thereby passed through bit for bit;
//   rr_bin_kernel     one thread per polygon: checks its ring (rings.h' classify_ring), appends a selected ring of at least 3
//                     open vertices to the list of its tier (append_by_route);
//   rr_sort_kernel    one single-wave workgroup per listed ring.  The lanes stride over the ring for the centre's sum (lane l
//                     adds vertices l, l + 64, ... in ascending order, then rings.h' butterfly over the lanes: one fixed
//                     order, the same bits in every lane), write the rounded differences d_k into LDS and sort the vertex
//                     INDICES (uint16, LDS) with a bitonic network over the padded size; an index >= n sorts last.  The
//                     comparator reads d through the index: half-plane class, then the sign of d_a x d_b from two FMA
//                     two-products and an exact expansion sum of the four terms, then |d| by components, then the index.
//                     A compare-exchange network only ever swaps two entries, so whatever the coordinates hold (NaN
//                     included) the result is a permutation and every write stays inside the ring.  The lanes then write
//                     the INPUT's bytes and their rows in sorted order.
//
// Why the indices are sorted and not the records: a swap then moves 2 bytes instead of 18, and the 16-byte LDS store is
// the expensive instruction (13 cycles a wave against 4 for the load).  The price is that the comparator's two loads of d
// are gathers -- 16 lanes of a ds_read_b128 group draw from the 16 slots of a bank row at random, some 3-way on average.
// NOT MEASURED which of the two wins; no counter run was made.
//
// Tiers, as simplify.hip: both stage the ring in LDS with the same body and differ in capacity only, n <= 256 in 4608 B and
// 256 < n <= SEGGER_MORPH_MAX_VERTS in 73728 B (two per CU).  No scratch, no float atomics.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "wave_sort.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kRrThreads = 256;
constexpr int kSmallCap = SEGGER_SIMPLIFY_SMALL_VERTS;
constexpr int kLargeCap = SEGGER_MORPH_MAX_VERTS;
static_assert((kSmallCap & (kSmallCap - 1)) == 0 && (kLargeCap & (kLargeCap - 1)) == 0, "the padded size of a ring fits its tier");
static_assert(kLargeCap <= 65536, "indices are uint16");

// ---------------------------------------------------------------- the exact comparator ---
// s + e == a + b exactly (Knuth); no contraction in this unit
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bv = s - a;
  e = (a - (s - bv)) + (b - bv);
}

// the sign of a.x b.y - a.y b.x, without rounding: each product is its rounded value plus the FMA's exact error term, and the
// four terms are summed into a non-overlapping expansion one at a time (Shewchuk's GROW-EXPANSION), whose highest non-zero
// component has the sign of the sum
__device__ __forceinline__ int cross_sign(double2 a, double2 b) {
  const double p = a.x * b.y, pe = __builtin_fma(a.x, b.y, -p);
  const double q = a.y * b.x, qe = __builtin_fma(a.y, b.x, -q);
  double h0, h1, h2, h3, t;
  two_sum(p, -q, h1, h0);                                            // (h0, h1)
  two_sum(pe, h0, t, h0);                                            // + pe: (h0, h1, h2)
  two_sum(t, h1, h2, h1);
  two_sum(-qe, h0, t, h0);                                           // - qe: (h0, h1, h2, h3)
  two_sum(t, h1, t, h1);
  two_sum(t, h2, h3, h2);
  const double top = h3 != 0.0 ? h3 : h2 != 0.0 ? h2 : h1 != 0.0 ? h1 : h0;
  return (int)(top > 0.0) - (int)(top < 0.0);
}

// where the angle of d lies: 0 in (-pi, 0), 1 at 0 (d = (0, 0) too), 2 in (0, pi), 3 at pi
__device__ __forceinline__ int half_class(double2 d) { return d.y < 0.0 ? 0 : d.y > 0.0 ? 2 : (d.x < 0.0 ? 3 : 1); }

// does vertex a come before vertex b?  A strict total order over 0 .. padded size; d is read for indices below n only
__device__ __forceinline__ bool before(const double2* d, int n, int a, int b) {
  if (a >= n || b >= n) return a < b;
  const double2 u = d[a], v = d[b];
  const int cu = half_class(u), cv = half_class(v);
  if (cu != cv) return cu < cv;
  const int s = cross_sign(u, v);                                    // within a class the angles differ by less than pi
  if (s != 0) return s > 0;
  // one exact angle: v = t u with t > 0, so |u|^2 < |v|^2 iff |u.x| < |v.x|, or |u.y| < |v.y| where both x are zero
  const double ux = fabs(u.x), vx = fabs(v.x);
  if (ux != vx) return ux < vx;
  const double uy = fabs(u.y), vy = fabs(v.y);
  if (uy != vy) return uy < vy;
  return a < b;
}

// ---------------------------------------------------------------- pass through, binning ---
__global__ __launch_bounds__(kRrThreads) void rr_copy_kernel(const double* __restrict__ xy, int64_t V, double* __restrict__ xy_out,
                                                             int64_t* __restrict__ vertex_index) {
  const int64_t stride = (int64_t)gridDim.x * kRrThreads;
  for (int64_t i = (int64_t)blockIdx.x * kRrThreads + threadIdx.x; i < V; i += stride) {
    reinterpret_cast<double2*>(xy_out)[i] = reinterpret_cast<const double2*>(xy)[i];
    vertex_index[i] = i;
  }
}

__global__ __launch_bounds__(kRrThreads) void rr_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy, int64_t P, int64_t V,
                                                            const uint8_t* __restrict__ select, int small_max, int32_t* __restrict__ words,
                                                            int32_t* __restrict__ list_small, int32_t* __restrict__ list_large) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kRrThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kRrThreads + (threadIdx.x & ~(kWave - 1)); base < P; base += stride) {
    const int64_t p = base + lane;
    int route = -1;
    if (p < P) {
      const RingClass c = classify_ring(off, xy, p, V);               // every ring is checked, selected or not
      if (c.bad) atomicOr(&words[kWordFlag], c.bad);
      else if (c.n >= 3 && (!select || select[p] != 0)) route = c.n > small_max;
    }
    append_by_route(route, p, words, list_small, list_large);
  }
}

// ---------------------------------------------------------------- the sort ---
struct RrSort { const int64_t* off; const double* xy; double* xy_out; int64_t* vertex_index; const int32_t* words; };

template <int kCap>
__global__ __launch_bounds__(kWave) void rr_sort_kernel(RrSort a, const int32_t* __restrict__ list, int word) {
  __shared__ double2 d[kCap];
  __shared__ uint16_t idx[kCap];
  const int lane = threadIdx.x;
  const int count = a.words[word];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int64_t p = list[w];
    const int64_t b = a.off[p], e = a.off[p + 1];
    const int n = __builtin_amdgcn_readfirstlane((int)open_count(a.xy, b, e));     // 3 <= n <= kCap: the binning kernel said so
    const bool closed = e - b > n;                                   // a closing duplicate follows the n open vertices
    const double2* src = reinterpret_cast<const double2*>(a.xy) + b;
    double sx = 0.0, sy = 0.0;
    for (int k = lane; k < n; k += kWave) {
      const double2 v = src[k];
      sx += v.x; sy += v.y;
    }
    sx = wave_sum_f64(sx); sy = wave_sum_f64(sy);
    const double2 first = src[0];
    const double cx = (sx + first.x) / (double)(n + 1), cy = (sy + first.y) / (double)(n + 1);
    int padded = 4;
    while (padded < n) padded <<= 1;
    __syncthreads();                                                 // the previous ring's readers are done
    for (int k = lane; k < n; k += kWave) {
      const double2 v = src[k];
      d[k] = double2{v.x - cx, v.y - cy};
    }
    for (int k = lane; k < padded; k += kWave) idx[k] = (uint16_t)k;
    __syncthreads();
    wave_bitonic_sort(idx, padded, [&](int x, int y) { return before(d, n, x, y); }, BlockSync{});      // wave_sort.h
    // A closing duplicate stays in the ring, next to its twin: it has vertex 0's d and the index n, so it follows vertex 0
    // and every vertex with the same d (they sort by index, all below n).
    int dup_at = n;
    if (closed) {
      const double2 d0 = d[0];
      int rank0 = 0, ties = 0;
      for (int r = lane; r < n; r += kWave) {
        if (idx[r] == 0) rank0 = r;
        const double2 u = d[r];
        ties += (int)(u.x == d0.x && u.y == d0.y);
      }
      dup_at = wave_sum_i32(rank0) + wave_sum_i32(ties);
      if (dup_at > n) dup_at = n;                                    // coordinates that are not numbers: stay inside the ring
    }
    for (int r = lane; r < n; r += kWave) {
      const int k = idx[r];                                          // < n: the n real indices sort before the padding
      const int64_t slot = b + r + (int)(r >= dup_at);
      reinterpret_cast<double2*>(a.xy_out)[slot] = src[k];
      a.vertex_index[slot] = b + k;
    }
    if (closed && lane == 0) {
      reinterpret_cast<double2*>(a.xy_out)[b + dup_at] = src[n];
      a.vertex_index[b + dup_at] = b + n;
    }
  }
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int segger_rings_resort(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                   const uint8_t* select, double* xy_out, int64_t* vertex_index, int32_t small_max_verts,
                                   void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_rings_resort";
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_polygons >= 0 && n_vertices >= 0, "%s: negative n_polygons or n_vertices", who);
  SEGGER_REQUIRE(n_polygons < 0x7fffffffLL, "%s: 2^31 - 1 polygons or more", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(small_max_verts >= 0 && small_max_verts <= SEGGER_SIMPLIFY_SMALL_VERTS, "%s: small_max_verts %d outside 0 .. %d", who,
                 (int)small_max_verts, SEGGER_SIMPLIFY_SMALL_VERTS);
  if (n_polygons == 0) return SEGGER_OK;
  Carver carve;
  const RingLists l = take_ring_lists(carve, n_polygons);            // the head of segger_simplify_rings_workspace_bytes' layout
  const int rc = check_ring_call(who, ring_offsets, xy, n_vertices, workspace, workspace_bytes, carve.total(),
                                 OtherPointers{(xy_out && vertex_index) || n_vertices == 0, is_aligned(vertex_index, 8), is_aligned(xy_out, 16),
                                               "ring_offsets and vertex_index", "xy and xy_out"});
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(xy_out != xy || n_vertices == 0, "%s: xy_out must not be xy", who);
  int32_t* words = at<int32_t>(workspace, l.words);
  int32_t* list_small = at<int32_t>(workspace, l.list_short);
  int32_t* list_large = at<int32_t>(workspace, l.list_long);
  const int cus = cu_count_or_default();
  SEGGER_HIP(hipMemsetAsync(words, 0, kRingWordsBytes, stream));
  if (n_vertices > 0) {
    hipLaunchKernelGGL(rr_copy_kernel, dim3(grid_stride_blocks(n_vertices, kRrThreads, (int64_t)cus * 8)), dim3(kRrThreads), 0, stream, xy,
                       n_vertices, xy_out, vertex_index);
    SEGGER_LAUNCH_CHECK("rr_copy_kernel");
  }
  hipLaunchKernelGGL(rr_bin_kernel, dim3(grid_stride_blocks(n_polygons, kRrThreads, (int64_t)cus * 8)), dim3(kRrThreads), 0, stream,
                     ring_offsets, xy, n_polygons, n_vertices, select, (int)small_max_verts, words, list_small, list_large);
  SEGGER_LAUNCH_CHECK("rr_bin_kernel");
  const RrSort a{ring_offsets, xy, xy_out, vertex_index, words};
  hipLaunchKernelGGL((rr_sort_kernel<kSmallCap>), dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 32)), dim3(kWave), 0, stream, a,
                     (const int32_t*)list_small, kWordShort);
  SEGGER_LAUNCH_CHECK("rr_sort_kernel<small>");
  hipLaunchKernelGGL((rr_sort_kernel<kLargeCap>), dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 2)), dim3(kWave), 0, stream, a,
                     (const int32_t*)list_large, kWordLong);
  SEGGER_LAUNCH_CHECK("rr_sort_kernel<large>");
  return SEGGER_OK;
}
