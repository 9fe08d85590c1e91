// segger_simplify_rings_mark / _emit and segger_rings_simple: the two steps the reference's CosMx intake takes right after
// masks_to_contours -- `geometry.simplify(tolerance)` (GEOS's topology-preserving simplifier, src/segger/io/cosmx.py:94-96)
// and the `is_valid` that fix_invalid_geometry asks first (io/utils.py:127-136) -- over the project's ring CSR.
// include/segger_amd.h has the contract: guarded Douglas-Peucker over the closed vertex sequence, `touch` of two segments
// (rings.h defines it, next to the overlap join's segments_meet), what a simple ring is.  UNPINNED against GEOS (never
// run): see the header.
//
// Kernels, one stream, no host synchronisation inside an entry point:
//   sr_bin_kernel     one thread per polygon: checks its ring (rings.h) and its tolerance, passes a ring of fewer than 3
//                     open vertices through, appends every other ring to the list of its tier (append_by_route);
//   sr_mark_kernel    one single-wave workgroup per ring: the ring translated into LDS (stage_long_ring), then the
//                     depth-first walk.  Within a section the lanes stride over the interior and a wave reduction gives the
//                     farthest vertex (lowest index among equals); the guard is a strided loop over the input edges outside
//                     the section and the chords emitted so far, with a ballot for "any touch".  Writes the keep mask (one
//                     byte per input vertex) and the ring's four statistics into the workspace;
//   sr_scan_kernel    one workgroup: the kept counts -> out_offsets (post_common.h's GroupScan), the statistics -> the
//                     counters (integer sums: the same bytes whatever the order);
//   sr_emit_kernel    one wave per ring: the kept vertices' INPUT bytes and their indices, each at its hit_slot
//                     (post_common.h);
//   sr_valid_kernel   one single-wave workgroup per ring: for edge i (uniform) the lanes stride over the edges j > i; the
//                     first lane of the first ballot that is not empty is the lowest j, so the reported pair is the lowest
//                     in (i, j) order whatever the scheduling -- no atomic decides it.
//
// Tiers instead of rings.h's register route.  The walk reads v_i, v_j and the interior at indices only known at run time and
// keeps per-ring state of up to n entries (the kept list and the stack of pending right halves), so a ring of n <= 64 in
// registers would still need that state in LDS and a second body.  What matters is that the contours this step exists for
// have some hundreds of vertices: with the 64 KB ring of rings.h' LDS route two workgroups fit a CU.  So both tiers stage
// the ring in LDS with the same body and differ in capacity only: n <= 256 in 4864 B (LDS never limits the single-wave
// workgroups of a CU), 256 < n <= SEGGER_MORPH_MAX_VERTS in 77824 B (two per CU).
//
// Per-ring state: sk[cap] uint16 holds the kept list from the bottom and the pending section ends from the top.  They never
// meet: the kept vertices have indices <= j once j is appended, the stored pending ends are distinct, > j and < n (the ring's
// own end n is always the bottom of the stack and is a flag, not an entry), so together at most n entries.  A pending
// section starts where the one before it ended, so its end is all the stack stores.  keep[cap] is the byte mask.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel; LDS per workgroup
// 16 cap + 2 cap + cap = 4864 B / 77824 B (mark) and 16 cap = 4096 B / 65536 B (valid).
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kSrThreads = 256;
constexpr int kSrWaves = kSrThreads / kWave;
constexpr int kSrScanThreads = 1024;
constexpr int kSmallCap = SEGGER_SIMPLIFY_SMALL_VERTS;
constexpr int kLargeCap = SEGGER_MORPH_MAX_VERTS;
constexpr int kKindPass = 1, kKindRestored = 2;                      // bits 24 .. of a ring's fourth statistic

// ---------------------------------------------------------------- the predicates of the contract ---
// (touch and same are rings.h's)
__device__ __forceinline__ double dist2(P2 v, P2 a, P2 b) {
  const double ex = b.x - a.x, ey = b.y - a.y;
  const double wx = v.x - a.x, wy = v.y - a.y;
  const double cr = ex * wy - ey * wx;
  const double dot = wx * ex + wy * ey;
  const double len2 = ex * ex + ey * ey;
  if (dot <= 0.0 || len2 == 0.0) return wx * wx + wy * wy;
  if (dot >= len2) {
    const double ux = v.x - b.x, uy = v.y - b.y;
    return ux * ux + uy * uy;
  }
  return cr * cr / len2;
}

// vertex k of a staged ring of n, index n meaning vertex 0
__device__ __forceinline__ P2 vert(const double2* pts, int n, int k) {
  const double2 p = pts[k == n ? 0 : k];
  return P2{p.x, p.y};
}

// ---------------------------------------------------------------- binning ---
struct SrBin {
  const int64_t* off; const double* xy; int64_t P, V;
  const double* tol; int64_t tol_stride;                             // NULL: the validity call, no tolerance
  int small_max;
  int4* stat; uint8_t* mask;                                         // simplify
  uint8_t* ok; int32_t* reason;                                      // validity
  int32_t *words, *list_small, *list_large;
};

__global__ __launch_bounds__(kSrThreads) void sr_bin_kernel(SrBin a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kSrThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kSrThreads + (threadIdx.x & ~(kWave - 1)); base < a.P; base += stride) {
    const int64_t p = base + lane;
    int route = -1;
    if (p < a.P) {
      const RingClass c = classify_ring(a.off, a.xy, p, a.V);
      int bad = c.bad;
      if (a.tol) {
        const double t = a.tol[p * a.tol_stride];
        if (!(t >= 0.0 && t < INFINITY)) bad |= SEGGER_SIMPLIFY_ERR_TOL;
      }
      if (bad) atomicOr(&a.words[kWordFlag], bad);
      const bool few = bad || c.n < 3;
      if (a.tol) {
        if (bad) a.stat[p] = make_int4(0, 0, 0, 0);
        else if (few) {                                              // passed through: its open vertices, as they are
          const int64_t b = a.off[p], e = a.off[p + 1];
          for (int64_t k = b; k < e; ++k) a.mask[k] = (uint8_t)(k - b < c.n);
          a.stat[p] = make_int4((int)c.n, (int)c.n, 0, kKindPass << 24);
        }
      } else if (few) {
        a.ok[p] = 0;
        a.reason[3 * p] = SEGGER_RING_TOO_FEW; a.reason[3 * p + 1] = -1; a.reason[3 * p + 2] = -1;
      }
      if (!few) route = c.n > a.small_max;
    }
    append_by_route(route, p, a.words, a.list_small, a.list_large);
  }
}

// ---------------------------------------------------------------- simplify: mark and count ---
struct SrMark {
  const int64_t* off; const double* xy; const double* tol; int64_t tol_stride; int preserve;
  int4* stat; uint8_t* mask; const int32_t* words;
};

template <int kCap>
__global__ __launch_bounds__(kWave) void sr_mark_kernel(SrMark a, const int32_t* __restrict__ list, int word) {
  __shared__ double2 pts[kCap];
  __shared__ uint16_t sk[kCap];
  __shared__ uint8_t keep[kCap];
  const int lane = threadIdx.x;
  const int count = a.words[word];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int64_t p = list[w];
    const LongRing r = stage_long_ring(a.off, a.xy, p, pts);         // 3 <= n <= kCap: the binning kernel said so
    const int n = r.n;
    const double tol = a.tol[p * a.tol_stride];
    const double tol2 = tol * tol;
    for (int k = lane; k < n; k += kWave) keep[k] = (uint8_t)(k == 0);
    if (lane == 0) sk[0] = 0;
    __syncthreads();
    int i = 0, j = n, t = 0, depth = 0, sections = 0, refused = 0;   // the same in every lane
    bool end_pending = false;
    for (;;) {
      ++sections;
      bool flat = true;                                              // a single input edge is emitted as it is
      int m = i + 1;
      if (j > i + 1) {
        const P2 va = vert(pts, n, i), vb = vert(pts, n, j);
        double best = -1.0;
        int best_k = 0x7fffffff;
        for (int k = i + 1 + lane; k < j; k += kWave) {
          const double d = dist2(vert(pts, n, k), va, vb);
          if (d > best) { best = d; best_k = k; }                    // ascending k: the lowest index of equals stays
        }
#pragma unroll
        for (int s = 1; s < kWave; s <<= 1) {
          const double od = shfl_xor_f64(best, s);
          const int ok = __shfl_xor(best_k, s, kWave);
          if (od > best || (od == best && ok < best_k)) { best = od; best_k = ok; }
        }
        m = __builtin_amdgcn_readfirstlane(best_k);
        best = readlane_f64(best, 0);
        if (m > j) m = i + 1;                                        // nothing compared (NaN coordinates): split, never flatten
        flat = best <= tol2;
        if (flat && a.preserve) {
          const int before = i, after = n - j, total = before + after + t;
          bool any = false;
          for (int base = 0; base < total && !any; base += kWave) {
            const int q = base + lane;
            bool hit = false;
            if (q < total) {
              int s0, s1;
              if (q < before) { s0 = q; s1 = q + 1; }
              else if (q < before + after) { s0 = j + (q - before); s1 = s0 + 1; }
              else { s0 = sk[q - before - after]; s1 = sk[q - before - after + 1]; }
              hit = touch(va, vb, vert(pts, n, s0), vert(pts, n, s1));
            }
            any = __ballot(hit) != 0;
          }
          if (any) { flat = false; ++refused; }
        }
      }
      if (flat) {
        if (j < n) {
          ++t;
          if (lane == 0) { sk[t] = (uint16_t)j; keep[j] = 1; }
        }
        if (depth == 0 && !end_pending) break;
        __syncthreads();
        i = j;
        if (depth > 0) { j = sk[kCap - depth]; --depth; }
        else { j = n; end_pending = false; }
      } else {
        if (j == n) end_pending = true;                              // the ring's end is the bottom of the stack: not stored
        else {
          if (lane == 0) sk[kCap - 1 - depth] = (uint16_t)j;
          ++depth;
        }
        j = m;
        __syncthreads();
      }
    }
    __syncthreads();
    int n_out = t + 1, kind = 0;
    if (n_out < 3) { n_out = n; kind = kKindRestored; }              // a collapsed ring is returned as it went in
    const int64_t b = a.off[p];
    const int entries = (int)(a.off[p + 1] - b);                     // n, or n + 1 with a closing duplicate
    for (int k = lane; k < entries; k += kWave) a.mask[b + k] = (uint8_t)(k < n && (kind == kKindRestored || keep[k]));
    if (lane == 0) a.stat[p] = make_int4(n_out, n, sections, refused | (kind << 24));
  }
}

// stat[p] -> out_offsets (exclusive scan of the kept counts) and the counters; one workgroup
__global__ __launch_bounds__(kSrScanThreads) void sr_scan_kernel(const int4* __restrict__ stat, int64_t P, const int32_t* __restrict__ words,
                                                                 int64_t* __restrict__ out_offsets, int64_t* __restrict__ counters) {
  __shared__ int64_t wave_total[kSrScanThreads / kWave];
  __shared__ int64_t sums[SEGGER_SIMPLIFY_COUNTERS][kSrScanThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  GroupScan<kSrScanThreads, int64_t> scan{wave_total, 0};
  int64_t acc[SEGGER_SIMPLIFY_COUNTERS] = {};
  for (int64_t base = 0; base < P; base += kSrScanThreads) {
    const int64_t i = base + threadIdx.x;
    const int4 s = i < P ? stat[i] : make_int4(0, 0, 0, 0);
    acc[0] += s.y; acc[1] += s.x; acc[2] += s.z; acc[3] += s.w & 0xffffff;
    acc[4] += (s.w >> 24) == kKindPass; acc[5] += (s.w >> 24) == kKindRestored;
    acc[6] = acc[6] > s.x ? acc[6] : (int64_t)s.x;
    const int64_t before = scan.step((int64_t)s.x);
    if (i < P) out_offsets[i + 1] = before + s.x;
  }
  if (threadIdx.x == 0) out_offsets[0] = 0;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    int64_t v = acc[c];
    if (c == 6) {
#pragma unroll
      for (int m = 1; m < kWave; m <<= 1) { const int64_t o = (int64_t)shfl_xor64((uint64_t)v, m); v = v > o ? v : o; }
    } else v = wave_sum_i64(v);
    if (lane == 0) sums[c][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int c = threadIdx.x;
    int64_t v = 0;
    for (int w = 0; w < kSrScanThreads / kWave; ++w) v = c == 6 ? (v > sums[c][w] ? v : sums[c][w]) : v + sums[c][w];
    counters[c] = v;
  }
  if (threadIdx.x == 7) counters[7] = words[kWordFlag];
}

// ---------------------------------------------------------------- simplify: emit ---
__global__ __launch_bounds__(kSrThreads) void sr_emit_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy, int64_t P,
                                                             int64_t V, const uint8_t* __restrict__ mask,
                                                             const int64_t* __restrict__ out_offsets, double* __restrict__ xy_out,
                                                             int64_t* __restrict__ vertex_index, int64_t capacity) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n_waves = (int64_t)gridDim.x * kSrWaves;
  for (int64_t p = (int64_t)blockIdx.x * kSrWaves + (threadIdx.x >> 6); p < P; p += n_waves) {                 // wave-uniform
    const int64_t b = off[p], e = off[p + 1];
    if (b < 0 || e < b || e > V) continue;                           // mark reported it; nothing is read
    const int64_t begin = out_offsets[p];
    int64_t end = out_offsets[p + 1];
    if (end > capacity) end = capacity;                              // nothing is ever written at or beyond either
    int64_t found = 0;
    for (int64_t base = b; base < e; base += kWave) {
      const int64_t k = base + lane;
      hit_slot(k < e && mask[k] != 0, begin, end, found, [&](int64_t slot) {
        reinterpret_cast<double2*>(xy_out)[slot] = reinterpret_cast<const double2*>(xy)[k];
        vertex_index[slot] = k;
      });
    }
  }
}

// ---------------------------------------------------------------- validity ---
template <int kCap>
__global__ __launch_bounds__(kWave) void sr_valid_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                         uint8_t* __restrict__ ok, int32_t* __restrict__ reason,
                                                         const int32_t* __restrict__ words, const int32_t* __restrict__ list, int word) {
  __shared__ double2 pts[kCap];
  const int lane = threadIdx.x;
  const int count = words[word];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int64_t p = list[w];
    const LongRing r = stage_long_ring(off, xy, p, pts);
    const int n = r.n;
    int distinct = 0;                                                // vertices left when consecutive duplicates are dropped
    for (int k = lane; k < n; k += kWave) distinct += !same(vert(pts, n, k), vert(pts, n, k + 1));
    distinct = wave_sum_i32(distinct);
    int code = SEGGER_RING_OK, bi = -1, bj = -1;
    if (distinct < 3) code = SEGGER_RING_TOO_FEW;
    else {
      for (int i = 0; i + 1 < n && code == SEGGER_RING_OK; ++i) {
        const P2 va = vert(pts, n, i), vb = vert(pts, n, i + 1);
        for (int base = i + 1; base < n; base += kWave) {
          const int j = base + lane;
          const bool hit = j < n && touch(va, vb, vert(pts, n, j), vert(pts, n, j + 1));
          const unsigned long long m = __ballot(hit);
          if (m != 0) {                                              // lanes hold ascending j: the first is the lowest
            code = SEGGER_RING_TOUCH; bi = i; bj = base + (int)__builtin_ctzll(m);
            break;
          }
        }
      }
    }
    if (lane == 0) {
      ok[p] = (uint8_t)(code == SEGGER_RING_OK);
      reason[3 * p] = code; reason[3 * p + 1] = bi; reason[3 * p + 2] = bj;
    }
  }
}

// ---------------------------------------------------------------- host ---
struct SrLayout { RingLists rings; size_t stat, mask, total; };

SrLayout sr_layout(int64_t P, int64_t V) {
  SrLayout l;
  Carver c;
  l.rings = take_ring_lists(c, P);
  l.stat = c.take((size_t)P * sizeof(int4));
  l.mask = c.take((size_t)V);
  l.total = c.total();
  return l;
}

int sr_check_sizes(const char* who, int64_t P, int64_t V) {
  SEGGER_REQUIRE(P >= 0 && V >= 0, "%s: negative n_polygons or n_vertices", who);
  SEGGER_REQUIRE(P < 0x7fffffffLL, "%s: 2^31 - 1 polygons or more", who);
  return SEGGER_OK;
}

int sr_launch_bin(const SrBin& a, hipStream_t stream) {
  SEGGER_HIP(hipMemsetAsync(a.words, 0, kRingWordsBytes, stream));
  hipLaunchKernelGGL(sr_bin_kernel, dim3(grid_stride_blocks(a.P, kSrThreads, (int64_t)cu_count_or_default() * 8)), dim3(kSrThreads), 0,
                     stream, a);
  SEGGER_LAUNCH_CHECK("sr_bin_kernel");
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_simplify_rings_workspace_bytes(int64_t n_polygons, int64_t n_vertices) {
  const int rc = sr_check_sizes("segger_simplify_rings_workspace_bytes", n_polygons, n_vertices);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)sr_layout(n_polygons, n_vertices).total;
}

extern "C" int segger_simplify_rings_mark(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                          const double* tolerance, int64_t tolerance_stride, int32_t preserve_topology,
                                          int32_t small_max_verts, int64_t* out_offsets, int64_t* counters, void* workspace,
                                          int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_simplify_rings_mark";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc0 = sr_check_sizes(who, n_polygons, n_vertices);
  if (rc0 != SEGGER_OK) return rc0;
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(tolerance_stride == 0 || tolerance_stride == 1, "%s: tolerance_stride %lld is neither 0 (one value) nor 1 (one per polygon)",
                 who, (long long)tolerance_stride);
  SEGGER_REQUIRE(small_max_verts >= 0 && small_max_verts <= SEGGER_SIMPLIFY_SMALL_VERTS, "%s: small_max_verts %d outside 0 .. %d", who,
                 (int)small_max_verts, SEGGER_SIMPLIFY_SMALL_VERTS);
  if (n_polygons == 0) return SEGGER_OK;
  const SrLayout l = sr_layout(n_polygons, n_vertices);
  const int rc = check_ring_call(who, ring_offsets, xy, n_vertices, workspace, workspace_bytes, l.total,
                                 OtherPointers{tolerance && out_offsets && counters,
                                               is_aligned(tolerance, 8) && is_aligned(out_offsets, 8) && is_aligned(counters, 8), true,
                                               "ring_offsets, tolerance, out_offsets and counters", "xy"});
  if (rc != SEGGER_OK) return rc;
  int32_t* words = at<int32_t>(workspace, l.rings.words);
  int32_t* list_small = at<int32_t>(workspace, l.rings.list_short);
  int32_t* list_large = at<int32_t>(workspace, l.rings.list_long);
  int4* stat = at<int4>(workspace, l.stat);
  uint8_t* mask = at<uint8_t>(workspace, l.mask);
  const int rc2 = sr_launch_bin(SrBin{ring_offsets, xy, n_polygons, n_vertices, tolerance, tolerance_stride, small_max_verts, stat, mask,
                                      nullptr, nullptr, words, list_small, list_large}, stream);
  if (rc2 != SEGGER_OK) return rc2;
  const SrMark a{ring_offsets, xy, tolerance, tolerance_stride, preserve_topology != 0, stat, mask, words};
  const int cus = cu_count_or_default();
  hipLaunchKernelGGL((sr_mark_kernel<kSmallCap>), dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 32)), dim3(kWave), 0, stream, a,
                     (const int32_t*)list_small, kWordShort);
  SEGGER_LAUNCH_CHECK("sr_mark_kernel<small>");
  hipLaunchKernelGGL((sr_mark_kernel<kLargeCap>), dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 2)), dim3(kWave), 0, stream, a,
                     (const int32_t*)list_large, kWordLong);
  SEGGER_LAUNCH_CHECK("sr_mark_kernel<large>");
  hipLaunchKernelGGL(sr_scan_kernel, dim3(1), dim3(kSrScanThreads), 0, stream, (const int4*)stat, n_polygons, (const int32_t*)words,
                     out_offsets, counters);
  SEGGER_LAUNCH_CHECK("sr_scan_kernel");
  return SEGGER_OK;
}

extern "C" int segger_simplify_rings_emit(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                          const int64_t* out_offsets, double* xy_out, int64_t* vertex_index, int64_t capacity,
                                          void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_simplify_rings_emit";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc0 = sr_check_sizes(who, n_polygons, n_vertices);
  if (rc0 != SEGGER_OK) return rc0;
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(capacity >= 0, "%s: negative capacity", who);
  if (n_polygons == 0 || capacity == 0) return SEGGER_OK;
  const SrLayout l = sr_layout(n_polygons, n_vertices);
  const int rc = check_ring_call(who, ring_offsets, xy, n_vertices, workspace, workspace_bytes, l.total,
                                 OtherPointers{out_offsets && xy_out && vertex_index, is_aligned(out_offsets, 8) && is_aligned(vertex_index, 8),
                                               is_aligned(xy_out, 16), "ring_offsets, out_offsets and vertex_index", "xy and xy_out"});
  if (rc != SEGGER_OK) return rc;
  hipLaunchKernelGGL(sr_emit_kernel, dim3(grid_stride_blocks(n_polygons, kSrWaves, (int64_t)cu_count_or_default() * 8)), dim3(kSrThreads), 0,
                     stream, ring_offsets, xy, n_polygons, n_vertices, (const uint8_t*)at<uint8_t>(workspace, l.mask), out_offsets, xy_out,
                     vertex_index, capacity);
  SEGGER_LAUNCH_CHECK("sr_emit_kernel");
  return SEGGER_OK;
}

extern "C" int segger_rings_simple(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices, uint8_t* ok,
                                   int32_t* reason, int32_t small_max_verts, void* workspace, int64_t workspace_bytes,
                                   segger_stream_t stream_) {
  const char* who = "segger_rings_simple";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc0 = sr_check_sizes(who, n_polygons, n_vertices);
  if (rc0 != SEGGER_OK) return rc0;
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(small_max_verts >= 0 && small_max_verts <= SEGGER_SIMPLIFY_SMALL_VERTS, "%s: small_max_verts %d outside 0 .. %d", who,
                 (int)small_max_verts, SEGGER_SIMPLIFY_SMALL_VERTS);
  if (n_polygons == 0) return SEGGER_OK;
  const SrLayout l = sr_layout(n_polygons, 0);
  const int rc = check_ring_call(who, ring_offsets, xy, n_vertices, workspace, workspace_bytes, l.total,
                                 OtherPointers{ok && reason, true, true, "ring_offsets", "xy"});
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(is_aligned(reason, 4), "%s: reason must be 4-byte aligned", who);
  int32_t* words = at<int32_t>(workspace, l.rings.words);
  int32_t* list_small = at<int32_t>(workspace, l.rings.list_short);
  int32_t* list_large = at<int32_t>(workspace, l.rings.list_long);
  const int rc2 = sr_launch_bin(SrBin{ring_offsets, xy, n_polygons, n_vertices, nullptr, 0, small_max_verts, nullptr, nullptr, ok, reason,
                                      words, list_small, list_large}, stream);
  if (rc2 != SEGGER_OK) return rc2;
  const int cus = cu_count_or_default();
  hipLaunchKernelGGL((sr_valid_kernel<kSmallCap>), dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 32)), dim3(kWave), 0, stream,
                     ring_offsets, xy, ok, reason, (const int32_t*)words, (const int32_t*)list_small, kWordShort);
  SEGGER_LAUNCH_CHECK("sr_valid_kernel<small>");
  hipLaunchKernelGGL((sr_valid_kernel<kLargeCap>), dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 2)), dim3(kWave), 0, stream,
                     ring_offsets, xy, ok, reason, (const int32_t*)words, (const int32_t*)list_large, kWordLong);
  SEGGER_LAUNCH_CHECK("sr_valid_kernel<large>");
  return SEGGER_OK;
}
