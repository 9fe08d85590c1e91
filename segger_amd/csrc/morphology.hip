// segger_polygon_props: area, convex hull, minimum-area rectangle and smallest enclosing circle of every ring of a CSR of
// polygons -- the parts of the reference's geometry/morphology.py (get_polygon_props), which goes through
// geopandas / shapely one polygon at a time.  include/segger_amd.h has the contract.
//
// Three kernels on one stream, no host synchronisation; rings.h has the ring layer they share with polygon_join.hip (the
// open vertex count, the two routes and their lists, the loaders):
//   morph_bin_kernel    one thread per polygon: a ring that cannot be computed (bad offsets, above the cap) or is empty
//                       gets a row of NaN, and the first two a bit in the error word; the others go to their route's list.
//   morph_short_kernel  n <= 64: one wave per polygon, ring and hull in registers (no LDS).
//   morph_long_kernel   64 < n <= SEGGER_MORPH_MAX_VERTS: one single-wave workgroup per polygon, the ring in LDS (64 KB)
//                       next to the hull's index list (8 KB), lanes striding over both.
// The order of a list depends on the order of the atomics, the row of a polygon does not: every sum is a per-lane sum in
// ascending vertex order followed by a 6-level butterfly, so the same input gives the same bits from call to call.
//
// Per polygon, in float64 on coordinates translated to the ring's first vertex, with FMA contraction off (a cross
// product of exactly representable coordinates is then exact, and cross(a, b) = -cross(b, a) to the bit):
//   1. shoelace area, centroid sums, vertex sums, bounds (bounds on the untranslated coordinates: exact);
//   2. convex hull by gift wrapping (rings.h: march_step) from the lexicographically lowest vertex: each step is one wave-wide arg-max of
//      "most clockwise as seen from the current vertex", ties broken by the larger distance, then by the lower index; a
//      vertex that coincides with the current one never competes.  Collinear and duplicate vertices therefore never
//      enter the hull and the march returns to its start after h <= n steps (n steps is also a hard cap);
//   3. shoelace over the hull;
//   4. minimum-area rectangle: lane e takes hull edge e (stride 64) and projects all h hull vertices, broadcast by
//      readlane or from LDS, on the edge and its normal; the lowest edge index wins a tie;
//   5. smallest enclosing circle: Welzl's iteration over the hull vertices in hull order, three nested levels (1, 2, 3
//      support points), each level's scan "first vertex in [lo, hi) outside the circle" one ballot per 64 vertices.  The
//      radius^2 of a circle is the largest squared distance from its centre to its support points and a vertex is
//      outside iff d^2 > r^2 (1 + SEGGER_MORPH_CIRCLE_SLACK), so a support point never tests as outside its own circle.
//      There is no shuffle: the order is the hull order, the result is reproducible, and every scan only moves forward,
//      so the worst case is h^3 / 64 ballots -- h <= 25 for the 13- and 25-vertex rings that are the bulk of real input;
//      a long ring whose hull has thousands of vertices (a finely sampled circle) is the slow case.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): morph_bin_kernel 20 VGPR, no LDS, 8 waves per SIMD;
// morph_short_kernel 94 VGPR, no LDS, 5 waves per SIMD; morph_long_kernel 104 VGPR, 73728 B LDS (two single-wave
// workgroups per CU); no scratch in any of them.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kMorphThreads = 256;
constexpr int kMorphWaves = kMorphThreads / kWave;
constexpr int kMorphCols = SEGGER_MORPH_COLS;
constexpr double kSlack = SEGGER_MORPH_CIRCLE_SLACK;

static_assert(SEGGER_MORPH_MAX_VERTS <= 65536, "the hull's index list is uint16");

// ---------------------------------------------------------------- the two hull stores ---
// push(k, i, q): hull vertex k is ring vertex i = q; own / at / uni as the ring stores of rings.h
struct RegHull {
  double x = 0.0, y = 0.0;                                           // hull vertex `lane`
  __device__ __forceinline__ void push(int k, int, P2 q) {
    if ((int)(threadIdx.x & (kWave - 1)) == k) { x = q.x; y = q.y; }
  }
  __device__ __forceinline__ void publish() const {}
  __device__ __forceinline__ P2 own(int) const { return P2{x, y}; }
  __device__ __forceinline__ P2 at(int k) const { return P2{shfl_f64(x, k), shfl_f64(y, k)}; }
  __device__ __forceinline__ P2 uni(int k) const { return P2{readlane_f64(x, k), readlane_f64(y, k)}; }
};
struct LdsHull {
  const double2* pts;
  uint16_t* idx;
  __device__ __forceinline__ void push(int k, int i, P2) {
    if ((threadIdx.x & (kWave - 1)) == 0) idx[k] = (uint16_t)i;
  }
  __device__ __forceinline__ void publish() const { __syncthreads(); }       // a workgroup is one wave here
  __device__ __forceinline__ P2 own(int k) const { const double2 p = pts[idx[k]]; return P2{p.x, p.y}; }
  __device__ __forceinline__ P2 at(int k) const { return own(k); }
  __device__ __forceinline__ P2 uni(int k) const { return own(k); }
};

// ---------------------------------------------------------------- circles ---
struct Circle { double cx, cy, r2; };

__device__ __forceinline__ double dist2(P2 p, double cx, double cy) {
  const double dx = p.x - cx, dy = p.y - cy;
  return dx * dx + dy * dy;
}
__device__ __forceinline__ Circle circle1(P2 a) { return Circle{a.x, a.y, 0.0}; }
__device__ __forceinline__ Circle circle2(P2 a, P2 b) {
  Circle c;
  c.cx = a.x + 0.5 * (b.x - a.x);
  c.cy = a.y + 0.5 * (b.y - a.y);
  c.r2 = fmax(dist2(a, c.cx, c.cy), dist2(b, c.cx, c.cy));
  return c;
}
__device__ __forceinline__ Circle circle3(P2 a, P2 b, P2 c) {
  const double bx = b.x - a.x, by = b.y - a.y, cx = c.x - a.x, cy = c.y - a.y;
  const double d = 2.0 * (bx * cy - by * cx);
  const double b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  if (d == 0.0) {                                                    // collinear: the circle on the longest of the three sides
    const double ex = c.x - b.x, ey = c.y - b.y, e2 = ex * ex + ey * ey;
    if (b2 >= c2 && b2 >= e2) return circle2(a, b);
    return c2 >= e2 ? circle2(a, c) : circle2(b, c);
  }
  Circle o;
  o.cx = a.x + (cy * b2 - by * c2) / d;
  o.cy = a.y + (bx * c2 - cx * b2) / d;
  o.r2 = fmax(dist2(a, o.cx, o.cy), fmax(dist2(b, o.cx, o.cy), dist2(c, o.cx, o.cy)));
  return o;
}

// first hull vertex k in [lo, hi) outside the circle, or -1; lo and hi are the same in every lane
template <class Hull>
__device__ __forceinline__ int first_outside(const Hull& hull, int lo, int hi, const Circle& c) {
  const int lane = threadIdx.x & (kWave - 1);
  const double thr = c.r2 + c.r2 * kSlack;
  for (int base = lo & ~(kWave - 1); base < hi; base += kWave) {
    const int k = base + lane;
    bool out = false;
    if (k >= lo && k < hi) out = dist2(hull.own(k), c.cx, c.cy) > thr;
    const unsigned long long m = __ballot(out);
    if (m) return base + (int)__builtin_ctzll(m);
  }
  return -1;
}

// ---------------------------------------------------------------- one polygon, one wave ---
// n >= 1 vertices (translated to org); xmin .. ymax are this lane's bounds over the untranslated vertices it owns
template <class Ring, class Hull>
__device__ __forceinline__ void polygon_body(const Ring& ring, Hull& hull, int n, P2 org, double xmin, double ymin, double xmax,
                                             double ymax, double* __restrict__ row) {
  const int lane = threadIdx.x & (kWave - 1);
  // 1. shoelace, centroid sums, vertex sums; the start of the march
  double a2 = 0.0, mx = 0.0, my = 0.0, sx = 0.0, sy = 0.0;
  int s_i = -1;
  double s_x = 0.0, s_y = 0.0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    const bool valid = i < n;
    const int ii = valid ? i : 0;
    const P2 p = ring.own(ii);
    const P2 q = ring.at((ii + 1 == n) ? 0 : ii + 1);            // the successor
    if (valid) {
      const double cr = p.x * q.y - q.x * p.y;
      a2 += cr;
      mx += (p.x + q.x) * cr;
      my += (p.y + q.y) * cr;
      sx += p.x;
      sy += p.y;
      if (s_i < 0 || p.x < s_x || (p.x == s_x && p.y < s_y)) { s_i = i; s_x = p.x; s_y = p.y; }
    }
  }
  a2 = wave_sum_f64(a2);
  mx = wave_sum_f64(mx);
  my = wave_sum_f64(my);
  sx = wave_sum_f64(sx);
  sy = wave_sum_f64(sy);
  xmin = wave_min_f64(xmin);
  ymin = wave_min_f64(ymin);
  xmax = wave_max_f64(xmax);
  ymax = wave_max_f64(ymax);
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {                              // lowest (x, y, index)
    const int oi = __shfl_xor(s_i, m, kWave);
    const double ox = shfl_xor_f64(s_x, m), oy = shfl_xor_f64(s_y, m);
    const bool take = oi >= 0 && (s_i < 0 || ox < s_x || (ox == s_x && (oy < s_y || (oy == s_y && oi < s_i))));
    if (take) { s_i = oi; s_x = ox; s_y = oy; }
  }
  const int start = __builtin_amdgcn_readfirstlane(s_i);

  // 2. the march
  int h = 0;
  int cur = start;
  for (int step = 0; step < n; ++step) {
    const P2 p = ring.uni(cur);
    hull.push(h, cur, p);
    ++h;
    const Cand best = march_step(ring, n, p);                        // rings.h: the tie rules
    if (best.i < 0 || best.i == start) break;
    cur = best.i;
  }
  hull.publish();

  // 3. hull area, 4. minimum-area rectangle
  double h2 = 0.0, rect = INFINITY;
  int rect_k = 0x7fffffff;
  for (int base = 0; base < h; base += kWave) {
    const int k = base + lane;
    const bool valid = k < h;
    const int kk = valid ? k : 0;
    const P2 a = hull.own(kk);
    const P2 b = hull.at((kk + 1 == h) ? 0 : kk + 1);
    const double ex = b.x - a.x, ey = b.y - a.y;
    double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    for (int j = 0; j < h; ++j) {
      const P2 q = hull.uni(j);
      const double dx = q.x - a.x, dy = q.y - a.y;
      const double u = dx * ex + dy * ey, v = dy * ex - dx * ey;
      umin = fmin(umin, u); umax = fmax(umax, u);
      vmin = fmin(vmin, v); vmax = fmax(vmax, v);
    }
    if (valid) {
      h2 += a.x * b.y - b.x * a.y;
      const double area = (umax - umin) * (vmax - vmin) / (ex * ex + ey * ey);
      if (area < rect) { rect = area; rect_k = k; }
    }
  }
  h2 = wave_sum_f64(h2);
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double oa = shfl_xor_f64(rect, m);
    const int ok = __shfl_xor(rect_k, m, kWave);
    if (oa < rect || (oa == rect && ok < rect_k)) { rect = oa; rect_k = ok; }
  }
  if (h < 2) rect = 0.0;

  // 5. smallest enclosing circle of the hull vertices
  Circle c = circle1(hull.uni(0));
  for (int i = 1; i < h;) {
    i = first_outside(hull, i, h, c);
    if (i < 0) break;
    const P2 pi = hull.uni(i);
    c = circle1(pi);
    for (int j = 0; j < i;) {
      j = first_outside(hull, j, i, c);
      if (j < 0) break;
      const P2 pj = hull.uni(j);
      c = circle2(pi, pj);
      for (int k = 0; k < j;) {
        k = first_outside(hull, k, j, c);
        if (k < 0) break;
        c = circle3(pi, pj, hull.uni(k));
        ++k;
      }
      ++j;
    }
    ++i;
  }

  if (lane == 0) {
    const double nd = (double)n;
    row[0] = 0.5 * fabs(a2);
    row[1] = 0.5 * fabs(h2);
    row[2] = rect;
    row[3] = (xmax - xmin) * (ymax - ymin);
    row[4] = sqrt(c.r2);
    row[5] = org.x + (a2 != 0.0 ? mx / (3.0 * a2) : sx / nd);
    row[6] = org.y + (a2 != 0.0 ? my / (3.0 * a2) : sy / nd);
    row[7] = xmin;
    row[8] = ymin;
    row[9] = xmax;
    row[10] = ymax;
    row[11] = (double)h;
  }
}

__device__ __forceinline__ void nan_row(double* __restrict__ row) {
#pragma unroll
  for (int c = 0; c < kMorphCols; ++c) row[c] = NAN;
}

__global__ __launch_bounds__(kMorphThreads) void morph_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                                  int64_t P, int64_t V, double* __restrict__ props,
                                                                  int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                                  int32_t* __restrict__ list_long) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kMorphThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kMorphThreads + (threadIdx.x & ~(kWave - 1)); base < P; base += stride) {
    const int64_t p = base + lane;
    int route = -1;                                                  // -1: nothing to compute
    if (p < P) {
      const RingClass c = classify_ring(off, xy, p, V);
      if (c.bad) atomicOr(&words[kWordFlag], c.bad);
      if (c.bad || c.n == 0) nan_row(props + p * kMorphCols);
      else route = ring_route(c.n);
    }
    append_by_route(route, p, words, list_short, list_long);
  }
}

__global__ __launch_bounds__(kMorphThreads) void morph_short_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                                    double* __restrict__ props, const int32_t* __restrict__ words,
                                                                    const int32_t* __restrict__ list) {
  const int count = words[kWordShort];
  const int n_waves = (int)gridDim.x * kMorphWaves;
  for (int w = (int)blockIdx.x * kMorphWaves + (int)(threadIdx.x >> 6); w < count; w += n_waves) {             // wave-uniform
    const int64_t p = list[w];
    const ShortRing s = load_short_ring(off, xy, p);
    RegHull hull;
    polygon_body(s.ring, hull, s.n, s.first, s.mine.x, s.mine.y, s.mine.x, s.mine.y, props + p * kMorphCols);
  }
}

__global__ __launch_bounds__(kWave) void morph_long_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                           double* __restrict__ props, const int32_t* __restrict__ words,
                                                           const int32_t* __restrict__ list) {
  __shared__ double2 pts[SEGGER_MORPH_MAX_VERTS];
  __shared__ uint16_t hidx[SEGGER_MORPH_MAX_VERTS];
  const int count = words[kWordLong];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int64_t p = list[w];
    const LongRing r = stage_long_ring(off, xy, p, pts);
    LdsRing ring{pts};
    LdsHull hull{pts, hidx};
    polygon_body(ring, hull, r.n, r.first, r.xmin, r.ymin, r.xmax, r.ymax, props + p * kMorphCols);
  }
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_morphology_workspace_bytes(int64_t n_polygons) {
  if (n_polygons < 0 || n_polygons >= 0x7fffffffLL) {
    set_error("segger_morphology_workspace_bytes: n_polygons = %lld outside 0 .. 2^31 - 2", (long long)n_polygons);
    return SEGGER_EINVAL;
  }
  Carver c;                                                          // the workspace is the ring lists and nothing else
  take_ring_lists(c, n_polygons);
  return (int64_t)c.total();
}

extern "C" int segger_polygon_props(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                    double* props, void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_polygon_props";
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_polygons >= 0 && n_vertices >= 0, "%s: negative n_polygons or n_vertices", who);
  SEGGER_REQUIRE(n_polygons < 0x7fffffffLL, "%s: 2^31 - 1 polygons or more", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  if (n_polygons == 0) return SEGGER_OK;
  Carver c;
  const RingLists l = take_ring_lists(c, n_polygons);
  const int rc = check_ring_call(who, ring_offsets, xy, n_vertices, workspace, workspace_bytes, c.total(),
                                 OtherPointers{props != nullptr, is_aligned(props, 8), true, "ring_offsets and props", "xy"});
  if (rc != SEGGER_OK) return rc;
  int32_t* words = at<int32_t>(workspace, l.words);
  int32_t* list_short = at<int32_t>(workspace, l.list_short);
  int32_t* list_long = at<int32_t>(workspace, l.list_long);
  SEGGER_HIP(hipMemsetAsync(words, 0, kRingWordsBytes, stream));
  const int cus = cu_count_or_default();
  hipLaunchKernelGGL(morph_bin_kernel, dim3(grid_stride_blocks(n_polygons, kMorphThreads, (int64_t)cus * 8)), dim3(kMorphThreads), 0,
                     stream, ring_offsets, xy, n_polygons, n_vertices, props, words, list_short, list_long);
  SEGGER_LAUNCH_CHECK("morph_bin_kernel");
  hipLaunchKernelGGL(morph_short_kernel, dim3(grid_stride_blocks(n_polygons, kMorphWaves, (int64_t)cus * 8)), dim3(kMorphThreads), 0,
                     stream, ring_offsets, xy, props, words, list_short);
  SEGGER_LAUNCH_CHECK("morph_short_kernel");
  hipLaunchKernelGGL(morph_long_kernel, dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 2)), dim3(kWave), 0, stream,
                     ring_offsets, xy, props, words, list_long);
  SEGGER_LAUNCH_CHECK("morph_long_kernel");
  return SEGGER_OK;
}
