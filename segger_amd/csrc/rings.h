// The ring layer shared by the units that read a CSR of float64 rings (morphology.hip, polygon_join.hip; included after
// post_common.h).  Polygon p is xy[off[p] .. off[p + 1]), either orientation; a closing duplicate of its first vertex is
// dropped, bit for bit.  A ring of n <= 64 open vertices takes the register route (one wave, vertex `lane` in lane `lane`),
// one of 64 < n <= SEGGER_MORPH_MAX_VERTS the LDS route (one single-wave workgroup, 64 KB); both hold the ring translated to
// its first vertex.  A binning kernel classifies every polygon and appends it to the list of its route; the polygon kernels
// read the list lengths from the workspace words and load what the binning kernel counted.  One definition each: the units
// agree on "entries", "open vertices" and "route" because they run the same code, and a fix is made here and nowhere else.
// The gift-wrapping march of morphology.hip is here too, because boundaries.hip runs it over a cell's transcripts (that unit
// reads no ring CSR -- it writes one -- and uses the stores, append_by_route and the march).  So is the plane geometry that
// two units share: the uniform double grid with its monotone cell_of (polygon_join.hip, polygon_overlap.hip) and the segment
// predicates orient, same, in_box, segments_meet and touch (polygon_overlap.hip, simplify.hip).
//
// Floating point: this header sets `#pragma clang fp contract(off)` itself, to the end of the including unit.  The loaders
// only subtract, but wave_sum_f64's additions are inlined next to the callers' products, which must not fuse with them.
#pragma once
#include <math.h>

#include "post_common.h"

#pragma clang fp contract(off)

namespace segger {

static_assert(SEGGER_MORPH_ERR_OFFSETS == SEGGER_PJOIN_ERR_OFFSETS, "classify_ring returns bits that both units OR into their word");
static_assert(SEGGER_MORPH_ERR_CAP == SEGGER_PJOIN_ERR_CAP, "classify_ring returns bits that both units OR into their word");
static_assert(SEGGER_MORPH_MAX_VERTS % kWave == 0, "lanes stride over whole chunks");

constexpr int kWordFlag = 0, kWordShort = 1, kWordLong = 2;          // int32 words at the start of the workspace
constexpr size_t kRingWordsBytes = 256;                              // the words' region, zeroed before the binning kernel

struct P2 { double x, y; };

// ---------------------------------------------------------------- float64 across the wave ---
__device__ __forceinline__ double shfl_f64(double v, int src) {
  return __longlong_as_double((long long)shfl64((uint64_t)__double_as_longlong(v), src));
}
__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
  return __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(v), mask));
}
// lane is the same in every lane of the wave
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// the same bits in every lane: a + b is commutative, so both partners of a level compute the same sum
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += shfl_xor_f64(v, m);
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v = fmin(v, shfl_xor_f64(v, m));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v = fmax(v, shfl_xor_f64(v, m));
  return v;
}

// ---------------------------------------------------------------- the uniform grid of the joins ---
// nx x ny square cells from (x0, y0), inv_cell = 1 / side.  (knn.hip's float grid is another struct under another contract.)
struct UniformGrid { double x0, y0, inv_cell; int nx, ny; };

// The cell of a coordinate, clamped into 0 .. n - 1 (NaN -> 0).  MONOTONE in v: that is what polygon_join.hip's walk (a
// point inside the grown bounds is in a walked cell) and polygon_overlap.hip's pair rule (the cell of the lower-left corner
// of two boxes' intersection is the maximum of their first cells) rely on, whatever the grid.
__device__ __forceinline__ int cell_of(double v, double origin, double inv_cell, int n) {
  const double c = floor((v - origin) * inv_cell);
  return (int)fmin(fmax(c, 0.0), (double)(n - 1));
}

// ---------------------------------------------------------------- segment predicates ---
// One expression each, contraction off: exact when the coordinate differences and their products are representable.
__device__ __forceinline__ int orient(P2 a, P2 b, P2 c) {
  const double d = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
  return (int)(d > 0.0) - (int)(d < 0.0);
}
__device__ __forceinline__ bool same(P2 a, P2 b) { return a.x == b.x && a.y == b.y; }
// p is collinear with (a, b) already: is it on the closed segment?
__device__ __forceinline__ bool in_box(P2 p, P2 a, P2 b) {
  return fmin(a.x, b.x) <= p.x && p.x <= fmax(a.x, b.x) && fmin(a.y, b.y) <= p.y && p.y <= fmax(a.y, b.y);
}
// p lies on (a, b) and is neither a nor b
__device__ __forceinline__ bool inside_of(int o, P2 p, P2 a, P2 b) { return o == 0 && in_box(p, a, b) && !same(p, a) && !same(p, b); }

// Two predicates over the closed segments (a, b) and (c, d); both hold at a proper crossing.  They differ at endpoints:
// segments_meet holds whenever the segments share any point, an endpoint included (the overlap join's "intersects");
// touch exempts a shared endpoint -- consecutive edges of a ring meet at one and are not a defect -- and holds only when
// an endpoint of one lies strictly inside the other, or when both are the same segment, longer than a point (the
// simplifier's guard and the ring validity of include/segger_amd.h).
__device__ __forceinline__ bool segments_meet(P2 a, P2 b, P2 c, P2 d) {
  const int o1 = orient(a, b, c), o2 = orient(a, b, d), o3 = orient(c, d, a), o4 = orient(c, d, b);
  if (o1 * o2 < 0 && o3 * o4 < 0) return true;
  return (o1 == 0 && in_box(c, a, b)) || (o2 == 0 && in_box(d, a, b)) || (o3 == 0 && in_box(a, c, d)) || (o4 == 0 && in_box(b, c, d));
}
__device__ __forceinline__ bool touch(P2 a, P2 b, P2 c, P2 d) {
  const int o1 = orient(a, b, c), o2 = orient(a, b, d), o3 = orient(c, d, a), o4 = orient(c, d, b);
  if (o1 * o2 < 0 && o3 * o4 < 0) return true;                       // a proper crossing
  if (inside_of(o1, c, a, b) || inside_of(o2, d, a, b) || inside_of(o3, a, c, d) || inside_of(o4, b, c, d)) return true;
  return !same(a, b) && ((same(a, c) && same(b, d)) || (same(a, d) && same(b, c)));      // the same segment, longer than a point
}

// ---------------------------------------------------------------- the two ring stores ---
// own(i): vertex i from the lane that owns it (i % 64 == lane), callable under any EXEC; at(i): any lane reads any vertex,
// every lane of the wave active; uni(i): i is the same in every lane.
struct RegRing {
  double x, y;                                                       // vertex `lane`, translated
  __device__ __forceinline__ P2 own(int) const { return P2{x, y}; }
  __device__ __forceinline__ P2 at(int i) const { return P2{shfl_f64(x, i), shfl_f64(y, i)}; }
  __device__ __forceinline__ P2 uni(int i) const { return P2{readlane_f64(x, i), readlane_f64(y, i)}; }
};
struct LdsRing {
  const double2* pts;
  __device__ __forceinline__ P2 own(int i) const { const double2 p = pts[i]; return P2{p.x, p.y}; }
  __device__ __forceinline__ P2 at(int i) const { return own(i); }
  __device__ __forceinline__ P2 uni(int i) const { return own(i); }
};

// ---------------------------------------------------------------- binning: classify, append ---
// vertices of ring [b, e) without a closing duplicate (e - b >= 0)
__device__ __forceinline__ int64_t open_count(const double* __restrict__ xy, int64_t b, int64_t e) {
  const int64_t n = e - b;
  if (n < 2) return n;
  const unsigned long long* u = reinterpret_cast<const unsigned long long*>(xy);
  return (u[2 * b] == u[2 * (e - 1)] && u[2 * b + 1] == u[2 * (e - 1) + 1]) ? n - 1 : n;
}

// polygon p < P of a CSR over V vertices: its open vertex count, and SEGGER_MORPH_ERR_OFFSETS or _CAP if it cannot be
// computed (n means nothing then; with bad offsets no vertex was read)
struct RingClass { int64_t n; int bad; };
__device__ __forceinline__ RingClass classify_ring(const int64_t* __restrict__ off, const double* __restrict__ xy, int64_t p, int64_t V) {
  const int64_t b = off[p], e = off[p + 1];
  if (b < 0 || e < b || e > V) return RingClass{0, SEGGER_MORPH_ERR_OFFSETS};
  const int64_t n = open_count(xy, b, e);
  return RingClass{n, n > SEGGER_MORPH_MAX_VERTS ? SEGGER_MORPH_ERR_CAP : 0};
}

// the route of a ring of 1 <= n <= SEGGER_MORPH_MAX_VERTS open vertices: 0 short (registers), 1 long (LDS)
__device__ __forceinline__ int ring_route(int64_t n) { return n > kWave; }

// Appends p to the list of its route (0, 1; anything else: to none): one integer atomic per wave and route.  Whole waves
// call this together: the ballots need every lane of the wave here, so the caller's loop iterates by waves, not by threads.
__device__ __forceinline__ void append_by_route(int route, int64_t p, int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                int32_t* __restrict__ list_long) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long m = __ballot(route == r);
    if (m == 0) continue;
    int pos = 0;
    if (lane == (int)__builtin_ctzll(m)) pos = atomicAdd(&words[r == 0 ? kWordShort : kWordLong], (int)__popcll(m));
    pos = __shfl(pos, (int)__builtin_ctzll(m), kWave);
    if (route == r) (r == 0 ? list_short : list_long)[pos + (int)__popcll(m & ((1ull << lane) - 1))] = (int32_t)p;
  }
}

// ---------------------------------------------------------------- the polygon kernels: load a listed ring ---
// Register route, one wave, p the same in every lane: vertex `lane` (the first vertex in the lanes beyond n), translated
// in `ring` and as given in `mine`.  n is what the binning kernel counted, 1 .. 64; readfirstlane tells the compiler what
// is true already, that it is the same in every lane, so the loops over it become scalar.
struct ShortRing { RegRing ring; int n; P2 first, mine; };
__device__ __forceinline__ ShortRing load_short_ring(const int64_t* __restrict__ off, const double* __restrict__ xy, int64_t p) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = off[p];
  const int n = __builtin_amdgcn_readfirstlane((int)open_count(xy, b, off[p + 1]));
  const double2 first = reinterpret_cast<const double2*>(xy)[b];
  const double2 mine = lane < n ? reinterpret_cast<const double2*>(xy)[b + lane] : first;
  return ShortRing{RegRing{mine.x - first.x, mine.y - first.y}, n, P2{first.x, first.y}, P2{mine.x, mine.y}};
}

// LDS route, a workgroup of one wave: the translated ring into pts[SEGGER_MORPH_MAX_VERTS], between two barriers (the
// previous ring's readers are done; this ring is visible).  n is 65 .. SEGGER_MORPH_MAX_VERTS; xmin .. ymax are this lane's
// bounds over the vertices it copied, as given.
struct LongRing { int n; P2 first; double xmin, ymin, xmax, ymax; };
__device__ __forceinline__ LongRing stage_long_ring(const int64_t* __restrict__ off, const double* __restrict__ xy, int64_t p,
                                                    double2* __restrict__ pts) {
  const int64_t b = off[p];
  const int n = __builtin_amdgcn_readfirstlane((int)open_count(xy, b, off[p + 1]));
  const double2 first = reinterpret_cast<const double2*>(xy)[b];
  LongRing r{n, P2{first.x, first.y}, first.x, first.y, first.x, first.y};
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kWave) {
    const double2 v = reinterpret_cast<const double2*>(xy)[b + i];
    r.xmin = fmin(r.xmin, v.x); r.xmax = fmax(r.xmax, v.x);
    r.ymin = fmin(r.ymin, v.y); r.ymax = fmax(r.ymax, v.y);
    pts[i] = double2{v.x - first.x, v.y - first.y};
  }
  __syncthreads();
  return r;
}

// The loops of the polygon kernels of the units that walk points against rings (polygon_join.hip, buffered_counts.hip,
// nearest_boundaries.hip): every listed ring of a route, loaded, with its bounds on the coordinates as given reduced over
// the wave, handed to body(ListedRing).  Short: `waves` waves a workgroup, one ring a wave; long: a workgroup of one wave
// and its stage pts[SEGGER_MORPH_MAX_VERTS].
// What a body receives, the same in every lane but for a RegRing's vertex: polygon p, its store `ring` of n >= 3 open
// vertices translated to `first`, and xmin .. ymax, the ring's bounds on the coordinates as given.
template <class Ring>
struct ListedRing { Ring ring; int n; P2 first; double xmin, ymin, xmax, ymax; int64_t p; };

template <class Body>
__device__ __forceinline__ void short_ring_loop(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                                const int32_t* __restrict__ words, const int32_t* __restrict__ list, int waves, Body&& body) {
  const int count = words[kWordShort];
  const int n_waves = (int)gridDim.x * waves;
  for (int w = (int)blockIdx.x * waves + (int)(threadIdx.x >> 6); w < count; w += n_waves) {                   // wave-uniform
    const int64_t p = list[w];
    const ShortRing s = load_short_ring(off, xy, p);                 // 3 .. 64 vertices
    body(ListedRing<RegRing>{s.ring, s.n, s.first, wave_min_f64(s.mine.x), wave_min_f64(s.mine.y), wave_max_f64(s.mine.x),
                             wave_max_f64(s.mine.y), p});
  }
}

template <class Body>
__device__ __forceinline__ void long_ring_loop(const int64_t* __restrict__ off, const double* __restrict__ xy,
                                               const int32_t* __restrict__ words, const int32_t* __restrict__ list,
                                               double2* __restrict__ pts, Body&& body) {
  const int count = words[kWordLong];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int64_t p = list[w];
    const LongRing r = stage_long_ring(off, xy, p, pts);
    body(ListedRing<LdsRing>{LdsRing{pts}, r.n, r.first, wave_min_f64(r.xmin), wave_min_f64(r.ymin), wave_max_f64(r.xmax),
                             wave_max_f64(r.ymax), p});
  }
}

// ---------------------------------------------------------------- gift wrapping: the march, one wave ---
// The convex hull of the n points of a store (own / uni as above), counter-clockwise from the lowest (x, then y, then
// index) point: from the current hull vertex the next one is the most clockwise point as seen from it, ties (collinear
// with it) go to the larger distance, then to the lower index, and a point that coincides with the current vertex never
// competes.  Collinear and duplicate points therefore never enter the hull, and the march is back at its start after
// h <= n steps.  morphology.hip marches over a ring's vertices, boundaries.hip over a cell's transcripts.
struct Cand { int i; double dx, dy; };                               // a vertex and its offset from the current hull vertex

// is b ahead of a in the march?  (i < 0: no candidate; neither offset is zero)
__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {
  if (b.i < 0) return false;
  if (a.i < 0) return true;
  const double cr = a.dx * b.dy - a.dy * b.dx;                       // < 0: b is to the right of current -> a
  if (cr != 0.0) return cr < 0.0;
  const double da = a.dx * a.dx + a.dy * a.dy, db = b.dx * b.dx + b.dy * b.dy;
  if (da != db) return db > da;
  return b.i < a.i;
}

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    Cand o;
    o.i = __shfl_xor(c.i, m, kWave);
    o.dx = shfl_xor_f64(c.dx, m);
    o.dy = shfl_xor_f64(c.dy, m);
    if (cand_better(c, o)) c = o;
  }
  c.i = __builtin_amdgcn_readfirstlane(c.i);                         // one answer per wave whatever the inputs hold
  return c;
}

// the point that follows hull vertex p (the same in every lane) among the n of the store; i < 0: every point equals p
template <class Ring>
__device__ __forceinline__ Cand march_step(const Ring& ring, int n, P2 p) {
  const int lane = threadIdx.x & (kWave - 1);
  Cand best{-1, 0.0, 0.0};
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    if (i < n) {
      const P2 q = ring.own(i);
      const Cand c{i, q.x - p.x, q.y - p.y};
      if ((c.dx != 0.0 || c.dy != 0.0) && cand_better(best, c)) best = c;
    }
  }
  return wave_best(best);
}

// where the march starts: the index of the lowest (x, then y, then index) of the n >= 1 points, the same in every lane
template <class Ring>
__device__ __forceinline__ int march_start(const Ring& ring, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  int s_i = -1;
  double s_x = 0.0, s_y = 0.0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    if (i < n) {
      const P2 p = ring.own(i);
      if (s_i < 0 || p.x < s_x || (p.x == s_x && p.y < s_y)) { s_i = i; s_x = p.x; s_y = p.y; }
    }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const int oi = __shfl_xor(s_i, m, kWave);
    const double ox = shfl_xor_f64(s_x, m), oy = shfl_xor_f64(s_y, m);
    const bool take = oi >= 0 && (s_i < 0 || ox < s_x || (ox == s_x && (oy < s_y || (oy == s_y && oi < s_i))));
    if (take) { s_i = oi; s_x = ox; s_y = oy; }
  }
  return __builtin_amdgcn_readfirstlane(s_i);
}

// ---------------------------------------------------------------- host: workspace and arguments ---
// the head of a ring consumer's workspace: the words, then one int32 list per route, each long enough for every polygon
struct RingLists { size_t words, list_short, list_long; };
inline RingLists take_ring_lists(Carver& c, int64_t n_polygons) {
  const size_t list_bytes = (size_t)n_polygons * sizeof(int32_t);
  return RingLists{c.take(kRingWordsBytes), c.take(list_bytes), c.take(list_bytes)};      // a braced list: left to right
}

// What an entry point rejects about the pointers of a non-empty call: the ring's own (ring_offsets, xy, workspace) and, in
// the same order and the same messages, the unit's further ones: whether the required ones are there, whether they are
// aligned, and how the two alignment messages name the lot ("ring_offsets and ...", "... xy").
struct OtherPointers { bool present, aligned8, aligned16; const char *names8, *names16; };
inline int check_ring_call(const char* who, const int64_t* ring_offsets, const double* xy, int64_t n_vertices, const void* workspace,
                           int64_t workspace_bytes, size_t need, const OtherPointers& o) {
  SEGGER_REQUIRE(ring_offsets && workspace && o.present, "%s: NULL pointer", who);
  SEGGER_REQUIRE(xy || n_vertices == 0, "%s: NULL xy with n_vertices > 0", who);
  SEGGER_REQUIRE(is_aligned(ring_offsets, 8) && o.aligned8, "%s: %s must be 8-byte aligned", who, o.names8);
  SEGGER_REQUIRE(is_aligned(xy, 16) && o.aligned16, "%s: %s must be 16-byte aligned", who, o.names16);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  SEGGER_REQUIRE((size_t)workspace_bytes >= need, "%s: workspace %lld < %zu bytes", who, (long long)workspace_bytes, need);
  return SEGGER_OK;
}

}  // namespace segger
