// segger_cell_outlines_large: segger_cell_outlines with a third route, through global memory, for the cells whose distinct
// points exceed the LDS budget (or a caller's lower `lds_max_points`).  include/segger_amd.h has the contract.
//
// The front end, the back end and the host code that drives them are cell_rings.h's, the two LDS routes outline_cell.h's,
// all shared with outlines.hip.  New here:
//   outl_bin_kernel      as out_bin_kernel; with lds_max_points = 0 every present cell goes to the large list at once;
//   outl_lds_kernel<N>   outline_cell<N> with the limit min(N, lds_max_points): a cell that exceeds it in stage 1 takes a
//                        slice of the large-cell workspace with one atomic bump of its rows and is appended to the large
//                        list; when the slices would exceed large_rows it is refused through the counters instead;
//   outl_large_kernel    one 256-thread WORKGROUP per listed cell, the cell's state in its slice, 32-bit ids.
// The same six stages as outline_cell<N>, on the same predicates (outline_cell.h), so a ring has the same bytes on either
// route: every stage's result is fixed by the points alone -- the sorted distinct points, the apex of an edge (the maximum
// of a total order), the fixed points of the peels and of the labels, the minimum that seeds the walk -- except the
// component areas, which are sums: those are added in the LDS route's order (64 partial sums by triangle index mod 64, then
// the butterfly), one wave per component.
//
// What differs is how a stage is carried out:
//   1 the rows are copied to the slice and sorted there by a bitonic network over the next power of two in which an index
//     past the rows counts as +inf and is never touched (every comparator orders ascending, so such an element never
//     moves); duplicates are squeezed out in place, 256 at a time;
//   2 the apex search uses all four waves and is pruned: the points are sorted by x, and a better apex lies inside or on the
//     circle through a, b and the best so far, so each wave walks outward from the edge, 32 points to the left and 32 to the
//     right per step, and stops when a step finds nothing inside the circle's x-extent.  The extent comes from a
//     circumcentre whose rounding error is bounded term by term and added (circle_x_extent): it is never too narrow, so a
//     point ON the circle is still seen and the tie rule still decides; an edge with nothing on its left scans all d.  The
//     directed-edge hash is open addressing over 8 d slots of (key, id); a wave reads 64 consecutive slots at once;
//   5 the components' areas are shared out over the waves; each wave scans from its root upward.
// Every loop has its trip count fixed before it is entered, as in outline_cell<N>.  The work per triangle is a chain of
// dependent reads of the slice (L2 latency), not arithmetic: see README for the measured cost per cell.
//
// Workspace per large-cell row, bytes (175): 16 points, 1 multiplicity flag, 24 triangle vertices (3 uint32 x 2 triangles),
// 24 twins, 6 predicate bits, 8 labels, 64 + 32 hash keys and ids (8 slots; the keys' region later holds the per-vertex
// minima).  A cell of more than 2^28 rows is refused: directed-edge ids and slot numbers are 32-bit.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel of the unit, the library's
// included; outl_large_kernel 184 VGPRs (two waves per SIMD), 384 B of LDS; outl_lds_kernel<256> 17408 B and outl_lds_kernel<2048> 139264 B of LDS.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "sort_config.h"
#include "cell_rings.h"
#include "outline_cell.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kLgThreads = 256, kLgWaves = kLgThreads / kWave, kLgHalf = kWave / 2;
constexpr uint32_t kNoneL = 0xffffffffu, kUnsetL = 0xfffffffeu;      // as kNone, kUnset
constexpr unsigned long long kEmptyKey = ~0ull, kNoKey = ~0ull - 1;  // an empty slot; what a lane past the table reads
constexpr int kLgMaxRows = 1 << 28;                                  // 6 d edge ids and 8 d slots stay below 2^31
constexpr int kWordLarge = 3, kWordBump = 4;                         // words: the large list's length; int64 rows taken
enum { kLargeCells = 10, kLargePoints = 11, kLargeRows = 12 };       // after outline_cell.h's words
static_assert(kLargeRows + 1 == SEGGER_OUTLINE_LARGE_COUNTERS, "the header documents the block");
static_assert(kLgWaves == 4 && (kWordBump + 2) * sizeof(int32_t) <= kRingWordsBytes && kWordBump % 2 == 0, "the words' region");

// the arrays over all large_rows rows; a cell whose slice starts at row `at` owns [at, at + len) of each, scaled
struct LargeArrays {
  double2* pts;
  uint8_t* flg;
  uint32_t *tv, *nb;
  uint8_t* ef;
  uint32_t* label;
  unsigned long long* hkey;
  uint32_t* hid;
};

struct LargeLists { int32_t* words; int32_t* list; int64_t* at; };

// Segment j of n rows needs the large route: its slice and its place in the list, or the refusal.  One thread calls this.
__device__ __forceinline__ void take_large(const BndSegs& s, int j, int n, const LargeLists& ll, int64_t large_rows,
                                           unsigned long long* __restrict__ counters) {
  bool fits = n <= kLgMaxRows;
  unsigned long long at = 0;
  if (fits) {
    at = atomicAdd(reinterpret_cast<unsigned long long*>(ll.words + kWordBump), (unsigned long long)n);
    fits = at + (unsigned long long)n <= (unsigned long long)large_rows;
    // A refused cell's rows are NOT given back: a cell that bumped in between holds a slice above them, and a counter
    // lowered under it would hand that slice out again.  So once a cell did not fit, every later one is refused too.
  }
  if (!fits) {
    atomicAdd(counters + kRefused, 1ull);
    atomicMax(counters + kRefusedCell, (s.keys[s.head[j]] >> 32) + 1ull);
    s.hull_n[j] = 0;
    return;
  }
  const int pos = atomicAdd(&ll.words[kWordLarge], 1);
  ll.list[pos] = j;
  ll.at[pos] = (int64_t)at;
  atomicAdd(counters + kLargeRows, (unsigned long long)n);
}

// ---------------------------------------------------------------- routes ---
__global__ __launch_bounds__(kBndThreads) void outl_bin_kernel(BndSegs s, unsigned long long* __restrict__ counters,
                                                               int32_t* __restrict__ list_short, int32_t* __restrict__ list_long,
                                                               LargeLists ll, int lds_max, int64_t large_rows) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t present = (int64_t)counters[kPresent];
  const int32_t n_counted = (int32_t)counters[kCounted];
  const int64_t stride = (int64_t)gridDim.x * kBndThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kBndThreads + (threadIdx.x & ~(kWave - 1)); base < present; base += stride) {
    const int64_t j = base + lane;
    int route = -1, n = 0;
    if (j < present) {
      n = (j + 1 < present ? s.head[j + 1] : n_counted) - s.head[j];
      s.len[j] = n;
      route = lds_max == 0 ? 2 : n > kOutSmall;
    }
    append_by_route(route, j, ll.words, list_short, list_long);
    if (route == 2) take_large(s, (int)j, n, ll, large_rows, counters);
  }
}

template <int N>
__global__ __launch_bounds__(kWave) void outl_lds_kernel(const double* __restrict__ xy, BndSegs s, int word,
                                                         const int32_t* __restrict__ list, OutParams prm, int limit, LargeLists ll,
                                                         int64_t large_rows, unsigned long long* __restrict__ counters) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[OutLds<N>::kBytes];
  const int count = ll.words[word];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int j = list[w];
    __syncthreads();                                                 // the previous cell's readers are done
    int h = outline_cell<N>(xy, s, j, lds, prm, limit);
    if (h == kTooMany) {
      if (threadIdx.x == 0) take_large(s, j, s.len[j], ll, large_rows, counters);
      continue;                                                      // hull_n[j] is the large kernel's, or 0 by the refusal
    }
    if (h < 0) {
      if (threadIdx.x == 0) {
        atomicAdd(counters + kFailed, 1ull);
        atomicMax(counters + kFailedCell, (s.keys[s.head[j]] >> 32) + 1ull);
      }
      h = 0;
    }
    if (threadIdx.x == 0) s.hull_n[j] = h;
  }
}

// ---------------------------------------------------------------- the large cell: workgroup helpers ---
struct LgShared {
  double f[kLgWaves];
  double2 p[kLgWaves];
  int i[kLgWaves], k[kLgWaves];
};

__device__ __forceinline__ uint32_t uniu(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The x-extent of the circle through a, b, p (not collinear), never too narrow.  With a at the origin the centre is
// (nx, ny) / (2 D); each of D, nx, ny is a difference of two products of rounded differences, so its absolute error is below
// 2^-48 times the sum of the two products' magnitudes (a dozen roundings of 2^-53 each, with room).  The bounds below divide
// the largest numerator by the smallest denominator; the radius is the centre's distance from a.  D within its error of
// zero, or anything not finite: no bound.
struct Extent { double lo, hi; };
__device__ __forceinline__ Extent circle_x_extent(double2 pa, double2 pb, double2 pp) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double E = 3.5527136788005009e-15;                           // 2^-48
  const double bx = pb.x - pa.x, by = pb.y - pa.y, px = pp.x - pa.x, py = pp.y - pa.y;
  const double t1 = bx * py, t2 = by * px;
  const double D = t1 - t2, eD = E * (fabs(t1) + fabs(t2));
  const double bb = bx * bx + by * by, qq = px * px + py * py;
  const double x1 = py * bb, x2 = by * qq, y1 = bx * qq, y2 = px * bb;
  const double nx = x1 - x2, ny = y1 - y2;
  const double enx = E * (fabs(x1) + fabs(x2)), eny = E * (fabs(y1) + fabs(y2));
  const double den_min = 2.0 * (fabs(D) - eD), den_max = 2.0 * (fabs(D) + eD);
  if (!(den_min > 0.0)) return Extent{-inf, inf};
  const double Ux = (fabs(nx) + enx) / den_min, Uy = (fabs(ny) + eny) / den_min;      // |centre - a| per axis, from above
  const double Lx = fmax(fabs(nx) - enx, 0.0) / den_max;                                // and from below
  const double cx = nx / (2.0 * D);
  const double R = sqrt(Ux * Ux + Uy * Uy);
  const double pad = (Ux - Lx) + E * (fabs(pa.x) + Ux + R);
  const double lo = pa.x + cx - R - pad, hi = pa.x + cx + R + pad;
  if (!(lo - lo == 0.0) || !(hi - hi == 0.0)) return Extent{-inf, inf};
  return Extent{lo, hi};
}

// the apex of a -> b among the d points sorted by x, -1 when nothing is left of it; the same in every thread.  Two barriers.
__device__ __forceinline__ int find_apex_large(const double2* __restrict__ pts, int d, int a, int b, LgShared& sh) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double2 pa = pts[a], pb = pts[b];
  int best = -1;
  double2 pbest = double2{0.0, 0.0};
  double lo = -inf, hi = inf;
  const int mid = (int)(((int64_t)a + b) >> 1);
  const int steps = d / (kLgHalf * kLgWaves) + 2;                    // all waves together pass every point on both sides
  for (int t = 0; t < steps; ++t) {
    const int64_t o = ((int64_t)t * kLgWaves + wave) * kLgHalf;
    const int64_t i64 = lane < kLgHalf ? (int64_t)mid - o - lane : (int64_t)mid + 1 + o + (lane - kLgHalf);
    bool in = i64 >= 0 && i64 < d;
    const int i = in ? (int)i64 : 0;
    const double2 q = pts[i];
    in = in && !(q.x < lo) && !(q.x > hi);
    if (__ballot(in) == 0) break;                                    // sorted by x: nothing farther out is inside either
    const bool cand = in && i != a && i != b && orient2d(pa, pb, q) > 0.0 && apex_better_at(a, b, pa, pb, best, pbest, i, q);
    if (__ballot(cand) == 0) continue;
    int ci = cand ? i : best;
    double2 cq = cand ? q : pbest;
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      const int oi = __shfl_xor(ci, m, kWave);
      const double2 oq = double2{shfl_xor_f64(cq.x, m), shfl_xor_f64(cq.y, m)};
      if (apex_better_at(a, b, pa, pb, ci, cq, oi, oq)) { ci = oi; cq = oq; }
    }
    best = uni(ci);
    pbest = double2{readlane_f64(cq.x, 0), readlane_f64(cq.y, 0)};
    const Extent x = circle_x_extent(pa, pb, pbest);
    lo = x.lo; hi = x.hi;
  }
  if (lane == 0) { sh.i[wave] = best; sh.p[wave] = pbest; }
  __syncthreads();
  int r = -1;
  double2 pr = double2{0.0, 0.0};
#pragma unroll
  for (int w = 0; w < kLgWaves; ++w) {
    const int oi = sh.i[w];
    const double2 oq = sh.p[w];
    if (apex_better_at(a, b, pa, pb, r, pr, oi, oq)) { r = oi; pr = oq; }
  }
  __syncthreads();                                                   // sh is free again
  return uni(r);
}

// the id of directed edge a -> b, -1 if it has no triangle yet; with `id` >= 0: insert it (kContradiction if it is there).
// Every wave reads the same slots and returns the same: nothing is written to the table between the caller's last barrier
// and the one below, which an insert passes in all 256 threads before wave 0 writes.  The caller's next barrier publishes
// the write.  (In a workgroup of several waves a read that another wave's write could overtake would let the waves take
// different returns; outline_cell<N> has one wave and needs neither barrier.)
__device__ __forceinline__ int hash_edge_large(unsigned long long* __restrict__ hkey, uint32_t* __restrict__ hid, uint32_t slots,
                                               int a, int b, int id) {
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long key = ((unsigned long long)(uint32_t)a << 32) | (unsigned long long)(uint32_t)b;
  const uint32_t h = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32);
  const uint32_t slot = (uint32_t)(((unsigned long long)h * slots) >> 32);
  const int trips = (int)((slots + (uint32_t)kWave - 1) / (uint32_t)kWave);
  for (int t = 0; t < trips; ++t) {
    const unsigned long long off = (unsigned long long)t * kWave + lane;
    const bool in = off < slots;
    unsigned long long idx = (unsigned long long)slot + off;
    if (idx >= slots) idx -= slots;
    const unsigned long long k = in ? hkey[idx] : kNoKey;
    const uint32_t v = in ? hid[idx] : 0u;
    const unsigned long long empty = __ballot(k == kEmptyKey), match = __ballot(k == key);
    const unsigned long long before = empty ? ((1ull << __builtin_ctzll(empty)) - 1ull) : ~0ull;
    if (match & before) {
      if (id >= 0) return kContradiction;
      return (int)__shfl((int)v, (int)__builtin_ctzll(match & before), kWave);
    }
    if (empty) {
      if (id >= 0) {
        __syncthreads();                                             // every wave has read this window: none meets the new key in it
        if (threadIdx.x == (unsigned)__builtin_ctzll(empty)) { hkey[idx] = key; hid[idx] = (uint32_t)id; }
      }
      return -1;
    }
  }
  return kContradiction;                                             // a full table: more edges than a triangulation has
}

// ---------------------------------------------------------------- the large cell ---
// The outline of segment j in its slice: its vertices to out[0 .. h), h returned in every thread; 0: no polygon;
// kContradiction: refused.  d_out: its distinct points.
__device__ __forceinline__ int outline_large(const double* __restrict__ xy, const BndSegs& s, int j, const LargeArrays& A, int64_t at0,
                                             const OutParams& prm, LgShared& sh, int& d_out) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  double2* pts = A.pts + at0;
  uint8_t* flg = A.flg + at0;
  uint32_t* tv = A.tv + 6 * at0;
  uint32_t* nb = A.nb + 6 * at0;
  uint8_t* ef = A.ef + 6 * at0;
  uint32_t* label = A.label + 2 * at0;
  unsigned long long* hkey = A.hkey + 8 * at0;
  uint32_t* hid = A.hid + 8 * at0;
  unsigned long long* vmin = hkey;
  const int64_t b0 = s.head[j];
  const int n = uni(s.len[j]);
  double2* out = s.hull + b0;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  d_out = 0;

  // ---- 1: distinct points, sorted by (x, y)
  for (int k = tid; k < n; k += kLgThreads) {
    const P2 p = point_at(xy, s.keys, b0 + k);
    pts[k] = double2{p.x, p.y};
  }
  int64_t P = 2;
  for (int q = 0; q < 31 && P < n; ++q) P <<= 1;
  __syncthreads();
  for (int64_t k = 2; k <= P; k <<= 1) {
    for (int64_t jj = k >> 1; jj > 0; jj >>= 1) {
      const bool flip = jj == (k >> 1);                              // the first pass of a merge pairs i with its mirror image
      for (int64_t i = tid; i < (P >> 1); i += kLgThreads) {
        const int64_t lo = ((i & ~(jj - 1)) << 1) | (i & (jj - 1));
        const int64_t hi = flip ? (lo | (k - 1)) - (i & (jj - 1)) : (lo | jj);
        if (hi >= n) continue;                                       // +inf: stays where it is
        const double2 a = pts[lo], b = pts[hi];
        if (lex_less(b, a)) { pts[lo] = b; pts[hi] = a; }
      }
      __syncthreads();
    }
  }
  int d = 0;                                                         // in place: an element never moves to a higher index
  for (int base = 0; base < n; base += kLgThreads) {
    const int i = base + tid;
    const bool in = i < n;
    const double2 p = pts[in ? i : 0];
    bool first = false, again = false;
    if (in) {
      const double2 before = pts[i > 0 ? i - 1 : 0];
      first = i == 0 || before.x != p.x || before.y != p.y;
      if (i + 1 < n) { const double2 after = pts[i + 1]; again = after.x == p.x && after.y == p.y; }
    }
    const unsigned long long mask = __ballot(first);
    if (lane == 0) sh.i[wave] = (int)__popcll(mask);
    __syncthreads();                                                 // the chunk is read; the counts are there
    int pos = d + (int)__popcll(mask & ((1ull << lane) - 1)), all = 0;
#pragma unroll
    for (int w = 0; w < kLgWaves; ++w) {
      const int c = sh.i[w];
      if (w < wave) pos += c;
      all += c;
    }
    if (first) { pts[pos] = p; flg[pos] = again ? 1 : 0; }
    d += all;
    __syncthreads();
  }
  d_out = d;
  if (d < 3) return 0;

  // ---- 2: Delaunay, edge by edge
  const uint32_t slots = 8u * (uint32_t)d;
  const int max_tris = 2 * d, max_edges = 6 * d;
  for (uint32_t k = tid; k < slots; k += kLgThreads) hkey[k] = kEmptyKey;
  int bi = -1;
  {
    double bd = inf;
    const double2 p0 = pts[0];
    for (int i = 1 + tid; i < d; i += kLgThreads) {                  // ascending: a thread's ties keep the lower index
      const double dx = pts[i].x - p0.x, dy = pts[i].y - p0.y, dd = dx * dx + dy * dy;
      if (dd < bd) { bd = dd; bi = i; }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      const double od = shfl_xor_f64(bd, m);
      const int oi = __shfl_xor(bi, m, kWave);
      if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
    }
    if (lane == 0) { sh.f[wave] = bd; sh.i[wave] = bi; }
    __syncthreads();
    bd = sh.f[0]; bi = sh.i[0];
#pragma unroll
    for (int w = 1; w < kLgWaves; ++w) {
      const double od = sh.f[w];
      const int oi = sh.i[w];
      if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
    }
    bi = uni(bi);
    __syncthreads();
  }
  int sa = 0, sb = bi;
  int sc = find_apex_large(pts, d, sa, sb, sh);
  if (sc < 0) { sa = bi; sb = 0; sc = find_apex_large(pts, d, sa, sb, sh); }
  if (sc < 0) return 0;                                              // nothing on either side of a Delaunay edge: collinear
  if (tid == 0) {
    tv[0] = (uint32_t)sa; tv[1] = (uint32_t)sb; tv[2] = (uint32_t)sc;
    nb[0] = kUnsetL; nb[1] = kUnsetL; nb[2] = kUnsetL;
  }
  int T = 1;
  __syncthreads();
  if (hash_edge_large(hkey, hid, slots, sa, sb, 0) == kContradiction) return kContradiction;
  __syncthreads();
  if (hash_edge_large(hkey, hid, slots, sb, sc, 1) == kContradiction) return kContradiction;
  __syncthreads();
  if (hash_edge_large(hkey, hid, slots, sc, sa, 2) == kContradiction) return kContradiction;
  __syncthreads();
  for (int e = 0; e < max_edges; ++e) {                              // the triangle list is the queue: T grows under e
    if (e >= 3 * T) break;
    const uint32_t twin = nb[e], va = tv[e], vb = tv[next_edge(e)];   // one round trip for the three
    if (uniu(twin) != kUnsetL) continue;
    const int a = (int)uniu(va), b = (int)uniu(vb);                  // e is a -> b; its twin b -> a
    const int f = hash_edge_large(hkey, hid, slots, b, a, -1);
    if (f == kContradiction) return kContradiction;
    if (f >= 0) {
      if (uniu(nb[f]) != kUnsetL) return kContradiction;
      __syncthreads();                                               // every wave has read nb[e] and nb[f]: all return, or none
      if (tid == 0) { nb[e] = (uint32_t)f; nb[f] = (uint32_t)e; }
      __syncthreads();
      continue;
    }
    const int c = find_apex_large(pts, d, b, a, sh);
    if (c < 0) {
      if (tid == 0) nb[e] = kNoneL;
      __syncthreads();
      continue;
    }
    if (T >= max_tris) return kContradiction;                        // more than 2 n - 5 triangles: not a triangulation
    const int g = 3 * T;
    ++T;
    if (tid == 0) {
      tv[g] = (uint32_t)b; tv[g + 1] = (uint32_t)a; tv[g + 2] = (uint32_t)c;
      nb[g] = (uint32_t)e; nb[e] = (uint32_t)g; nb[g + 1] = kUnsetL; nb[g + 2] = kUnsetL;
    }
    // all three edges go into the table, b -> a too: a later edge that asks for it finds a twin already taken
    if (hash_edge_large(hkey, hid, slots, b, a, g) == kContradiction) return kContradiction;
    __syncthreads();
    if (hash_edge_large(hkey, hid, slots, a, c, g + 1) == kContradiction) return kContradiction;
    __syncthreads();
    if (hash_edge_large(hkey, hid, slots, c, b, g + 2) == kContradiction) return kContradiction;
    __syncthreads();
  }
  if (uniu(nb[3 * T - 1]) == kUnsetL) return kContradiction;         // the bound ended the loop, not the queue
  const int E = 3 * T;

  // ---- 3: d_max, the largest nearest-neighbour distance; the hash is dead, its keys' region holds the per-vertex minima
  __syncthreads();
  for (int v = tid; v < d; v += kLgThreads) vmin[v] = 0x7ff0000000000000ull;
  __syncthreads();
  for (int e = tid; e < E; e += kLgThreads) {
    const int a = (int)tv[e], b = (int)tv[next_edge(e)];
    const double dx = pts[a].x - pts[b].x, dy = pts[a].y - pts[b].y;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(dx * dx + dy * dy);   // >= 0: ordered as integers
    atomicMin(&vmin[a], bits);
    atomicMin(&vmin[b], bits);
  }
  __syncthreads();
  double d_max = 0.0;
  for (int v = tid; v < d; v += kLgThreads) d_max = fmax(d_max, flg[v] ? 0.0 : sqrt(__longlong_as_double((long long)vmin[v])));
  d_max = wave_max_f64(d_max);
  if (lane == 0) sh.f[wave] = d_max;
  __syncthreads();
  d_max = fmax(fmax(sh.f[0], sh.f[1]), fmax(sh.f[2], sh.f[3]));
  __syncthreads();

  // ---- 4: the static predicates of every directed edge, then the two peels
  const double t_long = (2.0 * prm.connectivity) * d_max, t_mid = (1.5 * prm.connectivity) * d_max;
  const double max_angle = 180.0 - 11.25 / prm.connectivity;
  for (int e = tid; e < E; e += kLgThreads) {
    const int e1 = next_edge(e), e2 = next_edge(e1);
    const double2 pa = pts[tv[e]], pb = pts[tv[e1]], pc = pts[tv[e2]];
    const double dx = pa.x - pb.x, dy = pa.y - pb.y;
    const double len = sqrt(dx * dx + dy * dy);
    const double ux = pa.x - pc.x, uy = pa.y - pc.y, vx = pb.x - pc.x, vy = pb.y - pc.y;
    double cs = (ux * vx + uy * vy) / (sqrt(ux * ux + uy * uy) * sqrt(vx * vx + vy * vy) + 1e-12);
    cs = fmin(fmax(cs, -1.0), 1.0);
    const double angle = acos(cs) * (180.0 / 3.141592653589793);
    ef[e] = (uint8_t)((len > t_long ? 1 : 0) | (((len > t_mid && angle > 90.0) || angle > max_angle) ? 2 : 0));
  }
  for (int t = tid; t < T; t += kLgThreads) label[t] = (uint32_t)t;
  __syncthreads();
  for (int phase = 1; phase <= 2; ++phase) {
    for (int round = 0; round < T; ++round) {                        // a round without a removal is the fixed point
      int changed = 0;
      for (int t = tid; t < T; t += kLgThreads) {
        if (label[t] == kNoneL) continue;
        for (int k = 0; k < 3; ++k) {
          const int e = 3 * t + k;
          if (!(ef[e] & phase)) continue;
          const uint32_t o = nb[e];
          if (o == kNoneL || label[o / 3] == kNoneL) { label[t] = kNoneL; changed = 1; break; }
        }
      }
      if (__syncthreads_or(changed) == 0) break;
    }
  }

  // ---- 5: components over shared edges, the largest by area
  for (int round = 0; round < T; ++round) {
    int changed = 0;
    for (int t = tid; t < T; t += kLgThreads) {
      const uint32_t mine = label[t];
      if (mine == kNoneL) continue;
      uint32_t m = mine;
      for (int k = 0; k < 3; ++k) {
        const uint32_t o = nb[3 * t + k];
        if (o != kNoneL) { const uint32_t l2 = label[o / 3]; if (l2 < m) m = l2; }      // kNoneL is the largest value
      }
      const uint32_t l3 = label[m];
      if (l3 < m) m = l3;
      if (m < mine) { label[t] = m; changed = 1; }
    }
    if (__syncthreads_or(changed) == 0) break;
  }
  // wave w takes the roots of the chunks w, w + 4, ...; a root's sum runs in outline_cell's order: per lane the members
  // u = lane (mod 64) ascending (a member is never below its root), then the butterfly
  int best_root = -1, best_low = 0;
  double best_area = -1.0;
  for (int base = wave * kWave; base < T; base += kLgThreads) {
    const int t = base + lane;
    unsigned long long roots = __ballot(t < T && label[t] == (uint32_t)t);
    const int n_roots = (int)__popcll(roots);
    for (int q = 0; q < n_roots; ++q) {
      const int root = base + (int)__builtin_ctzll(roots);
      roots &= roots - 1;
      double area2 = 0.0;
      int low = d;
      for (int u = base + lane; u < T; u += kWave) {
        if (label[u] != (uint32_t)root) continue;
        const int va = (int)tv[3 * u], vb = (int)tv[3 * u + 1], vc = (int)tv[3 * u + 2];
        area2 += orient2d(pts[va], pts[vb], pts[vc]);
        low = min(low, min(va, min(vb, vc)));
      }
      area2 = wave_sum_f64(area2);
#pragma unroll
      for (int m = 1; m < kWave; m <<= 1) low = min(low, __shfl_xor(low, m, kWave));
      low = uni(low);
      if (area2 > best_area || (area2 == best_area && low < best_low)) { best_area = area2; best_low = low; best_root = root; }
    }
  }
  if (lane == 0) { sh.f[wave] = best_area; sh.i[wave] = best_root; sh.k[wave] = best_low; }
  __syncthreads();
  best_root = -1; best_low = 0; best_area = -1.0;
#pragma unroll
  for (int w = 0; w < kLgWaves; ++w) {                               // larger area, then lower lowest vertex, then found first
    const double ar = sh.f[w];
    const int ro = sh.i[w], lw = sh.k[w];
    if (ro < 0) continue;
    if (best_root < 0 || ar > best_area || (ar == best_area && (lw < best_low || (lw == best_low && ro < best_root)))) {
      best_area = ar; best_low = lw; best_root = ro;
    }
  }
  best_root = uni(best_root);
  best_low = uni(best_low);
  __syncthreads();
  if (best_root < 0) return 0;                                       // everything was peeled

  // ---- 6: the ring, interior on the left, from the component's lowest vertex
  int e0 = max_edges;
  for (int e = tid; e < E; e += kLgThreads) {
    if (label[e / 3] != (uint32_t)best_root || tv[e] != (uint32_t)best_low) continue;
    const uint32_t o = nb[e];
    if (o == kNoneL || label[o / 3] == kNoneL) e0 = min(e0, e);
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) e0 = min(e0, __shfl_xor(e0, m, kWave));
  if (lane == 0) sh.i[wave] = e0;
  __syncthreads();
  e0 = uni(min(min(sh.i[0], sh.i[1]), min(sh.i[2], sh.i[3])));
  __syncthreads();
  if (e0 >= E) return kContradiction;
  int h = 0, x = e0;
  bool closed = false;
  for (int it = 0; it < E; ++it) {                                   // every step consumes one directed edge of the component
    const uint32_t o = uniu(nb[x]);
    if (o == kNoneL || uniu(label[o / 3]) == kNoneL) {
      if (h >= d) return kContradiction;
      if (tid == 0) out[h] = pts[uniu(tv[x])];
      ++h;
      x = next_edge(x);
    } else {
      x = next_edge((int)o);                                         // across the interior edge: the next triangle of the fan
    }
    if (x == e0) { closed = true; break; }
  }
  return closed ? h : kContradiction;
}

__global__ __launch_bounds__(kLgThreads) void outl_large_kernel(const double* __restrict__ xy, BndSegs s, LargeLists ll, LargeArrays A,
                                                                OutParams prm, unsigned long long* __restrict__ counters) {
  __shared__ LgShared sh;
  const int count = ll.words[kWordLarge];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int j = ll.list[w];
    const int64_t at0 = ll.at[w];
    __syncthreads();                                                 // the previous cell's readers are done
    int d = 0;
    int h = outline_large(xy, s, j, A, at0, prm, sh, d);
    if (threadIdx.x == 0) {
      if (h < 0) {
        atomicAdd(counters + kFailed, 1ull);
        atomicMax(counters + kFailedCell, (s.keys[s.head[j]] >> 32) + 1ull);
        h = 0;
      }
      s.hull_n[j] = h;
      atomicAdd(counters + kLargeCells, 1ull);
      atomicAdd(counters + kLargePoints, (unsigned long long)d);
    }
  }
}

// ---------------------------------------------------------------- host ---
// cell_rings.h's head, then the large list and the arrays over large_rows.  With n_rows below 2^31 every term is below 2^38
// bytes: nothing here can overflow.
struct LargeLayout {
  CellRingsLayout head;
  size_t list_large, at_large, pts, flg, tv, nb, ef, label, hkey, hid, total;
};

LargeLayout large_layout(int64_t n_rows, int64_t n_cells, int64_t large_rows) {
  LargeLayout l;
  Carver c;
  l.head = take_cell_rings(c, n_rows, n_cells);
  const size_t c4 = (size_t)l.head.cells_cap * 4;
  const size_t r = (size_t)(large_rows > 0 ? large_rows : 1);
  l.list_large = c.take(c4);
  l.at_large = c.take(2 * c4);
  l.pts = c.take(16 * r);
  l.flg = c.take(r);
  l.tv = c.take(24 * r);
  l.nb = c.take(24 * r);
  l.ef = c.take(6 * r);
  l.label = c.take(8 * r);
  l.hkey = c.take(64 * r);
  l.hid = c.take(32 * r);
  l.total = c.total();
  return l;
}

int large_check_sizes(const char* who, int64_t n_rows, int64_t n_cells, int64_t large_rows) {
  const int rc = bnd_check_sizes(who, n_rows, n_cells);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(large_rows >= 0 && large_rows <= n_rows, "%s: large_rows = %lld outside 0 .. n_rows", who, (long long)large_rows);
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_cell_outlines_large_workspace_bytes(int64_t n_rows, int64_t n_cells, int64_t large_rows) {
  const int rc = large_check_sizes("segger_cell_outlines_large_workspace_bytes", n_rows, n_cells, large_rows);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)large_layout(n_rows, n_cells, large_rows).total;
}

extern "C" int segger_cell_outlines_large(const double* xy, const int32_t* cell, const uint8_t* keep, int64_t n_rows, int64_t n_cells,
                                          double connectivity, int32_t smoothing, int64_t* ring_offsets, double* xy_out,
                                          int64_t xy_capacity, int32_t* cell_ids, int64_t* n_transcripts, uint64_t* counters,
                                          void* workspace, int64_t workspace_bytes, int32_t lds_max_points, int64_t large_rows,
                                          segger_stream_t stream_) {
  const char* who = "segger_cell_outlines_large";
  hipStream_t stream = (hipStream_t)stream_;
  const CellRingsCall a{xy, cell, keep, n_rows, n_cells, smoothing, ring_offsets, xy_out, xy_capacity, cell_ids, n_transcripts,
                        counters, workspace, workspace_bytes};
  int rc = large_check_sizes(who, n_rows, n_cells, large_rows);
  if (rc != SEGGER_OK) return rc;
  const LargeLayout l = large_layout(n_rows, n_cells, large_rows);
  bool empty = false;
  rc = check_cell_rings_call(who, a, l.total, [&] {
    SEGGER_REQUIRE(connectivity > 0.0 && connectivity - connectivity == 0.0, "%s: connectivity = %g is not a finite number > 0", who,
                   connectivity);
    SEGGER_REQUIRE(lds_max_points >= 0 && lds_max_points <= SEGGER_OUTLINE_MAX_POINTS, "%s: lds_max_points = %d outside 0 .. %d", who,
                   (int)lds_max_points, SEGGER_OUTLINE_MAX_POINTS);
    return SEGGER_OK;
  }, &empty);
  if (rc != SEGGER_OK || empty) return rc;

  const CellRingsViews v = cell_rings_views(a, l.head);
  const BndSegs& s = v.s;
  const LargeLists ll{v.words, at<int32_t>(workspace, l.list_large), at<int64_t>(workspace, l.at_large)};
  const LargeArrays A{at<double2>(workspace, l.pts),   at<uint8_t>(workspace, l.flg),   at<uint32_t>(workspace, l.tv),
                      at<uint32_t>(workspace, l.nb),   at<uint8_t>(workspace, l.ef),    at<uint32_t>(workspace, l.label),
                      at<unsigned long long>(workspace, l.hkey), at<uint32_t>(workspace, l.hid)};
  const OutParams prm{connectivity};
  const int cus = cu_count_or_default();
  const int64_t cap = l.head.cells_cap;
  const int lds_max = (int)lds_max_points;

  rc = launch_cell_rings_front(a, l.head, v, SEGGER_OUTLINE_LARGE_COUNTERS, cus, stream);
  if (rc != SEGGER_OK) return rc;
  hipLaunchKernelGGL(outl_bin_kernel, dim3(grid_stride_blocks(cap, kBndThreads, (int64_t)cus * 8)), dim3(kBndThreads), 0, stream, s, v.cnt,
                     v.list_short, v.list_long, ll, lds_max, large_rows);
  SEGGER_LAUNCH_CHECK("outl_bin_kernel");
  if (lds_max > 0) {
    hipLaunchKernelGGL((outl_lds_kernel<kOutSmall>), dim3(grid_stride_blocks(cap, 1, (int64_t)cus * 9)), dim3(kWave), 0, stream, xy, s,
                       (int)kWordShort, (const int32_t*)v.list_short, prm, lds_max < kOutSmall ? lds_max : kOutSmall, ll, large_rows, v.cnt);
    SEGGER_LAUNCH_CHECK("outl_lds_kernel<256>");
    hipLaunchKernelGGL((outl_lds_kernel<kOutMax>), dim3(grid_stride_blocks(n_rows / (kOutSmall + 1), 1, (int64_t)cus)), dim3(kWave), 0,
                       stream, xy, s, (int)kWordLong, (const int32_t*)v.list_long, prm, lds_max, ll, large_rows, v.cnt);
    SEGGER_LAUNCH_CHECK("outl_lds_kernel<max>");
  }
  if (large_rows > 0) {                            // a cell of the large route has more than lds_max rows
    hipLaunchKernelGGL(outl_large_kernel, dim3(grid_stride_blocks(large_rows / (lds_max + 1), 1, (int64_t)cus * 4)), dim3(kLgThreads), 0,
                       stream, xy, s, ll, A, prm, v.cnt);
    SEGGER_LAUNCH_CHECK("outl_large_kernel");
  }
  return launch_cell_rings_back(a, l.head, v, cus, stream);
}
