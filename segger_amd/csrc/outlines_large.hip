// segger_cell_outlines_large: segger_cell_outlines with a third route, through global memory, for the cells whose distinct
// points exceed the LDS budget (or a caller's lower `lds_max_points`).  include/segger_amd.h has the contract.
//
// The front end, the back end and the host code that drives them are cell_rings.h's; the binning kernel, the kernel of the
// two LDS routes and the per-cell algorithm (outline_stages<R>: stages 2 to 6 over a route R) are outline_cell.h's, all
// shared with outlines.hip.  This unit's own part:
//   TakeLarge            what a cell gets that an LDS route does not take (more than min(N, lds_max_points) distinct points
//                        in stage 1; every present cell when lds_max_points = 0): a slice of the large-cell workspace by one
//                        atomic bump of its rows and a place in the large list; when the slices would exceed large_rows it
//                        is refused through the counters instead;
//   outl_large_kernel    one 256-thread WORKGROUP per listed cell: outline_stages over LargeRoute -- four waves, the cell's
//                        state in its slice, 32-bit ids -- after this route's stage 1.
// What the route does in its own way:
//   1 the rows are copied to the slice and sorted there by a bitonic network over the next power of two in which an index
//     past the rows counts as +inf and is never touched (every comparator orders ascending, so such an element never
//     moves); duplicates are squeezed out in place, 256 at a time;
//   2 the apex search uses all four waves and is pruned: the points are sorted by x, and a better apex lies inside or on the
//     circle through a, b and the best so far, so each wave walks outward from the edge, 32 points to the left and 32 to the
//     right per step, and stops when a step finds nothing inside the circle's x-extent.  The extent comes from a
//     circumcentre whose rounding error is bounded term by term and added (circle_x_extent): it is never too narrow, so a
//     point ON the circle is still seen and the tie rule still decides; an edge with nothing on its left scans all d.  The
//     directed-edge table is open addressing over 8 d slots of (key, id); a wave reads 64 consecutive slots at once.
// The work per triangle is a chain of dependent reads of the slice (L2 latency), not arithmetic: see README for the
// measured cost per cell.
//
// Workspace per large-cell row, bytes (175): 16 points, 1 multiplicity flag, 24 triangle vertices (3 uint32 x 2 triangles),
// 24 twins, 6 predicate bits, 8 labels, 64 + 32 hash keys and ids (8 slots; the keys' region later holds the per-vertex
// minima).  A cell of more than 2^28 rows is refused: directed-edge ids and slot numbers are 32-bit.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel of the unit, the library's
// included; outl_large_kernel two waves per SIMD, 384 B of LDS; out_cell_kernel<256> 17408 B and out_cell_kernel<2048> 139264 B of LDS.
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
constexpr unsigned long long kEmptyKey = ~0ull, kNoKey = ~0ull - 1;  // an empty slot; what a lane past the table reads
constexpr int kLgMaxRows = 1 << 28;                                  // 6 d edge ids and 8 d slots stay below 2^31
constexpr int kWordLarge = 3, kWordBump = 4;                         // words: the large list's length; int64 rows taken
enum { kLargeCells = 10, kLargePoints = 11, kLargeRows = 12 };       // after outline_cell.h's words
static_assert(kLargeRows + 1 == SEGGER_OUTLINE_LARGE_COUNTERS, "the header documents the block");
static_assert(kLgWaves == kMaxWaves && (kWordBump + 2) * sizeof(int32_t) <= kRingWordsBytes && kWordBump % 2 == 0, "the words' region");

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
    refuse_cell(s, j, counters);
    return;
  }
  const int pos = atomicAdd(&ll.words[kWordLarge], 1);
  ll.list[pos] = j;
  ll.at[pos] = (int64_t)at;
  atomicAdd(counters + kLargeRows, (unsigned long long)n);
}

// what out_bin_kernel and out_cell_kernel<N> (outline_cell.h) do with a cell that the LDS routes do not take
struct TakeLarge {
  LargeLists ll;
  int lds_max;
  int64_t large_rows;
  __device__ __forceinline__ bool every_cell() const { return lds_max == 0; }
  __device__ __forceinline__ int limit(int n) const { return min(n, lds_max); }
  __device__ __forceinline__ void operator()(const BndSegs& s, int j, int n, unsigned long long* counters) const {
    take_large(s, j, n, ll, large_rows, counters);
  }
};

// ---------------------------------------------------------------- the large cell: workgroup helpers ---
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
__device__ __forceinline__ int find_apex_large(const double2* __restrict__ pts, int d, int a, int b, WaveSlots& sh) {
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
// different returns; the LDS route has one wave and needs neither barrier.)
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
// The route of outline_stages: four waves, the cell's state in its slice of the workspace, 32-bit ids.
struct LargeRoute {
  using Id = uint32_t;
  static constexpr int kWaves = kLgWaves;
  static constexpr Id kNone = 0xffffffffu, kUnset = 0xfffffffeu;
  double2* pts;
  uint8_t* flg;
  Id *tv, *nb;
  uint8_t* ef;
  Id* label;
  unsigned long long *vmin, *hkey;                                   // one region: the minima once the table is dead
  uint32_t* hid;
  uint32_t slots;
  int max_tris, max_edges;
  WaveSlots& sh;
  __device__ __forceinline__ void clear_table() const {
    for (uint32_t k = threadIdx.x; k < slots; k += kLgThreads) hkey[k] = kEmptyKey;
  }
  __device__ __forceinline__ int find_apex(int d, int a, int b) const { return find_apex_large(pts, d, a, b, sh); }
  __device__ __forceinline__ int hash_edge(int a, int b, int id) const { return hash_edge_large(hkey, hid, slots, a, b, id); }
};

// The outline of segment j in its slice: its vertices to out[0 .. h), h returned in every thread; 0: no polygon;
// kContradiction: refused.  d_out: its distinct points.
__device__ __forceinline__ int outline_large(const double* __restrict__ xy, const BndSegs& s, int j, const LargeArrays& A, int64_t at0,
                                             const OutParams& prm, WaveSlots& sh, int& d_out) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  double2* pts = A.pts + at0;
  uint8_t* flg = A.flg + at0;
  unsigned long long* hkey = A.hkey + 8 * at0;
  const int64_t b0 = s.head[j];
  const int n = uni(s.len[j]);
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

  const LargeRoute r{pts, flg, A.tv + 6 * at0, A.nb + 6 * at0, A.ef + 6 * at0, A.label + 2 * at0, hkey, hkey, A.hid + 8 * at0,
                     8u * (uint32_t)d, 2 * d, 6 * d, sh};
  return outline_stages(r, d, s.hull + b0, prm);
}

__global__ __launch_bounds__(kLgThreads) void outl_large_kernel(const double* __restrict__ xy, BndSegs s, LargeLists ll, LargeArrays A,
                                                                OutParams prm, unsigned long long* __restrict__ counters) {
  __shared__ WaveSlots sh;
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
  rc = check_cell_rings_call(who, a, l.total, [&]() -> int {
    const int rc_k = check_connectivity(who, connectivity);
    if (rc_k != SEGGER_OK) return rc_k;
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
  const TakeLarge take{ll, lds_max, large_rows};

  rc = launch_cell_rings_front(a, l.head, v, SEGGER_OUTLINE_LARGE_COUNTERS, cus, stream);
  if (rc != SEGGER_OK) return rc;
  hipLaunchKernelGGL(out_bin_kernel<TakeLarge>, dim3(grid_stride_blocks(cap, kBndThreads, (int64_t)cus * 8)), dim3(kBndThreads), 0, stream,
                     s, v.cnt, v.words, v.list_short, v.list_long, take);
  SEGGER_LAUNCH_CHECK("out_bin_kernel");
  if (lds_max > 0) {
    hipLaunchKernelGGL((out_cell_kernel<kOutSmall, TakeLarge>), dim3(grid_stride_blocks(cap, 1, (int64_t)cus * 9)), dim3(kWave), 0, stream,
                       xy, s, (const int32_t*)v.words, (int)kWordShort, (const int32_t*)v.list_short, prm, take, v.cnt);
    SEGGER_LAUNCH_CHECK("out_cell_kernel<256>");
    hipLaunchKernelGGL((out_cell_kernel<kOutMax, TakeLarge>), dim3(grid_stride_blocks(n_rows / (kOutSmall + 1), 1, (int64_t)cus)),
                       dim3(kWave), 0, stream, xy, s, (const int32_t*)v.words, (int)kWordLong, (const int32_t*)v.list_long, prm, take, v.cnt);
    SEGGER_LAUNCH_CHECK("out_cell_kernel<max>");
  }
  if (large_rows > 0) {                            // a cell of the large route has more than lds_max rows
    hipLaunchKernelGGL(outl_large_kernel, dim3(grid_stride_blocks(large_rows / (lds_max + 1), 1, (int64_t)cus * 4)), dim3(kLgThreads), 0,
                       stream, xy, s, ll, A, prm, v.cnt);
    SEGGER_LAUNCH_CHECK("outl_large_kernel");
  }
  return launch_cell_rings_back(a, l.head, v, cus, stream);
}
