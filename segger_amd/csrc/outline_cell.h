// The per-cell concave outline that outlines.hip and outlines_large.hip share (included after cell_rings.h).  The algorithm
// is written once, outline_stages<R>: stages 2 to 6 of outlines.hip's header comment over a ROUTE R, which says how a group
// of threads works on one cell -- the group's size (one wave, or four), the id type with its two marks, where the per-cell
// arrays live, the capacity bounds, and the two operations that differ in kind: the apex search and the directed-edge table.
// Stage 1 (distinct points, sorted) belongs to a route: it leaves d points in r.pts, their multiplicity flags in r.flg, and
// calls outline_stages.  Here too: the predicates and their tie rule, the group-wide reductions, LdsRoute<N> with its
// stage 1 (outline_cell<N>; outlines_large.hip has the route through global memory), and the two kernels both units launch.
// One definition, so a ring has the same bytes whichever route produced it: every stage's result is fixed by the points
// alone, except a component's area, which every route sums in one order (64 partial sums by triangle index mod 64, then the
// butterfly, one wave per component).
#pragma once
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "cell_rings.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kOutMax = SEGGER_OUTLINE_MAX_POINTS;
constexpr int kOutSmall = 256;                                       // rows of a cell on the small route
constexpr int kTooMany = -1, kContradiction = -2;                    // what outline_cell returns instead of a length

enum { kFailed = 8, kFailedCell = 9 };                               // after cell_rings.h's words
static_assert(kFailedCell + 1 == SEGGER_OUTLINE_COUNTERS, "the header documents the block");
static_assert((kOutMax & (kOutMax - 1)) == 0 && kOutMax >= 2048 && 68 * kOutMax <= 160 * 1024, "a power of two that fits the LDS");

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

struct OutParams { double connectivity; };

// ---------------------------------------------------------------- predicates ---
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uniu(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// > 0: c is left of a -> b
__device__ __forceinline__ double orient2d(double2 a, double2 b, double2 c) {
  return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
}

// > 0: d is inside the circle through a, b, c (counter-clockwise)
__device__ __forceinline__ double incircle(double2 a, double2 b, double2 c, double2 d) {
  const double adx = a.x - d.x, ady = a.y - d.y, bdx = b.x - d.x, bdy = b.y - d.y, cdx = c.x - d.x, cdy = c.y - d.y;
  const double al = adx * adx + ady * ady, bl = bdx * bdx + bdy * bdy, cl = cdx * cdx + cdy * cdy;
  return al * (bdx * cdy - bdy * cdx) + bl * (cdx * ady - cdy * adx) + cl * (adx * bdy - ady * bdx);
}

__device__ __forceinline__ bool lex_less(double2 p, double2 q) { return p.x < q.x || (p.x == q.x && p.y < q.y); }

// Is q (at pq) a better apex for the directed edge a -> b than p (at pp)?  Both are strictly left of it (or -1: none).  q
// inside the circle through a, b, p beats p: a total order on the points left of ab.  Points on one circle tie; the tie is
// broken so that every edge of a co-circular polygon chooses the fan from the polygon's lowest vertex m: a candidate below
// min(a, b) wins by index (it is m); otherwise m is a or b and the candidate next to the other endpoint wins.
__device__ __forceinline__ bool apex_better_at(int a, int b, double2 pa, double2 pb, int p, double2 pp, int q, double2 pq) {
  if (q < 0) return false;
  if (p < 0) return true;
  const double ic = incircle(pa, pb, pp, pq);
  if (ic != 0.0) return ic > 0.0;
  const int lo = a < b ? a : b;
  if (p < lo || q < lo) return q < p;
  return a < b ? orient2d(pb, pq, pp) > 0.0 : orient2d(pq, pa, pp) > 0.0;
}

__device__ __forceinline__ bool apex_better(const double2* pts, int a, int b, double2 pa, double2 pb, int p, int q) {
  if (q < 0) return false;
  if (p < 0) return true;
  return apex_better_at(a, b, pa, pb, p, pts[p], q, pts[q]);
}

// The two static predicate bits of the directed edge a -> b of a triangle whose third corner is c: 1 the edge is long;
// 2 it is fairly long and the angle opposite it obtuse, or that angle is nearly flat.
__device__ __forceinline__ uint8_t edge_bits(double2 pa, double2 pb, double2 pc, double t_long, double t_mid, double max_angle) {
  const double dx = pa.x - pb.x, dy = pa.y - pb.y;
  const double len = sqrt(dx * dx + dy * dy);
  const double ux = pa.x - pc.x, uy = pa.y - pc.y, vx = pb.x - pc.x, vy = pb.y - pc.y;
  double cs = (ux * vx + uy * vy) / (sqrt(ux * ux + uy * uy) * sqrt(vx * vx + vy * vy) + 1e-12);
  cs = fmin(fmax(cs, -1.0), 1.0);
  const double angle = acos(cs) * (180.0 / 3.141592653589793);
  return (uint8_t)((len > t_long ? 1 : 0) | (((len > t_mid && angle > 90.0) || angle > max_angle) ? 2 : 0));
}

// Which component is kept: the larger area, then the lower lowest vertex, then the lower root.  (-1.0, 0, -1) is "none yet".
__device__ __forceinline__ bool component_better(double area, int low, int root, double best_area, int best_low, int best_root) {
  return area > best_area || (area == best_area && (low < best_low || (low == best_low && root < best_root)));
}

__device__ __forceinline__ int next_edge(int e) { return e % 3 == 2 ? e - 2 : e + 1; }

// ---------------------------------------------------------------- the group of a route ---
// R::kWaves waves work on a cell.  What they hand each other goes through r.sh, a slot per wave: lane 0 writes, a barrier,
// every thread reads all slots, a barrier (sh is free again).  With one wave none of that exists.  Every reduction returns
// the same value in every thread of the group.
constexpr int kMaxWaves = 4;
struct WaveSlots {
  double f[kMaxWaves];
  double2 p[kMaxWaves];
  int i[kMaxWaves], k[kMaxWaves];
};

// a barrier, then: did any thread of the group change something
template <class R>
__device__ __forceinline__ bool group_any(bool changed) {
  if constexpr (R::kWaves > 1) {
    return __syncthreads_or(changed ? 1 : 0) != 0;
  } else {
    __syncthreads();
    return __ballot(changed) != 0;
  }
}

template <class R>
__device__ __forceinline__ int group_min(const R& r, int v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v = min(v, __shfl_xor(v, m, kWave));
  if constexpr (R::kWaves > 1) {
    static_assert(R::kWaves == 4, "the combine is written out for four waves");
    if ((threadIdx.x & (kWave - 1)) == 0) r.sh.i[threadIdx.x >> 6] = v;
    __syncthreads();
    v = min(min(r.sh.i[0], r.sh.i[1]), min(r.sh.i[2], r.sh.i[3]));
    __syncthreads();
  }
  return uni(v);
}

template <class R>
__device__ __forceinline__ double group_max_f64(const R& r, double v) {
  v = wave_max_f64(v);
  if constexpr (R::kWaves > 1) {
    if ((threadIdx.x & (kWave - 1)) == 0) r.sh.f[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmax(fmax(r.sh.f[0], r.sh.f[1]), fmax(r.sh.f[2], r.sh.f[3]));
    __syncthreads();
  }
  return v;
}

// the index of the least distance, ties to the lower index; -1: no thread had one
template <class R>
__device__ __forceinline__ int group_argmin(const R& r, double bd, int bi) {
  const auto take = [&](double od, int oi) {
    if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
  };
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) take(shfl_xor_f64(bd, m), __shfl_xor(bi, m, kWave));
  if constexpr (R::kWaves > 1) {
    if ((threadIdx.x & (kWave - 1)) == 0) { r.sh.f[threadIdx.x >> 6] = bd; r.sh.i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bd = r.sh.f[0]; bi = r.sh.i[0];
#pragma unroll
    for (int w = 1; w < R::kWaves; ++w) take(r.sh.f[w], r.sh.i[w]);
    __syncthreads();
  }
  return uni(bi);
}

// ---------------------------------------------------------------- one cell, stages 2 to 6 ---
// The outline of a cell whose d >= 3 distinct points lie sorted in r.pts: its vertices to out[0 .. h), h returned in every
// thread; 0: no polygon; kContradiction: refused.  Every `return` is taken by the whole group or by no thread of it: its
// condition is a value every thread holds alike, and where that value was read from memory another wave writes, a barrier
// stands between the read and the write.  Every loop has its trip count fixed before it is entered.
template <class R>
__device__ __forceinline__ int outline_stages(const R& r, int d, double2* out, const OutParams& prm) {
  using Id = typename R::Id;
  constexpr int kThreads = R::kWaves * kWave;
  constexpr uint32_t kNone = R::kNone, kUnset = R::kUnset;           // nb: hull edge, not looked at yet; label: peeled
  // with one wave the mask tells the compiler that the thread's number is a lane's: below 64, never negative
  const int tid = R::kWaves == 1 ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const double2* pts = r.pts;
  Id *tv = r.tv, *nb = r.nb, *label = r.label;
  uint8_t* ef = r.ef;
  unsigned long long* vmin = r.vmin;
  const int max_tris = r.max_tris, max_edges = r.max_edges;

  // ---- 2: Delaunay, edge by edge
  r.clear_table();
  int bi = -1;
  {
    double bd = __longlong_as_double(0x7ff0000000000000ll);
    const double2 p0 = pts[0];
    for (int i = 1 + tid; i < d; i += kThreads) {                    // ascending: a thread's ties keep the lower index
      const double dx = pts[i].x - p0.x, dy = pts[i].y - p0.y, dd = dx * dx + dy * dy;
      if (dd < bd) { bd = dd; bi = i; }
    }
    bi = group_argmin(r, bd, bi);
  }
  __syncthreads();                                                   // the table is empty
  int sa = 0, sb = bi;
  int sc = r.find_apex(d, sa, sb);
  if (sc < 0) { sa = bi; sb = 0; sc = r.find_apex(d, sa, sb); }
  if (sc < 0) return 0;                                              // nothing on either side of a Delaunay edge: collinear
  if (tid == 0) {
    tv[0] = (Id)sa; tv[1] = (Id)sb; tv[2] = (Id)sc;
    nb[0] = (Id)kUnset; nb[1] = (Id)kUnset; nb[2] = (Id)kUnset;
  }
  int T = 1;
  __syncthreads();
  if (r.hash_edge(sa, sb, 0) == kContradiction) return kContradiction;
  __syncthreads();
  if (r.hash_edge(sb, sc, 1) == kContradiction) return kContradiction;
  __syncthreads();
  if (r.hash_edge(sc, sa, 2) == kContradiction) return kContradiction;
  __syncthreads();
  for (int e = 0; e < max_edges; ++e) {                              // the triangle list is the queue: T grows under e
    if (e >= 3 * T) break;
    const uint32_t twin = nb[e], va = tv[e], vb = tv[next_edge(e)];   // one round trip for the three
    if (uniu(twin) != kUnset) continue;
    const int a = (int)uniu(va), b = (int)uniu(vb);                  // e is a -> b; its twin b -> a
    const int f = r.hash_edge(b, a, -1);
    if (f == kContradiction) return kContradiction;
    if (f >= 0) {
      if (uniu(nb[f]) != kUnset) return kContradiction;
      if constexpr (R::kWaves > 1) __syncthreads();                  // every wave has read nb[e] and nb[f]: all return, or none
      if (tid == 0) { nb[e] = (Id)f; nb[f] = (Id)e; }
      __syncthreads();
      continue;
    }
    const int c = r.find_apex(d, b, a);
    if (c < 0) {
      if (tid == 0) nb[e] = (Id)kNone;
      __syncthreads();
      continue;
    }
    if (T >= max_tris) return kContradiction;                        // more than 2 n - 5 triangles: not a triangulation
    const int g = 3 * T;
    ++T;
    if (tid == 0) {
      tv[g] = (Id)b; tv[g + 1] = (Id)a; tv[g + 2] = (Id)c;
      nb[g] = (Id)e; nb[e] = (Id)g; nb[g + 1] = (Id)kUnset; nb[g + 2] = (Id)kUnset;
    }
    // All three edges go into the table, b -> a too: a later edge that asks for it finds a twin already taken.  No lookup
    // reads triangle g before the barrier after the first insert: the table does not name it until then.
    if (r.hash_edge(b, a, g) == kContradiction) return kContradiction;
    __syncthreads();
    if (r.hash_edge(a, c, g + 1) == kContradiction) return kContradiction;
    __syncthreads();
    if (r.hash_edge(c, b, g + 2) == kContradiction) return kContradiction;
    __syncthreads();
  }
  if (uniu(nb[3 * T - 1]) == kUnset) return kContradiction;          // the bound ended the loop, not the queue
  const int E = 3 * T;

  // ---- 3: d_max, the largest nearest-neighbour distance; the table is dead, its region holds the per-vertex minima
  __syncthreads();
  for (int v = tid; v < d; v += kThreads) vmin[v] = 0x7ff0000000000000ull;
  __syncthreads();
  for (int e = tid; e < E; e += kThreads) {
    const int a = (int)tv[e], b = (int)tv[next_edge(e)];
    const double dx = pts[a].x - pts[b].x, dy = pts[a].y - pts[b].y;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(dx * dx + dy * dy);   // >= 0: ordered as integers
    atomicMin(&vmin[a], bits);
    atomicMin(&vmin[b], bits);
  }
  __syncthreads();
  double d_max = 0.0;
  for (int v = tid; v < d; v += kThreads) d_max = fmax(d_max, r.flg[v] ? 0.0 : sqrt(__longlong_as_double((long long)vmin[v])));
  d_max = group_max_f64(r, d_max);

  // ---- 4: the static predicates of every directed edge, then the two peels
  const double t_long = (2.0 * prm.connectivity) * d_max, t_mid = (1.5 * prm.connectivity) * d_max;
  const double max_angle = 180.0 - 11.25 / prm.connectivity;
  for (int e = tid; e < E; e += kThreads) {
    const int e1 = next_edge(e), e2 = next_edge(e1);
    ef[e] = edge_bits(pts[tv[e]], pts[tv[e1]], pts[tv[e2]], t_long, t_mid, max_angle);
  }
  for (int t = tid; t < T; t += kThreads) label[t] = (Id)t;
  __syncthreads();
  for (int phase = 1; phase <= 2; ++phase) {
    for (int round = 0; round < T; ++round) {                        // a round without a removal is the fixed point
      bool changed = false;
      for (int t = tid; t < T; t += kThreads) {
        if (label[t] == kNone) continue;
        for (int k = 0; k < 3; ++k) {
          const int e = 3 * t + k;
          if (!(ef[e] & phase)) continue;
          const uint32_t o = nb[e];
          if (o == kNone || label[o / 3] == kNone) { label[t] = (Id)kNone; changed = true; break; }
        }
      }
      if (!group_any<R>(changed)) break;
    }
  }

  // ---- 5: components over shared edges, the largest by area
  for (int round = 0; round < T; ++round) {
    bool changed = false;
    for (int t = tid; t < T; t += kThreads) {
      const uint32_t mine = label[t];
      if (mine == kNone) continue;
      uint32_t m = mine;
      for (int k = 0; k < 3; ++k) {
        const uint32_t o = nb[3 * t + k];
        if (o != kNone) { const uint32_t l2 = label[o / 3]; if (l2 < m) m = l2; }      // kNone is the largest value
      }
      const uint32_t l3 = label[m];
      if (l3 < m) m = l3;
      if (m < mine) { label[t] = (Id)m; changed = true; }
    }
    if (!group_any<R>(changed)) break;
  }
  // Wave w takes the roots of the 64-triangle chunks w, w + kWaves, ...  A root's sum runs in one order on every route: per
  // lane the members u = lane (mod 64) ascending, from the root's chunk (a member is never below its root), then the butterfly.
  int best_root = -1, best_low = 0;
  double best_area = -1.0;
  for (int base = wave * kWave; base < T; base += kThreads) {
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
      if (component_better(area2, low, root, best_area, best_low, best_root)) { best_area = area2; best_low = low; best_root = root; }
    }
  }
  if constexpr (R::kWaves > 1) {
    if (lane == 0) { r.sh.f[wave] = best_area; r.sh.i[wave] = best_root; r.sh.k[wave] = best_low; }
    __syncthreads();
    best_root = -1; best_low = 0; best_area = -1.0;
#pragma unroll
    for (int w = 0; w < R::kWaves; ++w) {                            // a wave without a root left "none yet": it never wins
      const double ar = r.sh.f[w];
      const int ro = r.sh.i[w], lw = r.sh.k[w];
      if (component_better(ar, lw, ro, best_area, best_low, best_root)) { best_area = ar; best_low = lw; best_root = ro; }
    }
    best_root = uni(best_root);
    best_low = uni(best_low);
    __syncthreads();
  }
  if (best_root < 0) return 0;                                       // everything was peeled

  // ---- 6: the ring, interior on the left, from the component's lowest vertex
  int e0 = max_edges;
  for (int e = tid; e < E; e += kThreads) {
    if (label[e / 3] != (uint32_t)best_root || tv[e] != (uint32_t)best_low) continue;
    const uint32_t o = nb[e];
    if (o == kNone || label[o / 3] == kNone) e0 = min(e0, e);
  }
  e0 = group_min(r, e0);
  if (e0 >= E) return kContradiction;
  int h = 0, x = e0;
  bool closed = false;
  for (int it = 0; it < E; ++it) {                                   // every step consumes one directed edge of the component
    const uint32_t o = uniu(nb[x]);
    if (o == kNone || uniu(label[o / 3]) == kNone) {
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

// ---------------------------------------------------------------- the LDS route ---
// One wave, the cell's state in LDS (outlines.hip's header has the map), 16-bit ids, at most N distinct points.
template <int N>
struct LdsRoute {
  using Id = uint16_t;
  static constexpr int kWaves = 1;
  static constexpr Id kNone = 0xffff, kUnset = 0xfffe;               // also the table's empty slot
  static constexpr int kStage = 2 * N, max_tris = 2 * N, max_edges = 3 * max_tris, kSlots = 8 * N, kSlotBits = ilog2(kSlots);
  static constexpr int oPts = 0, oU = 16 * N, oTv = 32 * N, oNb = 44 * N, oEf = 56 * N, oLabel = 62 * N, oFlg = 66 * N;
  static constexpr int kBytes = 68 * N;
  static_assert(max_edges < kUnset, "directed edge ids and the two marks share uint16");

  double2* pts;
  uint16_t* hash;
  unsigned long long* vmin;
  Id *tv, *nb;
  uint8_t* ef;
  Id* label;
  uint8_t* flg;

  __device__ __forceinline__ explicit LdsRoute(unsigned char* lds)
      : pts(reinterpret_cast<double2*>(lds + oPts)), hash(reinterpret_cast<uint16_t*>(lds + oU)),
        vmin(reinterpret_cast<unsigned long long*>(lds + oU)), tv(reinterpret_cast<Id*>(lds + oTv)),
        nb(reinterpret_cast<Id*>(lds + oNb)), ef(lds + oEf), label(reinterpret_cast<Id*>(lds + oLabel)), flg(lds + oFlg) {}

  __device__ __forceinline__ void clear_table() const {
    for (int k = threadIdx.x & (kWave - 1); k < kSlots; k += kWave) hash[k] = kNone;
  }

  // the apex of a -> b among the d points, -1 when nothing is left of it; the same in every lane
  __device__ __forceinline__ int find_apex(int d, int a, int b) const {
    const int lane = threadIdx.x & (kWave - 1);
    const double2 pa = pts[a], pb = pts[b];
    int best = -1;
    for (int base = 0; base < d; base += kWave) {
      const int i = base + lane;
      if (i < d && i != a && i != b && orient2d(pa, pb, pts[i]) > 0.0 && apex_better(pts, a, b, pa, pb, best, i)) best = i;
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      const int o = __shfl_xor(best, m, kWave);
      if (apex_better(pts, a, b, pa, pb, best, o)) best = o;
    }
    return uni(best);
  }

  // the id of directed edge a -> b, -1 if it has no triangle yet; with `id` >= 0: insert it (kContradiction if it is there)
  __device__ __forceinline__ int hash_edge(int a, int b, int id) const {
    int slot = (int)(((((uint32_t)a << 16) | (uint32_t)b) * 2654435761u) >> (32 - kSlotBits));
    for (int probe = 0; probe < kSlots; ++probe) {
      const int f = uni(hash[slot]);
      if (f == kNone) {
        if (id >= 0 && (threadIdx.x & (kWave - 1)) == 0) hash[slot] = (uint16_t)id;
        return -1;
      }
      if (uni(tv[f]) == a && uni(tv[next_edge(f)]) == b) return id >= 0 ? kContradiction : f;
      slot = (slot + 1) & (kSlots - 1);
    }
    return kContradiction;                                           // a full table: more edges than a triangulation has
  }
};

// The outline of segment j: its vertices to out[0 .. h), h returned; 0: no polygon; kContradiction: refused; kTooMany:
// more than `limit` <= N distinct points (nothing was written for the cell).  Stage 1 here: the rows are staged into LDS
// round after round, each round sorted (bitonic) behind the distinct points so far and squeezed, the multiplicity flags
// carried through the sort.
template <int N>
__device__ __forceinline__ int outline_cell(const double* __restrict__ xy, const BndSegs& s, int j, unsigned char* lds,
                                            const OutParams& prm, int limit) {
  using L = LdsRoute<N>;
  const L r(lds);
  double2* pts = r.pts;
  uint8_t* flg = r.flg;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b0 = s.head[j];
  const int n = uni(s.len[j]);
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  int d = 0, consumed = 0;
  const int rounds = n / N + 1;                                      // every round but the last stages at least N new rows
  for (int rd = 0; rd < rounds && consumed < n; ++rd) {
    const int take = min(L::kStage - d, n - consumed);
    const int m = d + take;
    int P = kWave;
    for (int q = 0; q < 16 && P < m; ++q) P <<= 1;                   // m <= 2 N, a power of two
    __syncthreads();
    for (int k = lane; k < take; k += kWave) {
      const P2 p = point_at(xy, s.keys, b0 + consumed + k);
      pts[d + k] = double2{p.x, p.y};
      flg[d + k] = 0;
    }
    for (int k = m + lane; k < P; k += kWave) { pts[k] = double2{inf, inf}; flg[k] = 0; }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {                               // bitonic: log2(P) (log2(P) + 1) / 2 passes
      for (int jj = k >> 1; jj > 0; jj >>= 1) {
        for (int i = lane; i < (P >> 1); i += kWave) {
          const int lo = ((i & ~(jj - 1)) << 1) | (i & (jj - 1)), hi = lo | jj;
          const double2 a = pts[lo], b = pts[hi];
          if ((lo & k) == 0 ? lex_less(b, a) : lex_less(a, b)) {
            const uint8_t fa = flg[lo], fb = flg[hi];
            pts[lo] = b; pts[hi] = a;
            flg[lo] = fb; flg[hi] = fa;
          }
        }
        __syncthreads();
      }
    }
    int kept = 0;                                                    // in place: an element never moves to a higher index
    for (int base = 0; base < m; base += kWave) {
      const int i = base + lane;
      const bool in = i < m;
      const double2 p = in ? pts[i] : double2{0.0, 0.0};
      bool first = false, again = false;
      uint8_t f = 0;
      if (in) {
        f = flg[i];
        const double2 before = pts[i > 0 ? i - 1 : 0];
        first = i == 0 || before.x != p.x || before.y != p.y;
        if (i + 1 < m) { const double2 after = pts[i + 1]; again = after.x == p.x && after.y == p.y; }
      }
      const unsigned long long mask = __ballot(first);
      const int pos = kept + (int)__popcll(mask & ((1ull << lane) - 1));
      __syncthreads();
      if (first) { pts[pos] = p; flg[pos] = (again || f) ? 1 : 0; }
      kept += (int)__popcll(mask);
      __syncthreads();
    }
    d = kept;
    consumed += take;
    if (d > limit) return kTooMany;
  }
  if (d < 3) return 0;
  return outline_stages(r, d, s.hull + b0, prm);
}

// ---------------------------------------------------------------- the kernels of the LDS routes ---
// `too_many` is what a cell with more distinct points than an LDS route takes gets, the one switch between the two units:
//   every_cell()               true: no cell takes an LDS route, the binning kernel hands every present cell over;
//   limit(N)                   the distinct points an instance of capacity N takes, <= N;
//   (s, j, n, counters)        one thread hands over segment j of n rows; hull_n[j] is no longer this kernel's.
__device__ __forceinline__ void refuse_cell(const BndSegs& s, int j, unsigned long long* __restrict__ counters) {
  atomicAdd(counters + kRefused, 1ull);
  atomicMax(counters + kRefusedCell, (s.keys[s.head[j]] >> 32) + 1ull);
  s.hull_n[j] = 0;
}

// one thread per present cell: its length and its route (rings.h: append_by_route)
template <class TooMany>
__global__ __launch_bounds__(kBndThreads) void out_bin_kernel(BndSegs s, unsigned long long* __restrict__ counters,
                                                              int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                              int32_t* __restrict__ list_long, TooMany too_many) {
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
      route = too_many.every_cell() ? 2 : n > kOutSmall;
    }
    append_by_route(route, j, words, list_short, list_long);
    if (route == 2) too_many(s, (int)j, n, counters);
  }
}

// one single-wave workgroup per listed cell, capacity N
template <int N, class TooMany>
__global__ __launch_bounds__(kWave) void out_cell_kernel(const double* __restrict__ xy, BndSegs s, const int32_t* __restrict__ words,
                                                         int word, const int32_t* __restrict__ list, OutParams prm, TooMany too_many,
                                                         unsigned long long* __restrict__ counters) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LdsRoute<N>::kBytes];
  const int count = words[word];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) {
    const int j = list[w];
    __syncthreads();                                                 // the previous cell's readers are done
    int h = outline_cell<N>(xy, s, j, lds, prm, too_many.limit(N));
    if (h == kTooMany) {
      if (threadIdx.x == 0) too_many(s, j, s.len[j], counters);
      continue;
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

// what both entry points require of the one parameter
inline int check_connectivity(const char* who, double connectivity) {
  SEGGER_REQUIRE(connectivity > 0.0 && connectivity - connectivity == 0.0, "%s: connectivity = %g is not a finite number > 0", who,
                 connectivity);
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger
