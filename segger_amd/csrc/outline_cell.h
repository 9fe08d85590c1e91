// The per-cell outline in LDS that outlines.hip and outlines_large.hip share (included after cell_rings.h): the predicates
// and their tie rule, and outline_cell<N>, one single-wave workgroup's six stages over a cell of at most N distinct
// points.  outlines.hip's header comment describes the stages and the LDS map; both units run this one definition, and
// outlines_large.hip's workgroup-wide route through global memory uses the same predicates on the same expressions, so a
// ring has the same bytes whichever route produced it.
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
constexpr uint16_t kNone = 0xffff;                                   // nb: hull edge; hash: empty slot; label: peeled
constexpr uint16_t kUnset = 0xfffe;                                  // nb: not looked at yet
constexpr int kTooMany = -1, kContradiction = -2;                    // what outline_cell returns instead of a length

enum { kFailed = 8, kFailedCell = 9 };                               // after cell_rings.h's words
static_assert(kFailedCell + 1 == SEGGER_OUTLINE_COUNTERS, "the header documents the block");
static_assert((kOutMax & (kOutMax - 1)) == 0 && kOutMax >= 2048 && 68 * kOutMax <= 160 * 1024, "a power of two that fits the LDS");

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

template <int N>
struct OutLds {
  static constexpr int kStage = 2 * N, kTris = 2 * N, kEdges = 3 * kTris, kSlots = 8 * N, kSlotBits = ilog2(kSlots);
  static constexpr int oPts = 0, oU = 16 * N, oTv = 32 * N, oNb = 44 * N, oEf = 56 * N, oLabel = 62 * N, oFlg = 66 * N;
  static constexpr int kBytes = 68 * N;
  static_assert(kEdges < kUnset, "directed edge ids and the two marks share uint16");
};

struct OutParams { double connectivity; };

// ---------------------------------------------------------------- predicates ---
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

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

// the apex of a -> b among the d points, -1 when nothing is left of it; the same in every lane
__device__ __forceinline__ int find_apex(const double2* pts, int d, int a, int b) {
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

// ---------------------------------------------------------------- one cell ---
__device__ __forceinline__ int next_edge(int e) { return e % 3 == 2 ? e - 2 : e + 1; }

template <int N>
__device__ __forceinline__ int hash_slot(int a, int b) {
  return (int)(((((uint32_t)a << 16) | (uint32_t)b) * 2654435761u) >> (32 - OutLds<N>::kSlotBits));
}

// the id of directed edge a -> b, -1 if it has no triangle yet; with `id` >= 0: insert it (kContradiction if it is there)
template <int N>
__device__ __forceinline__ int hash_edge(uint16_t* hash, const uint16_t* tv, int a, int b, int id) {
  constexpr int kSlots = OutLds<N>::kSlots;
  int slot = hash_slot<N>(a, b);
  for (int probe = 0; probe < kSlots; ++probe) {
    const int f = uni(hash[slot]);
    if (f == kNone) {
      if (id >= 0 && (threadIdx.x & (kWave - 1)) == 0) hash[slot] = (uint16_t)id;
      return -1;
    }
    if (uni(tv[f]) == a && uni(tv[next_edge(f)]) == b) return id >= 0 ? kContradiction : f;
    slot = (slot + 1) & (kSlots - 1);
  }
  return kContradiction;                                             // a full table: more edges than a triangulation has
}

// The outline of segment j: its vertices to out[0 .. h), h returned; 0: no polygon; kContradiction: refused; kTooMany:
// more than `limit` <= N distinct points (nothing was written for the cell).
template <int N>
__device__ __forceinline__ int outline_cell(const double* __restrict__ xy, const BndSegs& s, int j, unsigned char* lds,
                                            const OutParams& prm, int limit) {
  using L = OutLds<N>;
  double2* pts = reinterpret_cast<double2*>(lds + L::oPts);
  uint16_t* hash = reinterpret_cast<uint16_t*>(lds + L::oU);
  unsigned long long* vmin = reinterpret_cast<unsigned long long*>(lds + L::oU);
  uint16_t* tv = reinterpret_cast<uint16_t*>(lds + L::oTv);
  uint16_t* nb = reinterpret_cast<uint16_t*>(lds + L::oNb);
  uint8_t* ef = lds + L::oEf;
  uint16_t* label = reinterpret_cast<uint16_t*>(lds + L::oLabel);
  uint8_t* flg = lds + L::oFlg;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b0 = s.head[j];
  const int n = uni(s.len[j]);
  double2* out = s.hull + b0;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  // ---- 1: distinct points, sorted by (x, y)
  int d = 0, consumed = 0;
  const int rounds = n / N + 1;                                      // every round but the last stages at least N new rows
  for (int r = 0; r < rounds && consumed < n; ++r) {
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

  // ---- 2: Delaunay, edge by edge
  for (int k = lane; k < L::kSlots; k += kWave) hash[k] = kNone;
  double bd = inf;
  int bi = -1;
  {
    const double2 p0 = pts[0];
    for (int i = 1 + lane; i < d; i += kWave) {                      // ascending: a lane's ties keep the lower index
      const double dx = pts[i].x - p0.x, dy = pts[i].y - p0.y, dd = dx * dx + dy * dy;
      if (dd < bd) { bd = dd; bi = i; }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      const double od = shfl_xor_f64(bd, m);
      const int oi = __shfl_xor(bi, m, kWave);
      if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
    }
    bi = uni(bi);
  }
  __syncthreads();
  int sa = 0, sb = bi;
  int sc = find_apex(pts, d, sa, sb);
  if (sc < 0) { sa = bi; sb = 0; sc = find_apex(pts, d, sa, sb); }
  if (sc < 0) return 0;                                              // nothing on either side of a Delaunay edge: collinear
  if (lane == 0) {
    tv[0] = (uint16_t)sa; tv[1] = (uint16_t)sb; tv[2] = (uint16_t)sc;
    nb[0] = kUnset; nb[1] = kUnset; nb[2] = kUnset;
  }
  int T = 1;
  __syncthreads();
  for (int k = 0; k < 3; ++k) {
    if (hash_edge<N>(hash, tv, uni(tv[k]), uni(tv[next_edge(k)]), k) == kContradiction) return kContradiction;
    __syncthreads();
  }
  for (int e = 0; e < L::kEdges; ++e) {                              // the triangle list is the queue: T grows under e
    if (e >= 3 * T) break;
    if (uni(nb[e]) != kUnset) continue;
    const int a = uni(tv[e]), b = uni(tv[next_edge(e)]);             // e is a -> b; its twin b -> a
    const int f = hash_edge<N>(hash, tv, b, a, -1);
    if (f == kContradiction) return kContradiction;
    if (f >= 0) {
      if (uni(nb[f]) != kUnset) return kContradiction;
      if (lane == 0) { nb[e] = (uint16_t)f; nb[f] = (uint16_t)e; }
      __syncthreads();
      continue;
    }
    const int c = find_apex(pts, d, b, a);
    if (c < 0) {
      if (lane == 0) nb[e] = kNone;
      __syncthreads();
      continue;
    }
    if (T >= L::kTris) return kContradiction;                        // more than 2 n - 5 triangles: not a triangulation
    const int g = 3 * T;
    ++T;
    if (lane == 0) {
      tv[g] = (uint16_t)b; tv[g + 1] = (uint16_t)a; tv[g + 2] = (uint16_t)c;
      nb[g] = (uint16_t)e; nb[e] = (uint16_t)g; nb[g + 1] = kUnset; nb[g + 2] = kUnset;
    }
    __syncthreads();
    // all three edges go into the table, b -> a too: a later edge that asks for it finds a twin already taken
    if (hash_edge<N>(hash, tv, b, a, g) == kContradiction) return kContradiction;
    __syncthreads();
    if (hash_edge<N>(hash, tv, a, c, g + 1) == kContradiction) return kContradiction;
    __syncthreads();
    if (hash_edge<N>(hash, tv, c, b, g + 2) == kContradiction) return kContradiction;
    __syncthreads();
  }
  if (uni(nb[3 * T - 1]) == kUnset) return kContradiction;           // the bound ended the loop, not the queue
  const int E = 3 * T;

  // ---- 3: d_max, the largest nearest-neighbour distance; the hash is dead, its region holds the per-vertex minima
  __syncthreads();
  for (int v = lane; v < d; v += kWave) vmin[v] = 0x7ff0000000000000ull;
  __syncthreads();
  for (int e = lane; e < E; e += kWave) {
    const int a = tv[e], b = tv[next_edge(e)];
    const double dx = pts[a].x - pts[b].x, dy = pts[a].y - pts[b].y;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(dx * dx + dy * dy);   // >= 0: ordered as integers
    atomicMin(&vmin[a], bits);
    atomicMin(&vmin[b], bits);
  }
  __syncthreads();
  double d_max = 0.0;
  for (int v = lane; v < d; v += kWave) d_max = fmax(d_max, flg[v] ? 0.0 : sqrt(__longlong_as_double((long long)vmin[v])));
  d_max = wave_max_f64(d_max);

  // ---- 4: the static predicates of every directed edge, then the two peels
  const double t_long = (2.0 * prm.connectivity) * d_max, t_mid = (1.5 * prm.connectivity) * d_max;
  const double max_angle = 180.0 - 11.25 / prm.connectivity;
  for (int e = lane; e < E; e += kWave) {
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
  for (int t = lane; t < T; t += kWave) label[t] = (uint16_t)t;
  __syncthreads();
  for (int phase = 1; phase <= 2; ++phase) {
    for (int round = 0; round < T; ++round) {                        // a round without a removal is the fixed point
      bool changed = false;
      for (int t = lane; t < T; t += kWave) {
        if (label[t] == kNone) continue;
        for (int k = 0; k < 3; ++k) {
          const int e = 3 * t + k;
          if (!(ef[e] & phase)) continue;
          const int o = nb[e];
          if (o == kNone || label[o / 3] == kNone) { label[t] = kNone; changed = true; break; }
        }
      }
      __syncthreads();
      if (__ballot(changed) == 0) break;
    }
  }

  // ---- 5: components over shared edges, the largest by area
  for (int round = 0; round < T; ++round) {
    bool changed = false;
    for (int t = lane; t < T; t += kWave) {
      const int mine = label[t];
      if (mine == kNone) continue;
      int m = mine;
      for (int k = 0; k < 3; ++k) {
        const int o = nb[3 * t + k];
        if (o != kNone) { const int l2 = label[o / 3]; if (l2 < m) m = l2; }      // kNone is the largest value
      }
      const int l3 = label[m];
      if (l3 < m) m = l3;
      if (m < mine) { label[t] = (uint16_t)m; changed = true; }
    }
    __syncthreads();
    if (__ballot(changed) == 0) break;
  }
  int best_root = -1, best_low = 0;
  double best_area = -1.0;
  for (int base = 0; base < T; base += kWave) {
    const int t = base + lane;
    unsigned long long roots = __ballot(t < T && label[t] == t);
    const int n_roots = (int)__popcll(roots);
    for (int q = 0; q < n_roots; ++q) {
      const int root = base + (int)__builtin_ctzll(roots);
      roots &= roots - 1;
      double area2 = 0.0;
      int low = N;
      for (int u = lane; u < T; u += kWave) {
        if (label[u] != root) continue;
        const int va = tv[3 * u], vb = tv[3 * u + 1], vc = tv[3 * u + 2];
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
  if (best_root < 0) return 0;                                       // everything was peeled

  // ---- 6: the ring, interior on the left, from the component's lowest vertex
  int e0 = L::kEdges;
  for (int e = lane; e < E; e += kWave) {
    if (label[e / 3] != best_root || tv[e] != best_low) continue;
    const int o = nb[e];
    if (o == kNone || label[o / 3] == kNone) e0 = min(e0, e);
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) e0 = min(e0, __shfl_xor(e0, m, kWave));
  e0 = uni(e0);
  if (e0 >= E) return kContradiction;
  int h = 0, x = e0;
  bool closed = false;
  for (int it = 0; it < E; ++it) {                                   // every step consumes one directed edge of the component
    const int o = uni(nb[x]);
    if (o == kNone || uni(label[o / 3]) == kNone) {
      if (h >= d) return kContradiction;
      if (lane == 0) out[h] = pts[uni(tv[x])];
      ++h;
      x = next_edge(x);
    } else {
      x = next_edge(o);                                              // across the interior edge: the next triangle of the fan
    }
    if (x == e0) { closed = true; break; }
  }
  return closed ? h : kContradiction;
}

}  // namespace
}  // namespace segger
