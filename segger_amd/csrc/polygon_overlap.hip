// segger_polygon_overlap_candidates / _pairs: the overlap join of two ring CSRs -- for every pair (a, b) of polygons whose
// closed bounding boxes overlap, whether the closed polygons share a point and the area of their intersection.  This is the
// reference's polygons_in_polygons (src/segger/geometry/query.py:244-285, a CPU gpd.sjoin with predicate='intersects') and
// the sizing of a segmentation-against-vendor comparison (IoU per cell).  include/segger_amd.h has the contract: the
// measure-theoretic area formula, the predicate, the arithmetic.
//
// Kernels, one stream, no host synchronisation inside an entry point (the grid, cell_of and segments_meet are rings.h's; the
// scan kernel and the slot of a candidate, hit_slot, are post_common.h's):
//   ov_bin_kernel    one thread per polygon of a set: checks its ring (rings.h), its bounding box, the range of grid cells
//                    the box covers, and appends it to the list of its route -- "gridded" (at most SEGGER_OVERLAP_WIDE_CELLS
//                    cells) or "wide"; a gridded polygon of set B adds one to the count of every cell it covers;
//   counts_to_offsets_kernel<int32 | int64>  one workgroup: counts -> starts, in place (the cells of the grid; the items of
//                    the candidate pass);
//   ov_grid_kernel   one thread per gridded polygon of B: its id into every cell it covers (an integer cursor per cell: the
//                    order within a cell is the scheduling's, and nothing that is returned depends on it);
//   ov_cand_kernel   count / fill over ONE traversal, one wave per item.  Item a < Pa is polygon a of A: gridded, it walks
//                    the cells it covers and meets b there; a pair is emitted only in the cell (max(cx0_a, cx0_b),
//                    max(cy0_a, cy0_b)) -- the cell of the lower-left corner of the two boxes' intersection, because the
//                    cell of a coordinate is monotone -- so once; wide, it is tested against every polygon of B.  Item
//                    Pa + b is polygon b of B and does something only when b is wide: it is tested against every gridded
//                    polygon of A (wide a against wide b was item a's).  No Pa x Pb pass unless a polygon is wide;
//   ov_pair_kernel   one wave per candidate, in three tiers by max(n_a, n_b): both rings in registers (<= 64), both in LDS
//                    of a single-wave workgroup at 256 vertices each (8192 B) or at SEGGER_MORPH_MAX_VERTS each (131072 B:
//                    one workgroup per CU).  Every tier's launch strides over the whole candidate list and takes its own.
//
// The pair, one definition for the three tiers (pair_body): both rings translated to the first vertex of ring A, y0 the lowest
// y of the pair.  Edge pair (k of A, l of B) has index t = k n_b + l and belongs to lane t mod 64; a lane adds its terms in
// increasing t; the lanes are combined with wave_sum_f64.  So the bits do not depend on the tier, on the order of the
// polygons in either set or on the run.  No float atomics.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel; LDS per workgroup 0 / 8192 B /
// 131072 B for the three tiers of ov_pair_kernel, at most 2 KB for the scan, none elsewhere.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kOvThreads = 256;
constexpr int kOvWaves = kOvThreads / kWave;
constexpr int kOvSmallCap = SEGGER_OVERLAP_SMALL_VERTS;
constexpr int kOvLargeCap = SEGGER_MORPH_MAX_VERTS;
// int32 words of the workspace's first region: set A's flag and list lengths at 0 .. 2 (rings.h), set B's at 8 .. 10
constexpr int kWordsB = 8, kWordLdsPairs = 16;

__device__ __forceinline__ bool is_wide(int4 c) { return (int64_t)(c.z - c.x + 1) * (c.w - c.y + 1) > SEGGER_OVERLAP_WIDE_CELLS; }
// closed boxes
__device__ __forceinline__ bool boxes_meet(double4 a, double4 b) { return a.x <= b.z && b.x <= a.z && a.y <= b.w && b.y <= a.w; }

// ---------------------------------------------------------------- binning ---
struct OvSet {
  const int64_t* off; const double* xy; int64_t P, V;
  double4* box; int4* cells; int32_t* nv;                            // per polygon; nv = 0: pairs with nothing
  int32_t *words, *list_grid, *list_wide;
};

__global__ __launch_bounds__(kOvThreads) void ov_bin_kernel(OvSet s, UniformGrid g, int32_t* __restrict__ cell_count) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kOvThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kOvThreads + (threadIdx.x & ~(kWave - 1)); base < s.P; base += stride) {
    const int64_t p = base + lane;
    int route = -1;
    if (p < s.P) {
      const RingClass c = classify_ring(s.off, s.xy, p, s.V);
      if (c.bad) atomicOr(&s.words[kWordFlag], c.bad);
      double4 box = make_double4(0.0, 0.0, 0.0, 0.0);
      int4 cells = make_int4(0, 0, 0, 0);
      const bool pairs = !c.bad && c.n >= 3;
      if (pairs) {
        const double2* v = reinterpret_cast<const double2*>(s.xy) + s.off[p];
        box = make_double4(v[0].x, v[0].y, v[0].x, v[0].y);
        for (int k = 1; k < (int)c.n; ++k) {
          const double2 q = v[k];
          box.x = fmin(box.x, q.x); box.y = fmin(box.y, q.y); box.z = fmax(box.z, q.x); box.w = fmax(box.w, q.y);
        }
        cells = make_int4(cell_of(box.x, g.x0, g.inv_cell, g.nx), cell_of(box.y, g.y0, g.inv_cell, g.ny),
                          cell_of(box.z, g.x0, g.inv_cell, g.nx), cell_of(box.w, g.y0, g.inv_cell, g.ny));
        if (cells.z < cells.x) cells.z = cells.x;                    // NaN coordinates: an empty range would be a negative count
        if (cells.w < cells.y) cells.w = cells.y;
        route = is_wide(cells);
        if (cell_count && route == 0)
          for (int cy = cells.y; cy <= cells.w; ++cy)
            for (int cx = cells.x; cx <= cells.z; ++cx) atomicAdd(&cell_count[(int64_t)cy * g.nx + cx + 1], 1);
      }
      s.box[p] = box; s.cells[p] = cells; s.nv[p] = pairs ? (int32_t)c.n : 0;
    }
    append_by_route(route, p, s.words, s.list_grid, s.list_wide);
  }
}

__global__ __launch_bounds__(kOvThreads) void ov_grid_kernel(const int4* __restrict__ cells, const int32_t* __restrict__ words,
                                                             const int32_t* __restrict__ list_grid, UniformGrid g,
                                                             const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor,
                                                             int32_t* __restrict__ entries, int64_t capacity) {
  const int count = words[kWordShort];
  const int stride = (int)gridDim.x * kOvThreads;
  for (int w = (int)blockIdx.x * kOvThreads + (int)threadIdx.x; w < count; w += stride) {
    const int32_t b = list_grid[w];
    const int4 c = cells[b];
    for (int cy = c.y; cy <= c.w; ++cy)
      for (int cx = c.x; cx <= c.z; ++cx) {
        const int64_t cell = (int64_t)cy * g.nx + cx;
        const int64_t pos = (int64_t)cell_start[cell] + atomicAdd(&cursor[cell], 1);
        if (pos >= 0 && pos < capacity && pos < cell_start[cell + 1]) entries[pos] = b;
      }
  }
}

// ---------------------------------------------------------------- candidates ---
struct OvCand {
  const double4 *box_a, *box_b; const int4 *cells_a, *cells_b; const int32_t *nv_a, *nv_b;
  int64_t Pa, Pb; UniformGrid g;
  const int32_t *cell_start, *entries;
  int64_t* item_off;                                                 // [Pa + Pb + 1]: count writes [i + 1], fill reads
  int64_t* cand; int64_t capacity;                                   // fill: a << 32 | b
};

// One wave tests the polygons ids[s0 .. s1) (ids == NULL: s0 .. s1 themselves) of the other set against `mine`; kMode 0: `mine`
// is a gridded a in cell (cx, cy), the others the b of that cell; 1: a wide a against every b; 2: a wide b against the gridded a.
template <bool kFill, int kMode>
__device__ __forceinline__ int64_t span_test(const OvCand& c, int64_t me, double4 mine, int4 my_cells, int cx, int cy, const int32_t* ids,
                                             int64_t s0, int64_t s1, int64_t begin, int64_t found, int64_t end) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t sb = s0; sb < s1; sb += kWave) {
    const int64_t s = sb + lane;
    bool hit = false;
    int64_t other = 0;
    if (s < s1) {
      other = ids ? (int64_t)ids[s] : s;
      if (kMode == 2) hit = c.nv_a[other] > 0 && !is_wide(c.cells_a[other]) && boxes_meet(mine, c.box_a[other]);
      else {
        hit = c.nv_b[other] > 0 && boxes_meet(mine, c.box_b[other]);
        if (kMode == 0) {
          const int4 o = c.cells_b[other];
          hit = hit && cx == (my_cells.x > o.x ? my_cells.x : o.x) && cy == (my_cells.y > o.y ? my_cells.y : o.y);
        }
      }
    }
    hit_slot<kFill>(hit, begin, end, found, [&](int64_t slot) { c.cand[slot] = kMode == 2 ? ((other << 32) | me) : ((me << 32) | other); });
  }
  return found;
}

template <bool kFill>
__global__ __launch_bounds__(kOvThreads) void ov_cand_kernel(OvCand c) {
  const int64_t items = c.Pa + c.Pb;
  const int64_t n_waves = (int64_t)gridDim.x * kOvWaves;
  for (int64_t i = (int64_t)blockIdx.x * kOvWaves + (threadIdx.x >> 6); i < items; i += n_waves) {             // wave-uniform
    int64_t begin = 0, end = 0, found = 0;
    if (kFill) {
      begin = c.item_off[i];
      end = c.item_off[i + 1];
      if (end > c.capacity) end = c.capacity;                        // nothing is ever written at or beyond either
    }
    if (i < c.Pa) {
      if (c.nv_a[i] > 0) {
        const double4 mine = c.box_a[i];
        const int4 mc = c.cells_a[i];
        if (is_wide(mc)) found = span_test<kFill, 1>(c, i, mine, mc, 0, 0, nullptr, 0, c.Pb, begin, found, end);
        else
          for (int cy = mc.y; cy <= mc.w; ++cy)
            for (int cx = mc.x; cx <= mc.z; ++cx) {
              const int64_t cell = (int64_t)cy * c.g.nx + cx;
              found = span_test<kFill, 0>(c, i, mine, mc, cx, cy, c.entries, c.cell_start[cell], c.cell_start[cell + 1], begin, found, end);
            }
      }
    } else {
      const int64_t b = i - c.Pa;
      if (c.nv_b[b] > 0 && is_wide(c.cells_b[b]))
        found = span_test<kFill, 2>(c, b, c.box_b[b], c.cells_b[b], 0, 0, nullptr, 0, c.Pa, begin, found, end);
    }
    if (!kFill && (threadIdx.x & (kWave - 1)) == 0) c.item_off[i + 1] = found;
  }
}

// ---------------------------------------------------------------- the pair ---
// (segments_meet is rings.h's, defined next to simplify.hip's touch)
// y of the line through p and q (p.x != q.x) at x; an endpoint's own y at an endpoint's x, so shared vertices agree bit for bit
__device__ __forceinline__ double y_at(P2 p, P2 q, double x) {
  if (x == p.x) return p.y;
  if (x == q.x) return q.y;
  return p.y + (x - p.x) * ((q.y - p.y) / (q.x - p.x));
}
// the integral of min(y_e, y_f) - y0 over the overlap of the x-ranges of e = (p, q) and f = (r, s); neither is vertical
__device__ __forceinline__ double edge_term(P2 p, P2 q, P2 r, P2 s, double y0) {
  const double xl = fmax(fmin(p.x, q.x), fmin(r.x, s.x)), xr = fmin(fmax(p.x, q.x), fmax(r.x, s.x));
  if (!(xl < xr)) return 0.0;
  const double el = y_at(p, q, xl), er = y_at(p, q, xr), fl = y_at(r, s, xl), fr = y_at(r, s, xr);
  const double dl = el - fl, dr = er - fr, w = xr - xl;
  const double ml = fmin(el, fl) - y0, mr = fmin(er, fr) - y0;
  if ((dl < 0.0 && dr > 0.0) || (dl > 0.0 && dr < 0.0)) {            // the lines cross once inside: two trapezoids
    const double t = dl / (dl - dr);
    const double mc = (el + t * (er - el)) - y0;
    return 0.5 * w * (t * (ml + mc) + (1.0 - t) * (mc + mr));
  }
  return 0.5 * w * (ml + mr);
}

struct PairOut { bool hit; double area; };

// One pair, one wave, every lane active.  Both stores hold their ring translated to ring A's first vertex.
template <class Ring>
__device__ __forceinline__ PairOut pair_body(const Ring& ra, int na, const Ring& rb, int nb) {
  const int lane = threadIdx.x & (kWave - 1);
  // the shoelace sums (their signs are the orientations) and the lowest y: vertex k belongs to lane k mod 64 on every tier
  double sa = 0.0, sb = 0.0, y0 = INFINITY;
  const int nmax = na > nb ? na : nb;
  for (int base = 0; base < nmax; base += kWave) {
    const int k = base + lane;
    const int ka = k < na ? k : 0, kb = k < nb ? k : 0;
    const P2 a0 = ra.at(ka), a1 = ra.at(ka + 1 == na ? 0 : ka + 1), b0 = rb.at(kb), b1 = rb.at(kb + 1 == nb ? 0 : kb + 1);
    if (k < na) { sa += a0.x * a1.y - a1.x * a0.y; y0 = fmin(y0, a0.y); }
    if (k < nb) { sb += b0.x * b1.y - b1.x * b0.y; y0 = fmin(y0, b0.y); }
  }
  sa = wave_sum_f64(sa); sb = wave_sum_f64(sb); y0 = wave_min_f64(y0);
  const double sign_a = (double)((int)(sa > 0.0) - (int)(sa < 0.0)), sign_b = (double)((int)(sb > 0.0) - (int)(sb < 0.0));

  // vertex 0 of A in B and vertex 0 of B in A, points_in_polygons' half-open parity rule
  const P2 pa = ra.at(0), pb = rb.at(0);
  bool in_b = false, in_a = false;
  for (int base = 0; base < nmax; base += kWave) {
    const int k = base + lane;
    const int ka = k < na ? k : 0, kb = k < nb ? k : 0;
    const P2 a0 = ra.at(ka), a1 = ra.at(ka + 1 == na ? 0 : ka + 1), b0 = rb.at(kb), b1 = rb.at(kb + 1 == nb ? 0 : kb + 1);
    if (k < nb) {
      const double cr = (b1.x - b0.x) * (pa.y - b0.y) - (b1.y - b0.y) * (pa.x - b0.x);
      const bool lo0 = b0.y <= pa.y, lo1 = b1.y <= pa.y;
      in_b ^= (lo0 && !lo1 && cr > 0.0) || (!lo0 && lo1 && cr < 0.0);
    }
    if (k < na) {
      const double cr = (a1.x - a0.x) * (pb.y - a0.y) - (a1.y - a0.y) * (pb.x - a0.x);
      const bool lo0 = a0.y <= pb.y, lo1 = a1.y <= pb.y;
      in_a ^= (lo0 && !lo1 && cr > 0.0) || (!lo0 && lo1 && cr < 0.0);
    }
  }
  bool hit = ((__popcll(__ballot(in_b)) | __popcll(__ballot(in_a))) & 1) != 0;

  // the edge pairs: t = k nb + l, lane t mod 64, ascending t
  const int64_t total = (int64_t)na * nb;
  const int step_k = kWave / nb, step_l = kWave % nb;
  int k = lane / nb, l = lane % nb;
  double acc = 0.0;
  bool meet = false;
  for (int64_t base = 0; base < total; base += kWave) {
    const bool valid = base + lane < total;
    const int kk = valid ? k : 0, ll = valid ? l : 0;
    const P2 p = ra.at(kk), q = ra.at(kk + 1 == na ? 0 : kk + 1), r = rb.at(ll), s = rb.at(ll + 1 == nb ? 0 : ll + 1);
    // closed x-ranges apart: no shared point and an empty overlap, the term is zero
    if (valid && fmax(p.x, q.x) >= fmin(r.x, s.x) && fmax(r.x, s.x) >= fmin(p.x, q.x)) {
      if (fmax(p.y, q.y) >= fmin(r.y, s.y) && fmax(r.y, s.y) >= fmin(p.y, q.y)) meet = meet || segments_meet(p, q, r, s);
      if (p.x != q.x && r.x != s.x) {
        const double sigma = (p.x > q.x ? sign_a : -sign_a) * (r.x > s.x ? sign_b : -sign_b);
        acc += sigma * edge_term(p, q, r, s, y0);
      }
    }
    k += step_k; l += step_l;
    if (l >= nb) { l -= nb; ++k; }
  }
  hit = hit || __ballot(meet) != 0;
  return PairOut{hit, wave_sum_f64(acc)};
}

struct OvPair {
  const int64_t *off_a, *off_b; const double *xy_a, *xy_b;
  const int32_t *nv_a, *nv_b; int64_t Pa, Pb;
  const double *area_a, *area_b;                                     // NULL: no upper clamp
  const int64_t* cand; const int64_t* n_cand; int64_t capacity;
  int reg_max, small_max;                                            // the tiers' upper ends
  uint8_t* hit; double* area; int32_t* words;
};

__device__ __forceinline__ void pair_store(const OvPair& a, int64_t w, int64_t ia, int64_t ib, PairOut o) {
  if ((threadIdx.x & (kWave - 1)) != 0) return;
  double v = 0.0;
  if (o.hit) {                                                       // apart: the intersection is empty, exactly
    v = fmax(o.area, 0.0);                                           // (a NaN becomes 0)
    if (a.area_a) v = fmin(v, fmin(a.area_a[ia], a.area_b[ib]));
  }
  a.hit[w] = (uint8_t)o.hit;
  a.area[w] = v;
}

// tier of a pair: 0 registers, 1 small LDS, 2 large LDS
__device__ __forceinline__ int pair_tier(const OvPair& a, int na, int nb) {
  const int n = na > nb ? na : nb;
  return n <= a.reg_max ? 0 : (n <= a.small_max ? 1 : 2);
}

__global__ __launch_bounds__(kOvThreads) void ov_pair_reg_kernel(OvPair a) {
  const int lane = threadIdx.x & (kWave - 1);
  int64_t count = *a.n_cand;
  if (count > a.capacity) count = a.capacity;
  const int64_t n_waves = (int64_t)gridDim.x * kOvWaves;
  for (int64_t w = (int64_t)blockIdx.x * kOvWaves + (threadIdx.x >> 6); w < count; w += n_waves) {              // wave-uniform
    const int64_t key = a.cand[w], ia = key >> 32, ib = key & 0xffffffffll;
    if ((uint64_t)ia >= (uint64_t)a.Pa || (uint64_t)ib >= (uint64_t)a.Pb) continue;      // never: the fill wrote every key
    const int na = __builtin_amdgcn_readfirstlane(a.nv_a[ia]), nb = __builtin_amdgcn_readfirstlane(a.nv_b[ib]);
    if (pair_tier(a, na, nb) != 0) continue;
    const double2* va = reinterpret_cast<const double2*>(a.xy_a) + a.off_a[ia];
    const double2* vb = reinterpret_cast<const double2*>(a.xy_b) + a.off_b[ib];
    const double2 org = va[0];
    const double2 ma = va[lane < na ? lane : 0], mb = vb[lane < nb ? lane : 0];
    const RegRing ra{ma.x - org.x, ma.y - org.y}, rb{mb.x - org.x, mb.y - org.y};
    pair_store(a, w, ia, ib, pair_body(ra, na, rb, nb));
  }
}

template <int kCap>
__global__ __launch_bounds__(kWave) void ov_pair_lds_kernel(OvPair a, int tier) {
  __shared__ double2 pts_a[kCap];
  __shared__ double2 pts_b[kCap];
  const int lane = threadIdx.x;
  int64_t count = *a.n_cand;
  if (count > a.capacity) count = a.capacity;
  for (int64_t w = (int64_t)blockIdx.x; w < count; w += (int64_t)gridDim.x) {
    const int64_t key = a.cand[w], ia = key >> 32, ib = key & 0xffffffffll;
    if ((uint64_t)ia >= (uint64_t)a.Pa || (uint64_t)ib >= (uint64_t)a.Pb) continue;      // never: the fill wrote every key
    const int na = __builtin_amdgcn_readfirstlane(a.nv_a[ia]), nb = __builtin_amdgcn_readfirstlane(a.nv_b[ib]);
    if (pair_tier(a, na, nb) != tier || na > kCap || nb > kCap) continue;
    const double2* va = reinterpret_cast<const double2*>(a.xy_a) + a.off_a[ia];
    const double2* vb = reinterpret_cast<const double2*>(a.xy_b) + a.off_b[ib];
    const double2 org = va[0];
    __syncthreads();                                                 // the previous pair's readers are done
    for (int i = lane; i < na; i += kWave) { const double2 v = va[i]; pts_a[i] = double2{v.x - org.x, v.y - org.y}; }
    for (int i = lane; i < nb; i += kWave) { const double2 v = vb[i]; pts_b[i] = double2{v.x - org.x, v.y - org.y}; }
    __syncthreads();
    if (lane == 0) atomicAdd(&a.words[kWordLdsPairs], 1);
    pair_store(a, w, ia, ib, pair_body(LdsRing{pts_a}, na, LdsRing{pts_b}, nb));
  }
}

// ---------------------------------------------------------------- host ---
struct OvLayout {
  size_t words;
  RingLists lists_a, lists_b;
  size_t box_a, box_b, cells_a, cells_b, nv_a, nv_b, cell_start, cursor, entries, item_off, total;
};

// with Pa, Pb and n_cells below 2^31 every term is below 2^40 bytes: nothing here can overflow
OvLayout ov_layout(int64_t Pa, int64_t Pb, int64_t n_cells) {
  OvLayout l;
  Carver c;
  l.lists_a = take_ring_lists(c, Pa);                                // its words are the unit's: A's at 0, B's at kWordsB
  l.words = l.lists_a.words;
  l.lists_b.words = l.words + kWordsB * sizeof(int32_t);
  const size_t list_b = (size_t)Pb * sizeof(int32_t);
  l.lists_b.list_short = c.take(list_b);
  l.lists_b.list_long = c.take(list_b);
  l.box_a = c.take((size_t)Pa * sizeof(double4));
  l.box_b = c.take((size_t)Pb * sizeof(double4));
  l.cells_a = c.take((size_t)Pa * sizeof(int4));
  l.cells_b = c.take((size_t)Pb * sizeof(int4));
  l.nv_a = c.take((size_t)Pa * sizeof(int32_t));
  l.nv_b = c.take((size_t)Pb * sizeof(int32_t));
  l.cell_start = c.take((size_t)(n_cells + 1) * sizeof(int32_t));
  l.cursor = c.take((size_t)n_cells * sizeof(int32_t));
  l.entries = c.take((size_t)Pb * SEGGER_OVERLAP_WIDE_CELLS * sizeof(int32_t));
  l.item_off = c.take((size_t)(Pa + Pb + 1) * sizeof(int64_t));
  l.total = c.total();
  return l;
}

int ov_check_sizes(const char* who, int64_t Pa, int64_t Pb, int32_t nx, int32_t ny) {
  SEGGER_REQUIRE(Pa >= 0 && Pb >= 0, "%s: negative n_polygons_a or n_polygons_b", who);
  SEGGER_REQUIRE(Pa < 0x7fffffffLL / SEGGER_OVERLAP_WIDE_CELLS && Pb < 0x7fffffffLL / SEGGER_OVERLAP_WIDE_CELLS,
                 "%s: 2^31 / %d polygons or more in a set", who, SEGGER_OVERLAP_WIDE_CELLS);
  SEGGER_REQUIRE(nx >= 1 && ny >= 1 && (int64_t)nx * ny < 0x7fffffffLL, "%s: bad grid: nx, ny >= 1 and nx * ny < 2^31 - 1", who);
  return SEGGER_OK;
}

struct OvCall {
  const int64_t* off_a; const double* xy_a; int64_t Pa, Va; const int64_t* off_b; const double* xy_b; int64_t Pb, Vb;
  double x0, y0, cell; int32_t nx, ny; void* workspace; int64_t workspace_bytes;
};

// everything both entry points reject; *empty = nothing to do (no pointer was looked at)
int ov_check(const char* who, const OvCall& c, bool* empty) {
  *empty = false;
  const int rc = ov_check_sizes(who, c.Pa, c.Pb, c.nx, c.ny);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(c.Va >= 0 && c.Vb >= 0, "%s: negative n_vertices_a or n_vertices_b", who);
  SEGGER_REQUIRE(c.workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(c.cell > 0.0 && c.cell < INFINITY && c.x0 - c.x0 == 0.0 && c.y0 - c.y0 == 0.0,
                 "%s: bad grid: the origin must be finite and the cell side positive and finite", who);
  if (c.Pa == 0 || c.Pb == 0) { *empty = true; return SEGGER_OK; }
  const size_t need = ov_layout(c.Pa, c.Pb, (int64_t)c.nx * c.ny).total;
  return check_ring_call(who, c.off_a, c.xy_a, c.Va, c.workspace, c.workspace_bytes, need,
                         OtherPointers{c.off_b && (c.xy_b || c.Vb == 0), is_aligned(c.off_b, 8), is_aligned(c.xy_b, 16),
                                       "ring_offsets_a and ring_offsets_b", "xy_a and xy_b"});
}

OvSet ov_set(const OvCall& c, const OvLayout& l, bool b) {
  void* ws = c.workspace;
  const RingLists& r = b ? l.lists_b : l.lists_a;
  return OvSet{b ? c.off_b : c.off_a, b ? c.xy_b : c.xy_a, b ? c.Pb : c.Pa, b ? c.Vb : c.Va,
               at<double4>(ws, b ? l.box_b : l.box_a), at<int4>(ws, b ? l.cells_b : l.cells_a), at<int32_t>(ws, b ? l.nv_b : l.nv_a),
               at<int32_t>(ws, r.words), at<int32_t>(ws, r.list_short), at<int32_t>(ws, r.list_long)};
}

OvCand ov_cand(const OvCall& c, const OvLayout& l, int64_t* cand, int64_t capacity) {
  void* ws = c.workspace;
  return OvCand{at<double4>(ws, l.box_a), at<double4>(ws, l.box_b), at<int4>(ws, l.cells_a), at<int4>(ws, l.cells_b),
                at<int32_t>(ws, l.nv_a), at<int32_t>(ws, l.nv_b), c.Pa, c.Pb, UniformGrid{c.x0, c.y0, 1.0 / c.cell, c.nx, c.ny},
                at<int32_t>(ws, l.cell_start), at<int32_t>(ws, l.entries), at<int64_t>(ws, l.item_off), cand, capacity};
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_polygon_overlap_workspace_bytes(int64_t n_polygons_a, int64_t n_polygons_b, int32_t nx, int32_t ny) {
  const int rc = ov_check_sizes("segger_polygon_overlap_workspace_bytes", n_polygons_a, n_polygons_b, nx, ny);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)ov_layout(n_polygons_a, n_polygons_b, (int64_t)nx * ny).total;
}

extern "C" int segger_polygon_overlap_candidates(const int64_t* ring_offsets_a, const double* xy_a, int64_t n_polygons_a,
                                                 int64_t n_vertices_a, const int64_t* ring_offsets_b, const double* xy_b,
                                                 int64_t n_polygons_b, int64_t n_vertices_b, double x0, double y0, double cell,
                                                 int32_t nx, int32_t ny, int64_t* n_candidates, void* workspace,
                                                 int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_polygon_overlap_candidates";
  hipStream_t stream = (hipStream_t)stream_;
  const OvCall c{ring_offsets_a, xy_a, n_polygons_a, n_vertices_a, ring_offsets_b, xy_b, n_polygons_b, n_vertices_b,
                 x0, y0, cell, nx, ny, workspace, workspace_bytes};
  bool empty = false;
  const int rc = ov_check(who, c, &empty);
  if (rc != SEGGER_OK || empty) return rc;
  SEGGER_REQUIRE(n_candidates, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(n_candidates, 8), "%s: n_candidates must be 8-byte aligned", who);
  const int64_t n_cells = (int64_t)nx * ny;
  const OvLayout l = ov_layout(n_polygons_a, n_polygons_b, n_cells);
  const OvSet sa = ov_set(c, l, false), sb = ov_set(c, l, true);
  const OvCand k = ov_cand(c, l, nullptr, 0);
  int32_t* cell_start = at<int32_t>(workspace, l.cell_start);
  int32_t* cursor = at<int32_t>(workspace, l.cursor);
  const int cus = cu_count_or_default();
  SEGGER_HIP(hipMemsetAsync(sa.words, 0, kRingWordsBytes, stream));
  SEGGER_HIP(hipMemsetAsync(cell_start, 0, (size_t)(n_cells + 1) * sizeof(int32_t), stream));
  SEGGER_HIP(hipMemsetAsync(cursor, 0, (size_t)n_cells * sizeof(int32_t), stream));
  hipLaunchKernelGGL(ov_bin_kernel, dim3(grid_stride_blocks(c.Pa, kOvThreads, (int64_t)cus * 8)), dim3(kOvThreads), 0, stream, sa, k.g,
                     (int32_t*)nullptr);
  SEGGER_LAUNCH_CHECK("ov_bin_kernel<a>");
  hipLaunchKernelGGL(ov_bin_kernel, dim3(grid_stride_blocks(c.Pb, kOvThreads, (int64_t)cus * 8)), dim3(kOvThreads), 0, stream, sb, k.g,
                     cell_start);
  SEGGER_LAUNCH_CHECK("ov_bin_kernel<b>");
  hipLaunchKernelGGL((counts_to_offsets_kernel<int32_t>), dim3(1), dim3(kScanThreads), 0, stream, cell_start, n_cells, (int64_t*)nullptr);
  SEGGER_LAUNCH_CHECK("counts_to_offsets_kernel<cells>");
  hipLaunchKernelGGL(ov_grid_kernel, dim3(grid_stride_blocks(c.Pb, kOvThreads, (int64_t)cus * 8)), dim3(kOvThreads), 0, stream,
                     (const int4*)sb.cells, (const int32_t*)sb.words, (const int32_t*)sb.list_grid, k.g, (const int32_t*)cell_start, cursor,
                     at<int32_t>(workspace, l.entries), c.Pb * SEGGER_OVERLAP_WIDE_CELLS);
  SEGGER_LAUNCH_CHECK("ov_grid_kernel");
  hipLaunchKernelGGL((ov_cand_kernel<false>), dim3(grid_stride_blocks(c.Pa + c.Pb, kOvWaves, (int64_t)cus * 16)), dim3(kOvThreads), 0,
                     stream, k);
  SEGGER_LAUNCH_CHECK("ov_cand_kernel<count>");
  hipLaunchKernelGGL((counts_to_offsets_kernel<int64_t>), dim3(1), dim3(kScanThreads), 0, stream, k.item_off, c.Pa + c.Pb, n_candidates);
  SEGGER_LAUNCH_CHECK("counts_to_offsets_kernel<items>");
  return SEGGER_OK;
}

extern "C" int segger_polygon_overlap_pairs(const int64_t* ring_offsets_a, const double* xy_a, int64_t n_polygons_a,
                                            int64_t n_vertices_a, const int64_t* ring_offsets_b, const double* xy_b,
                                            int64_t n_polygons_b, int64_t n_vertices_b, double x0, double y0, double cell,
                                            int32_t nx, int32_t ny, const double* area_a, const double* area_b,
                                            const int64_t* n_candidates, int64_t* candidates, uint8_t* intersects, double* area,
                                            int64_t capacity, int32_t reg_max_verts, int32_t small_max_verts, void* workspace,
                                            int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_polygon_overlap_pairs";
  hipStream_t stream = (hipStream_t)stream_;
  const OvCall c{ring_offsets_a, xy_a, n_polygons_a, n_vertices_a, ring_offsets_b, xy_b, n_polygons_b, n_vertices_b,
                 x0, y0, cell, nx, ny, workspace, workspace_bytes};
  bool empty = false;
  const int rc = ov_check(who, c, &empty);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(capacity >= 0, "%s: negative capacity", who);
  SEGGER_REQUIRE(reg_max_verts >= 0 && reg_max_verts <= kWave, "%s: reg_max_verts %d outside 0 .. %d", who, (int)reg_max_verts, kWave);
  SEGGER_REQUIRE(small_max_verts >= 0 && small_max_verts <= SEGGER_OVERLAP_SMALL_VERTS, "%s: small_max_verts %d outside 0 .. %d", who,
                 (int)small_max_verts, SEGGER_OVERLAP_SMALL_VERTS);
  if (empty || capacity == 0) return SEGGER_OK;
  SEGGER_REQUIRE(n_candidates && candidates && intersects && area && (area_a != nullptr) == (area_b != nullptr), "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(n_candidates, 8) && is_aligned(candidates, 8) && is_aligned(area, 8) && is_aligned(area_a, 8) &&
                 is_aligned(area_b, 8), "%s: n_candidates, candidates, area, area_a and area_b must be 8-byte aligned", who);
  const OvLayout l = ov_layout(n_polygons_a, n_polygons_b, (int64_t)nx * ny);
  const OvCand k = ov_cand(c, l, candidates, capacity);
  const int cus = cu_count_or_default();
  hipLaunchKernelGGL((ov_cand_kernel<true>), dim3(grid_stride_blocks(c.Pa + c.Pb, kOvWaves, (int64_t)cus * 16)), dim3(kOvThreads), 0,
                     stream, k);
  SEGGER_LAUNCH_CHECK("ov_cand_kernel<fill>");
  const OvPair p{ring_offsets_a, ring_offsets_b, xy_a, xy_b, k.nv_a, k.nv_b, n_polygons_a, n_polygons_b, area_a, area_b, candidates, n_candidates, capacity,
                 reg_max_verts, small_max_verts > reg_max_verts ? small_max_verts : reg_max_verts, intersects, area,
                 at<int32_t>(workspace, l.words)};
  hipLaunchKernelGGL(ov_pair_reg_kernel, dim3(grid_stride_blocks(capacity, kOvWaves, (int64_t)cus * 16)), dim3(kOvThreads), 0, stream, p);
  SEGGER_LAUNCH_CHECK("ov_pair_reg_kernel");
  hipLaunchKernelGGL((ov_pair_lds_kernel<kOvSmallCap>), dim3(grid_stride_blocks(capacity, 1, (int64_t)cus * 16)), dim3(kWave), 0, stream,
                     p, 1);
  SEGGER_LAUNCH_CHECK("ov_pair_lds_kernel<small>");
  hipLaunchKernelGGL((ov_pair_lds_kernel<kOvLargeCap>), dim3(grid_stride_blocks(capacity, 1, (int64_t)cus)), dim3(kWave), 0, stream, p, 2);
  SEGGER_LAUNCH_CHECK("ov_pair_lds_kernel<large>");
  return SEGGER_OK;
}
