// segger_rasterize_rings: an [H, W] int32 label image from a CSR of rings -- the transform opposite to contours.hip's.  No
// reference counterpart exists (the reference only reads label images); include/segger_amd.h has the contract, which is
// this project's own.  Pixel (row r, column c) stands for the world point (c sx + tx, r sy + ty), one multiplication and
// one addition in float64, not fused; that point is tested against the ring as given with ring_predicate.h's
// ring_decide(ring_distance(...), 0, predicate) -- the code of polygon_join.hip, so the pixels of polygon p are, bit for bit,
// the pairs the join lists for p over the pixel centres.  A pixel matched by several polygons goes to the lowest or the
// highest polygon INDEX: an integer atomic min or max on the index, mapped to the label by a later pass.
//
// Five kernels on one stream, no host synchronisation:
//   raster_bin_kernel     one thread per polygon: checks its ring (rings.h), zeroes n_covered and n_won, counts a ring of
//                         fewer than 3 vertices (degenerate, empty) and appends the others to the list of their route;
//   raster_short_kernel   n <= 64: one wave per polygon, the ring in registers, four waves a workgroup, no LDS;
//   raster_long_kernel    64 < n <= SEGGER_MORPH_MAX_VERTS (or every ring, reg_max = 0): one single-wave workgroup per
//                         polygon, the ring in LDS (64 KB, two workgroups a CU, as the join's);
//   raster_finish_kernel  one thread per pixel: index -> label (0 where no polygon claimed the pixel), n_won with equal
//                         neighbours of a wave folded into one int64 atomic, n_pixels_set;
// (the image is set to 0xff bytes first: 0xffffffff loses every unsigned min, -1 every signed max).
// The two polygon kernels are rings.h's loops around raster_body: the wave converts the ring's bounds to a clipped pixel
// range (pixel_range), takes the range in B x B blocks, 64 block centres a step, and evaluates ring_distance ONCE at each
// centre.  A block whose centre is farther from the ring than the block reaches (block_threshold) holds no edge: it is
// filled or skipped whole.  The other blocks are compacted (one ds_permute) and their pixels evaluated one per lane, 64 a
// step.  B = 1: no centres, every pixel of the range is evaluated.
//
// Why the bytes do not depend on B, on the route or on scheduling: the shortcut only ever answers what the predicate
// answers at every pixel of the block (the argument is at block_threshold), the min / max are integer atomics, and the
// counts are integer sums.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel; raster_long_kernel holds
// 65536 B of LDS, the others none.  DESIGN 3.5s has the register figures.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "ring_predicate.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

static_assert(SEGGER_RASTER_ERR_OFFSETS == SEGGER_MORPH_ERR_OFFSETS && SEGGER_RASTER_ERR_CAP == SEGGER_MORPH_ERR_CAP,
              "classify_ring returns the bits this unit ORs into its word");
static_assert(SEGGER_RASTER_INTERSECTS == SEGGER_PJOIN_INTERSECTS && SEGGER_RASTER_CONTAINS == SEGGER_PJOIN_CONTAINS,
              "ring_decide reads the join's predicate codes");

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / kWave;
constexpr int kCtrSet = 0, kCtrOverlaps = 1, kCtrEmpty = 2, kCtrClipped = 3, kCtrDegenerate = 4, kCtrLarge = 5, kCtrFilled = 6;
static_assert(kCtrFilled + 1 == SEGGER_RASTER_COUNTERS, "the counters of include/segger_amd.h");

struct RasterArgs {
  const int64_t* off;
  const double* xy;
  int32_t* words;
  int H, W;
  double sx, sy, tx, ty;
  double inv_sx, inv_sy;                                             // for the pixel range alone, never for a decision
  double half_diag;                                                  // (B - 1) / 2 * |(sx, sy)|: centre to the farthest pixel centre
  double pad;                                                        // what block_threshold adds to the ring's bounds
  int predicate, highest, log2_block;
  int32_t* image;
  int64_t* n_covered;
  unsigned long long* counters;
};

// what a wave adds to the counters once, after its last polygon
struct WaveTotals { unsigned long long covered = 0, empty = 0, clipped = 0, large = 0, filled = 0; };

// ---------------------------------------------------------------- the binning kernel ---
__global__ __launch_bounds__(kRsThreads) void raster_bin_kernel(const int64_t* __restrict__ off, const double* __restrict__ xy, int64_t P,
                                                                 int64_t V, int reg_max, int64_t* __restrict__ n_covered,
                                                                 int64_t* __restrict__ n_won, unsigned long long* __restrict__ counters,
                                                                 int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                                 int32_t* __restrict__ list_long) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kRsThreads;
  unsigned long long degenerate = 0;                                 // the same in every lane
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kRsThreads + (threadIdx.x & ~(kWave - 1)); base < P; base += stride) {
    const int64_t p = base + lane;
    int route = -1;                                                  // -1: matches nothing
    bool few = false;
    if (p < P) {
      const RingClass c = classify_ring(off, xy, p, V);
      if (c.bad) atomicOr(&words[kWordFlag], c.bad);
      n_covered[p] = 0;
      n_won[p] = 0;
      few = !c.bad && c.n < 3;
      if (!c.bad && c.n >= 3) route = c.n > reg_max;                 // reg_max is kWave or 0
    }
    degenerate += (unsigned long long)__popcll(__ballot(few));
    append_by_route(route, p, words, list_short, list_long);
  }
  if (lane == 0 && degenerate) {
    atomicAdd(&counters[kCtrDegenerate], degenerate);
    atomicAdd(&counters[kCtrEmpty], degenerate);                     // they match nothing, as in the join
  }
}

// ---------------------------------------------------------------- bounds -> pixels ---
// The pixel indices lo .. hi (hi < lo: none) of the 0 .. n - 1 along one axis whose centre i s + t can lie in [vmin, vmax],
// the ring's bounds on that axis.  A matching pixel is inside the ring or on it, so in exact arithmetic its centre is
// within the bounds and its index within (vmin - t) / s .. (vmax - t) / s.  The quotient is formed with inv_s = fl(1 / s),
// three roundings of 2^-53 relative each; the centre itself, fl(fl(i s) + t), is off the exact lattice by at most two ulp
// of max(|vmin|, |vmax|, |t|), which is that many ulp / |s| pixels.  The range is therefore widened by ONE WHOLE PIXEL plus
// 2^-40 of the quotient plus 2^-40 of those magnitudes in pixels (four thousand ulp each) instead of being divided
// cleverly: the predicate decides membership, the range only has to hold every candidate.  NaN bounds give no pixels.
// (readfirstlane: the values are the same in every lane already; it tells the compiler so, and the loops become scalar)
struct PixelRange { int lo, hi; };
__device__ __forceinline__ PixelRange pixel_range(double vmin, double vmax, double t, double inv_s, int n) {
  const double a = (vmin - t) * inv_s, b = (vmax - t) * inv_s;
  const double lo = fmin(a, b), hi = fmax(a, b);                     // s may be negative
  const double m = 1.0 + 0x1p-40 * fmax(fabs(lo), fabs(hi)) + 0x1p-40 * fmax(fmax(fabs(vmin), fabs(vmax)), fabs(t)) * fabs(inv_s);
  const double l = floor(lo - m), h = ceil(hi + m);
  const bool some = h >= 0.0 && l <= (double)(n - 1);                // false with a NaN
  PixelRange r;
  r.lo = __builtin_amdgcn_readfirstlane(some ? (int)fmax(l, 0.0) : 0);
  r.hi = __builtin_amdgcn_readfirstlane(some ? (int)fmin(h, (double)(n - 1)) : -1);
  return r;
}

// The squared distance from a block's centre beyond which no edge of the ring passes through the block.  The block is
// B x B pixel centres, its centre their mean, half_diag = (B - 1) / 2 |(sx, sy)| the distance from it to the farthest of
// them.  Let D be the true distance from the centre to the ring and M = the largest magnitude among the ring's bounds plus
// `pad` (four pixels, four half-diagonals and the translation: every centre and every pixel the walk evaluates, and the
// product c s on the way to it, has a magnitude below M).
//  * ring_distance's `best` at the centre has a relative error below 2^-19 once D > 2^-31 M: cr = e x w is off by at most
//    2^-51 |e| |w|, |w| <= 2 M, against |cr| >= |e| D;  the two other branches are sums of squares, a few ulp.
//  * so best > (half_diag (1 + 2^-16) + 2^-30 M)^2 implies D > half_diag + 2^-31 M: the factor 1 + 2^-16 pays for the
//    2^-19 above and for the rounding of half_diag itself (a square root and two products on the host).
//  * the pixel centres as computed, and the translation to the ring's first vertex, move a point by a few ulp of M, below
//    2^-49 M;  every pixel of the block is therefore farther than 2^-32 M from the ring, and so is the straight path from
//    the centre to it.  Its own `best` is not 0 (cr is off by at most 2^-19 of itself there, as above), and the crossing
//    parity does not change along a path that stays off the ring;  the computed parity is the exact one of the computed
//    point: for an edge that straddles the point's y, |cr| = |e.y| h with h >= 2^-32 M the horizontal distance to the
//    crossing, against an error below 2^-51 |e.y| (|e.x| + |w.x|) <= 2^-49 |e.y| M.
// Both predicates then answer the parity at every pixel of the block, which is the centre's: filled or skipped whole.
// A NaN anywhere fails the comparison and the block is evaluated pixel by pixel.
__device__ __forceinline__ double block_threshold(const RasterArgs& a, double xmin, double ymin, double xmax, double ymax) {
  const double M = fmax(fmax(fabs(xmin), fabs(xmax)), fmax(fabs(ymin), fabs(ymax))) + a.pad;
  const double t = a.half_diag * (1.0 + 0x1p-16) + 0x1p-30 * M;
  return t * t;
}

// ---------------------------------------------------------------- the polygon kernels ---
// the pixel goes to the lowest or the highest polygon index that claims it
__device__ __forceinline__ void claim(const RasterArgs& a, int row, int col, int64_t p) {
  int32_t* px = a.image + ((int64_t)row * a.W + col);
  if (a.highest) atomicMax(px, (int)p);                              // -1 before the first claim
  else atomicMin(reinterpret_cast<unsigned int*>(px), (unsigned int)p);      // 0xffffffff before it
}

// The blocks of the lanes in `m`, (bx, by) each in its own lane, compacted to the lanes 0 .. popc(m) - 1 (one permutation
// of the wave: the others go behind them), and their pixels handed to visit(valid, row, col) one per lane, 64 a step, in
// EVERY lane (a visitor may ballot).  A pixel beyond the range's end is not valid.
template <class Visit>
__device__ __forceinline__ void for_block_pixels(unsigned long long m, int bx, int by, int log2_block, const PixelRange& cx,
                                                 const PixelRange& cy, Visit&& visit) {
  const int lane = threadIdx.x & (kWave - 1);
  const int count = (int)__popcll(m);                                // wave-uniform
  if (count == 0) return;
  const int below = (int)__popcll(m & ((1ull << lane) - 1));
  const int dest = ((m >> lane) & 1) ? below : count + (lane - below);
  const int cbx = __builtin_amdgcn_ds_permute(dest << 2, bx), cby = __builtin_amdgcn_ds_permute(dest << 2, by);
  const int total = count << (2 * log2_block);                       // <= 64 * 32 * 32
  const int side_mask = (1 << log2_block) - 1, area_mask = (1 << (2 * log2_block)) - 1;
  for (int tb = 0; tb < total; tb += kWave) {
    const int t = tb + lane;
    const int k = (t >> (2 * log2_block)) & (kWave - 1), within = t & area_mask;
    const int col = cx.lo + (__shfl(cbx, k, kWave) << log2_block) + (within & side_mask);
    const int row = cy.lo + (__shfl(cby, k, kWave) << log2_block) + (within >> log2_block);
    visit(t < total && col <= cx.hi && row <= cy.hi, row, col);
  }
}

// One polygon, one wave, every lane active: r is what rings.h's loops hand over.
template <class Ring>
__device__ __forceinline__ void raster_body(const ListedRing<Ring>& r, const RasterArgs& a, WaveTotals& tot) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = r.p;
  // the closed rectangle of the pixel centres, computed as the centres are
  const double xe = (double)(a.W - 1) * a.sx + a.tx, ye = (double)(a.H - 1) * a.sy + a.ty;
  const bool clipped = r.xmin < fmin(a.tx, xe) || r.xmax > fmax(a.tx, xe) || r.ymin < fmin(a.ty, ye) || r.ymax > fmax(a.ty, ye);
  const PixelRange cx = pixel_range(r.xmin, r.xmax, a.tx, a.inv_sx, a.W), cy = pixel_range(r.ymin, r.ymax, a.ty, a.inv_sy, a.H);
  int64_t covered = 0;                                               // the same in every lane
  auto evaluate = [&](bool valid, int row, int col) {
    bool hit = false;
    if (valid) {                                                     // the edge loop runs under the mask, as in the join's walk
      const double x = (double)col * a.sx + a.tx, y = (double)row * a.sy + a.ty;
      hit = ring_decide(ring_distance(r.ring, r.n, x - r.first.x, y - r.first.y), 0.0, a.predicate);
      if (hit) claim(a, row, col, p);
    }
    covered += (int64_t)__popcll(__ballot(hit));
  };
  if (cx.hi >= cx.lo && cy.hi >= cy.lo) {
    const int wc = cx.hi - cx.lo + 1, hr = cy.hi - cy.lo + 1;
    const int lb = a.log2_block;
    if (lb == 0) {                                                   // no shortcut: the range, row-major, 64 pixels a step
      const uint32_t total = (uint32_t)wc * (uint32_t)hr;            // <= H W < 2^31: 32-bit division, and tb + lane cannot wrap
      for (uint32_t tb = 0; tb < total; tb += kWave) {
        const uint32_t t = tb + lane;
        const uint32_t row = t / (uint32_t)wc, col = t - row * (uint32_t)wc;
        evaluate(t < total, cy.lo + (int)row, cx.lo + (int)col);
      }
    } else {
      const int side = 1 << lb;
      const int nbx = (wc + side - 1) >> lb, nby = (hr + side - 1) >> lb;
      const uint32_t n_blocks = (uint32_t)nbx * (uint32_t)nby;       // <= H W < 2^31
      const double far2 = block_threshold(a, r.xmin, r.ymin, r.xmax, r.ymax);
      const double half = 0.5 * (double)(side - 1);
      for (uint32_t base = 0; base < n_blocks; base += kWave) {
        const uint32_t bi = base + lane;
        int bx = 0, by = 0, state = 0;                               // 0 skipped whole, 1 filled whole, 2 pixel by pixel
        if (bi < n_blocks) {
          by = (int)(bi / (uint32_t)nbx);
          bx = (int)(bi - (uint32_t)by * (uint32_t)nbx);
          const double x = ((double)(cx.lo + (bx << lb)) + half) * a.sx + a.tx;
          const double y = ((double)(cy.lo + (by << lb)) + half) * a.sy + a.ty;
          const RingDistance rd = ring_distance(r.ring, r.n, x - r.first.x, y - r.first.y);
          state = rd.best > far2 ? (rd.inside ? 1 : 0) : 2;
        }
        const unsigned long long filled = __ballot(state == 1);
        tot.filled += (unsigned long long)__popcll(filled);
        for_block_pixels(filled, bx, by, lb, cx, cy, [&](bool valid, int row, int col) {
          if (valid) claim(a, row, col, p);
          covered += (int64_t)__popcll(__ballot(valid));
        });
        for_block_pixels(__ballot(state == 2), bx, by, lb, cx, cy, evaluate);
      }
    }
  }
  if (lane == 0) a.n_covered[p] = covered;
  tot.covered += (unsigned long long)covered;
  tot.empty += covered == 0 ? 1u : 0u;
  tot.clipped += clipped ? 1u : 0u;
}

__device__ __forceinline__ void add_totals(const RasterArgs& a, const WaveTotals& tot) {
  if ((threadIdx.x & (kWave - 1)) != 0) return;
  if (tot.covered) atomicAdd(&a.counters[kCtrOverlaps], tot.covered);      // the finishing pass subtracts n_pixels_set
  if (tot.empty) atomicAdd(&a.counters[kCtrEmpty], tot.empty);
  if (tot.clipped) atomicAdd(&a.counters[kCtrClipped], tot.clipped);
  if (tot.large) atomicAdd(&a.counters[kCtrLarge], tot.large);
  if (tot.filled) atomicAdd(&a.counters[kCtrFilled], tot.filled);
}

__global__ __launch_bounds__(kRsThreads) void raster_short_kernel(RasterArgs a, const int32_t* __restrict__ list) {
  WaveTotals tot;
  short_ring_loop(a.off, a.xy, a.words, list, kRsWaves, [&](const auto& r) { raster_body(r, a, tot); });
  add_totals(a, tot);
}

__global__ __launch_bounds__(kWave) void raster_long_kernel(RasterArgs a, const int32_t* __restrict__ list) {
  __shared__ double2 pts[SEGGER_MORPH_MAX_VERTS];
  WaveTotals tot;
  long_ring_loop(a.off, a.xy, a.words, list, pts, [&](const auto& r) {
    raster_body(r, a, tot);
    tot.large += 1u;
  });
  add_totals(a, tot);
}

// ---------------------------------------------------------------- the finishing pass ---
// One thread per pixel, whole waves together: polygon index -> label (labels == NULL: index + 1), 0 where nothing claimed
// the pixel.  n_won: a run of equal indices among the wave's 64 consecutive pixels is one int64 atomic, added by the run's
// first lane, so a large polygon does not serialise on its counter pixel by pixel.
__global__ __launch_bounds__(kRsThreads) void raster_finish_kernel(int32_t* __restrict__ image, int64_t n_pixels,
                                                                    const int32_t* __restrict__ labels,
                                                                    unsigned long long* __restrict__ n_won,
                                                                    unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kRsThreads;
  unsigned long long set = 0;                                        // the same in every lane
  for (int64_t base = (int64_t)blockIdx.x * kRsThreads + (threadIdx.x & ~(kWave - 1)); base < n_pixels; base += stride) {
    const int64_t i = base + lane;
    const int v = i < n_pixels ? image[i] : -1;                      // -1: unclaimed under either rule, or beyond the end
    if (i < n_pixels) image[i] = v < 0 ? 0 : (labels ? labels[v] : v + 1);
    const int before = __shfl_up(v, 1, kWave);
    const unsigned long long heads = __ballot(lane == 0 || v != before);
    if (((heads >> lane) & 1) && v >= 0) {
      const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
      const int len = above ? (int)__builtin_ctzll(above) + 1 : kWave - lane;
      atomicAdd(&n_won[v], (unsigned long long)len);
    }
    set += (unsigned long long)__popcll(__ballot(v >= 0));
  }
  if (lane == 0 && set) {
    atomicAdd(&counters[kCtrSet], set);
    atomicAdd(&counters[kCtrOverlaps], 0ull - set);                  // n_overlaps = sum n_covered - n_pixels_set
  }
}

// ---------------------------------------------------------------- host ---
struct RsLayout { RingLists rings; size_t total; };
RsLayout rs_layout(int64_t P) {
  Carver c;
  RsLayout l;
  l.rings = take_ring_lists(c, P);
  l.total = c.total();
  return l;
}

int rs_check_polygons(const char* who, int64_t P) {
  SEGGER_REQUIRE(P >= 0, "%s: negative n_polygons", who);
  SEGGER_REQUIRE(P < 0x7fffffffLL, "%s: 2^31 - 1 polygons, or more", who);
  return SEGGER_OK;
}

bool is_finite(double v) { return v - v == 0.0; }

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_rasterize_workspace_bytes(int64_t n_polygons) {
  const int rc = rs_check_polygons("segger_rasterize_workspace_bytes", n_polygons);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)rs_layout(n_polygons).total;
}

extern "C" int segger_rasterize_rings(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                      const int32_t* labels, int32_t height, int32_t width, double sx, double sy, double tx,
                                      double ty, int32_t predicate, int32_t overlap, int32_t block, int32_t reg_max,
                                      int32_t* image, int64_t* n_covered, int64_t* n_won, int64_t* counters, void* workspace,
                                      int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_rasterize_rings";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rs_check_polygons(who, n_polygons);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(n_vertices >= 0, "%s: negative n_vertices", who);
  SEGGER_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", who);
  SEGGER_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= 0x7fffffffLL,
                 "%s: bad shape: height, width >= 1 and height * width < 2^31", who);
  SEGGER_REQUIRE(is_finite(sx) && is_finite(sy) && sx != 0.0 && sy != 0.0 && is_finite(tx) && is_finite(ty),
                 "%s: bad frame: the scale must be finite and non-zero and the translation finite", who);
  SEGGER_REQUIRE(predicate == SEGGER_RASTER_CONTAINS || predicate == SEGGER_RASTER_INTERSECTS,
                 "%s: predicate %d is neither SEGGER_RASTER_CONTAINS nor SEGGER_RASTER_INTERSECTS", who, (int)predicate);
  SEGGER_REQUIRE(overlap == SEGGER_RASTER_LOWEST || overlap == SEGGER_RASTER_HIGHEST,
                 "%s: overlap %d is neither SEGGER_RASTER_LOWEST nor SEGGER_RASTER_HIGHEST", who, (int)overlap);
  SEGGER_REQUIRE(block >= 1 && block <= SEGGER_RASTER_MAX_BLOCK && (block & (block - 1)) == 0,
                 "%s: block %d is no power of two in 1 .. SEGGER_RASTER_MAX_BLOCK = %d", who, (int)block, SEGGER_RASTER_MAX_BLOCK);
  SEGGER_REQUIRE(reg_max == 0 || reg_max == kWave, "%s: reg_max %d is neither 0 nor 64", who, (int)reg_max);
  if (n_polygons == 0) return SEGGER_OK;                             // nothing is written: the image is all background
  const RsLayout l = rs_layout(n_polygons);
  const int rc2 = check_ring_call(who, ring_offsets, xy, n_vertices, workspace, workspace_bytes, l.total,
                                  OtherPointers{image && n_covered && n_won && counters,
                                                is_aligned(n_covered, 8) && is_aligned(n_won, 8) && is_aligned(counters, 8), true,
                                                "ring_offsets, n_covered, n_won and counters", "xy"});
  if (rc2 != SEGGER_OK) return rc2;
  SEGGER_REQUIRE(is_aligned(image, 4) && is_aligned(labels, 4), "%s: image and labels must be 4-byte aligned", who);

  int log2_block = 0;
  while ((1 << log2_block) < block) ++log2_block;
  RasterArgs a{};
  a.off = ring_offsets;
  a.xy = xy;
  a.words = at<int32_t>(workspace, l.rings.words);
  a.H = height; a.W = width;
  a.sx = sx; a.sy = sy; a.tx = tx; a.ty = ty;
  a.inv_sx = 1.0 / sx; a.inv_sy = 1.0 / sy;
  a.half_diag = 0.5 * (double)(block - 1) * sqrt(sx * sx + sy * sy);
  a.pad = 4.0 * (fabs(sx) + fabs(sy)) + 4.0 * a.half_diag + fmax(fabs(tx), fabs(ty));
  a.predicate = predicate;
  a.highest = overlap == SEGGER_RASTER_HIGHEST;
  a.log2_block = log2_block;
  a.image = image;
  a.n_covered = n_covered;
  a.counters = reinterpret_cast<unsigned long long*>(counters);
  int32_t* list_short = at<int32_t>(workspace, l.rings.list_short);
  int32_t* list_long = at<int32_t>(workspace, l.rings.list_long);
  const int64_t n_pixels = (int64_t)height * width;
  const int cus = cu_count_or_default();

  SEGGER_HIP(hipMemsetAsync(a.words, 0, kRingWordsBytes, stream));
  SEGGER_HIP(hipMemsetAsync(counters, 0, SEGGER_RASTER_COUNTERS * sizeof(int64_t), stream));
  SEGGER_HIP(hipMemsetAsync(image, 0xff, (size_t)n_pixels * sizeof(int32_t), stream));
  hipLaunchKernelGGL(raster_bin_kernel, dim3(grid_stride_blocks(n_polygons, kRsThreads, (int64_t)cus * 8)), dim3(kRsThreads), 0, stream,
                     ring_offsets, xy, n_polygons, n_vertices, (int)reg_max, n_covered, n_won, a.counters, a.words, list_short, list_long);
  SEGGER_LAUNCH_CHECK("raster_bin_kernel");
  hipLaunchKernelGGL(raster_short_kernel, dim3(grid_stride_blocks(n_polygons, kRsWaves, (int64_t)cus * 8)), dim3(kRsThreads), 0, stream,
                     a, (const int32_t*)list_short);
  SEGGER_LAUNCH_CHECK("raster_short_kernel");
  hipLaunchKernelGGL(raster_long_kernel, dim3(grid_stride_blocks(n_polygons, 1, (int64_t)cus * 2)), dim3(kWave), 0, stream, a,
                     (const int32_t*)list_long);
  SEGGER_LAUNCH_CHECK("raster_long_kernel");
  hipLaunchKernelGGL(raster_finish_kernel, dim3(grid_stride_blocks(n_pixels, kRsThreads, (int64_t)cus * 32)), dim3(kRsThreads), 0, stream,
                     image, n_pixels, labels, reinterpret_cast<unsigned long long*>(n_won), a.counters);
  SEGGER_LAUNCH_CHECK("raster_finish_kernel");
  return SEGGER_OK;
}
