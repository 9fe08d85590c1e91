// The predicate of the points-in-buffered-polygons units, once (polygon_join.hip, buffered_counts.hip,
// nearest_boundaries.hip; included after rings.h): what one point is to one ring grown by d, which grid cells a wave has
// to walk to meet every point that can match, and the walk itself (walk_grown_ring).  include/segger_amd.h
// (segger_polygon_join_*) has the definition; all units run THIS code, so a pair is in the join's list exactly when it is
// in the count matrix and among the candidates of the nearest boundaries, bit for bit, and a fix is made here and nowhere
// else.  The walk is here and not in a header of its own because the rounding margin of grown_cell_range is an argument
// about the cells the walk visits: the two are one claim and are read, and changed, together.
//
// Floating point: `#pragma clang fp contract(off)`, as rings.h sets it, to the end of the including unit: the cross product
// of coordinates that are exact after the translation must stay exact.
#pragma once
#include <math.h>

#include "rings.h"

#pragma clang fp contract(off)

namespace segger {

// What is the point (px, py) -- translated to the ring's first vertex, as the ring's n >= 3 vertices are -- to the ring, and
// is it in the ring grown by d, dd = d * d?  Every lane evaluates its own point over the same edges (ring.uni): crossing parity with the half-open
// rule and the smallest squared distance to a closed edge.  Per edge (a, b) and point t:  e = b - a, w = t - a,
// cr = e.x w.y - e.y w.x, dot = w.e, len2 = e.e;  dist2 = |w|^2 if dot <= 0 or len2 == 0, |t - b|^2 if dot >= len2,
// cr cr / len2 otherwise.
// ring_distance returns the two numbers, ring_decide folds them into the predicate's answer; the walk below hands both to
// its visitor: the join and the counts keep the answer, nearest_boundaries.hip the numbers as well.
struct RingDistance { bool inside; double best; };                   // crossing parity, smallest squared distance

template <class Ring>
__device__ __forceinline__ RingDistance ring_distance(const Ring& ring, int n, double px, double py) {
  bool inside = false;
  double best = INFINITY;
  P2 va = ring.uni(0);
  for (int j = 0; j < n; ++j) {
    const P2 vb = ring.uni(j + 1 == n ? 0 : j + 1);
    const double ex = vb.x - va.x, ey = vb.y - va.y;
    const double wx = px - va.x, wy = py - va.y;
    const double cr = ex * wy - ey * wx;
    const double dot = wx * ex + wy * ey;
    const double len2 = ex * ex + ey * ey;
    const bool a_below = va.y <= py, b_below = vb.y <= py;           // the half-open rule
    inside ^= (a_below && !b_below && cr > 0.0) || (!a_below && b_below && cr < 0.0);
    double d2;
    if (dot <= 0.0 || len2 == 0.0) d2 = wx * wx + wy * wy;
    else if (dot >= len2) {
      const double ux = px - vb.x, uy = py - vb.y;
      d2 = ux * ux + uy * uy;
    } else d2 = cr * cr / len2;
    best = fmin(best, d2);
    va = vb;
  }
  return RingDistance{inside, best};
}

// the predicate on the two numbers: dd = d * d
__device__ __forceinline__ bool ring_decide(const RingDistance& r, double dd, int predicate) {
  return predicate == SEGGER_PJOIN_CONTAINS ? (r.best < dd || (r.inside && r.best > 0.0)) : (r.best <= dd || r.inside);
}

// The cells cx0 .. cx1 x cy0 .. cy1 that overlap a ring's bounds (on the coordinates as given, the same in every lane)
// grown by d.  Every matching point has dist2 <= d^2 or lies inside the ring, so in exact arithmetic it is within the
// bounds grown by d.  The margin covers the rounding of dist2, of the translation and of the subtraction below (a few ulp
// of the coordinates: 2^-40 of them is four thousand ulp); cell_of is monotone, so a point inside the grown bounds is in a
// walked cell whatever the grid, and the result does not depend on the grid.
// (readfirstlane: the values are the same in every lane already; it tells the compiler so, and the loops become scalar)
struct CellRange { int cx0, cx1, cy0, cy1; };
__device__ __forceinline__ CellRange grown_cell_range(double xmin, double ymin, double xmax, double ymax, double d, const UniformGrid& g) {
  const double m = d + d * 0x1p-20 + 0x1p-40 * fmax(fmax(fabs(xmin), fabs(xmax)), fmax(fabs(ymin), fabs(ymax)));
  CellRange r;
  r.cx0 = __builtin_amdgcn_readfirstlane(cell_of(xmin - m, g.x0, g.inv_cell, g.nx));
  r.cx1 = __builtin_amdgcn_readfirstlane(cell_of(xmax + m, g.x0, g.inv_cell, g.nx));
  r.cy0 = __builtin_amdgcn_readfirstlane(cell_of(ymin - m, g.y0, g.inv_cell, g.ny));
  r.cy1 = __builtin_amdgcn_readfirstlane(cell_of(ymax + m, g.y0, g.inv_cell, g.ny));
  return r;
}

// The walk, one wave, every lane active: the ring (n >= 3 vertices translated to org; xmin .. ymax its bounds on the
// coordinates as given, the same in every lane) grown by d against the cell-ordered points `pts`.  The wave takes the rows
// of the cell range one after the other -- a row of cells is one contiguous span of the points, cell_start[] its ends -- 64
// points a step, one per lane, and calls visit(hit, s, rd) once a step in EVERY lane (a visitor may ballot): s is the
// lane's position in cell order, rd what its point is to the ring, hit whether s is a point of the span and the predicate
// holds.  In a lane beyond the span's end hit is false and s and rd mean nothing.
template <class Ring, class Visit>
__device__ __forceinline__ void walk_grown_ring(const Ring& ring, int n, P2 org, double xmin, double ymin, double xmax, double ymax,
                                                double d, int predicate, const UniformGrid& g, const int32_t* __restrict__ cell_start,
                                                const double2* __restrict__ pts, Visit&& visit) {
  const int lane = threadIdx.x & (kWave - 1);
  const double dd = d * d;
  const CellRange r = grown_cell_range(xmin, ymin, xmax, ymax, d, g);
  for (int cy = r.cy0; cy <= r.cy1; ++cy) {
    const int64_t row = (int64_t)cy * g.nx;
    const int s0 = __builtin_amdgcn_readfirstlane(cell_start[row + r.cx0]);
    const int s1 = __builtin_amdgcn_readfirstlane(cell_start[row + r.cx1 + 1]);
    for (int sb = s0; sb < s1; sb += kWave) {
      const int s = sb + lane;
      const bool valid = s < s1;
      const double2 t = pts[valid ? s : s0];
      // The edge loop runs under the span's mask, as the join and the counts ran it before the walk was lifted
      // (`valid && ring_match(...)` short-circuits); the nearest boundaries evaluated every lane on pts[s0] and masked
      // afterwards.  One walk has one form, and this is the one of the two older, hotter units: a padding lane then
      // never takes a branch of the distance of its own.  uni() reads lanes or LDS whatever EXEC is.
      RingDistance rd{false, INFINITY};
      if (valid) rd = ring_distance(ring, n, t.x - org.x, t.y - org.y);
      visit(valid && ring_decide(rd, dd, predicate), s, rd);
    }
  }
}

}  // namespace segger
