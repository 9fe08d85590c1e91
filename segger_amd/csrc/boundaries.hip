// segger_cell_boundaries: one boundary polygon per segmented cell, the convex hull of the cell's transcripts, optionally
// rounded by Chaikin corner cutting -- the reference's generate_boundaries with method="convex_hull"
// (src/segger/export/boundary.py:157-217; the default method, "delaunay", is segger_cell_outlines in outlines.hip).
// include/segger_amd.h has the contract.  The output is a ring CSR that segger_polygon_props and segger_polygon_join_* take as it is.
//
// Kernels and library calls on one stream, no host synchronisation (every size after the keys is a device counter; the keys,
// scan and emit kernels are cell_rings.h's, shared with outlines.hip and outlines_large.hip, and so is the host code that
// lays out the head of the workspace, refuses a call and launches the front and the back; here: the bin and hull kernels):
//   bnd_keys_kernel    one thread per row: key = cell << 32 | row for a counted row, the sentinel n_cells << 32 otherwise;
//   (rocprim keys sort: stable by construction, the row is part of the key; rocprim select: the first sorted position of
//   every present cell)
//   bnd_bin_kernel     one thread per present cell: its length, its route (rings.h: append_by_route for the two ring
//                      routes, one integer atomic per cell for the rare chunked one);
//   bnd_short_kernel   n <= 64: one wave per cell, point `lane` in registers, no LDS;
//   bnd_long_kernel    64 < n <= SEGGER_MORPH_MAX_VERTS: one single-wave workgroup per cell, the points in LDS (64 KB);
//   bnd_chunk_kernel   above that: the same body, round after round: hull what is staged, reload the hull to the front of
//                      LDS, stage the next points behind it;
//   bnd_scan_kernel    one workgroup: the cells with h >= 3, their output positions and ring offsets, K and V;
//   bnd_emit_kernel<S> one wave per kept cell: the ring, after S Chaikin iterations.
// The march (march_start, march_step) is rings.h's, the one morphology.hip runs over a ring's vertices.  A hull kernel
// writes hull vertex k of a cell to slot k of the cell's own segment of a scratch array (h <= n: there is room); that is
// also where the chunked route reads its running hull back from.  The points are gathered through the sorted keys as
// they are staged, once each; no sorted copy of the coordinates exists.
//
// Arithmetic: float64, FMA contraction off (rings.h).  The march subtracts the current vertex from the coordinates as
// given -- no translation, so a hull vertex is an input coordinate bit for bit (-0.0 read as +0.0) -- and its cross
// products are exact for integer coordinates below 2^25.  No floating-point atomics; a list's order depends on the order
// of the atomics, a cell's ring does not.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel of the unit, the library's
// included (the sort is instantiated with NoScratchSortConfig); bnd_long_kernel and bnd_chunk_kernel hold 65536 B of LDS,
// two single-wave workgroups per CU.
#include <math.h>

#include "common.h"
#include "post_common.h"
#include "rings.h"
#include "sort_config.h"
#include "cell_rings.h"

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kBndCap = SEGGER_MORPH_MAX_VERTS;                      // points in LDS
constexpr int kWordChunk = 3;                                        // the third list's length, after rings.h's words

static_assert(SEGGER_BOUNDARY_CHUNK_MAX_HULL < kBndCap, "a round of the chunked route must stage at least one new point");

// counters block of segger_cell_boundaries (cell_rings.h names the words)
static_assert(kRefusedCell + 1 == SEGGER_BOUNDARY_COUNTERS, "the header documents the block");

// ---------------------------------------------------------------- routes ---
__global__ __launch_bounds__(kBndThreads) void bnd_bin_kernel(BndSegs s, const unsigned long long* __restrict__ counters,
                                                              int32_t* __restrict__ words, int32_t* __restrict__ list_short,
                                                              int32_t* __restrict__ list_long, int32_t* __restrict__ list_chunk) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t present = (int64_t)counters[kPresent];
  const int32_t n_counted = (int32_t)counters[kCounted];
  const int64_t stride = (int64_t)gridDim.x * kBndThreads;
  // whole waves iterate together: append_by_route needs every lane of a wave in the loop
  for (int64_t base = (int64_t)blockIdx.x * kBndThreads + (threadIdx.x & ~(kWave - 1)); base < present; base += stride) {
    const int64_t j = base + lane;
    int route = -1;
    if (j < present) {
      const int32_t n = (j + 1 < present ? s.head[j + 1] : n_counted) - s.head[j];
      s.len[j] = n;
      route = n > kBndCap ? 2 : ring_route(n);
      if (route == 2) list_chunk[atomicAdd(&words[kWordChunk], 1)] = (int32_t)j;
    }
    append_by_route(route, j, words, list_short, list_long);
  }
}

// ---------------------------------------------------------------- the hull of one cell, one wave ---
// The march over the m points of a store: hull vertex k goes to out[k]; returns h <= m.  Lane 0 writes: the vertex is the
// same in every lane.
template <class Ring>
__device__ __forceinline__ int march_to(const Ring& ring, int m, double2* out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int start = march_start(ring, m);
  int h = 0;
  int cur = start;
  for (int step = 0; step < m; ++step) {
    const P2 p = ring.uni(cur);
    if (lane == 0) out[h] = double2{p.x, p.y};
    ++h;
    const Cand best = march_step(ring, m, p);
    if (best.i < 0 || best.i == start) break;
    cur = best.i;
  }
  return h;
}

__global__ __launch_bounds__(kBndThreads) void bnd_short_kernel(const double* __restrict__ xy, BndSegs s,
                                                                const int32_t* __restrict__ words, const int32_t* __restrict__ list) {
  const int lane = threadIdx.x & (kWave - 1);
  const int count = words[kWordShort];
  const int n_waves = (int)gridDim.x * kBndWaves;
  for (int w = (int)blockIdx.x * kBndWaves + (int)(threadIdx.x >> 6); w < count; w += n_waves) {               // wave-uniform
    const int j = list[w];
    const int64_t b = s.head[j];
    const int n = __builtin_amdgcn_readfirstlane(s.len[j]);          // 1 .. 64
    const P2 mine = point_at(xy, s.keys, b + (lane < n ? lane : 0)); // the lanes beyond n: a copy that never competes
    const RegRing ring{mine.x, mine.y};
    const int h = march_to(ring, n, s.hull + b);
    if (lane == 0) s.hull_n[j] = h;
  }
}

// One cell in LDS, n > 64 points.  n <= kBndCap is one round.  Beyond that, round after round: the hull of what is staged
// goes to the cell's slots of s.hull, comes back to the front of pts, and the next kBndCap - h points are staged behind it.
// The running hull never loses a vertex of the final one, so the last round's hull is the cell's.  A workgroup is one wave.
__device__ __forceinline__ void lds_cell(const double* __restrict__ xy, const BndSegs& s, int j, double2* __restrict__ pts,
                                         unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = s.head[j];
  const int n = __builtin_amdgcn_readfirstlane(s.len[j]);
  double2* out = s.hull + b;
  const LdsRing ring{pts};
  int h = 0, consumed = 0;
  while (true) {
    const int take = min(kBndCap - h, n - consumed);
    __syncthreads();                                                 // the previous round's (or cell's) readers are done
    for (int k = lane; k < h; k += kWave) pts[k] = out[k];           // written by this wave before the barrier
    for (int k = lane; k < take; k += kWave) {
      const P2 p = point_at(xy, s.keys, b + consumed + k);
      pts[h + k] = double2{p.x, p.y};
    }
    __syncthreads();
    h = march_to(ring, h + take, out);
    consumed += take;
    if (consumed >= n) break;
    if (h > SEGGER_BOUNDARY_CHUNK_MAX_HULL) {                        // no room to make progress: refuse the cell
      if (lane == 0) {
        atomicAdd(counters + kRefused, 1ull);
        atomicMax(counters + kRefusedCell, (s.keys[b] >> 32) + 1ull);
      }
      h = 0;
      break;
    }
  }
  if (lane == 0) s.hull_n[j] = h;
}

__global__ __launch_bounds__(kWave) void bnd_long_kernel(const double* __restrict__ xy, BndSegs s, const int32_t* __restrict__ words,
                                                         const int32_t* __restrict__ list, unsigned long long* __restrict__ counters) {
  __shared__ double2 pts[kBndCap];
  const int count = words[kWordLong];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) lds_cell(xy, s, list[w], pts, counters);
}

__global__ __launch_bounds__(kWave) void bnd_chunk_kernel(const double* __restrict__ xy, BndSegs s, const int32_t* __restrict__ words,
                                                          const int32_t* __restrict__ list, unsigned long long* __restrict__ counters) {
  __shared__ double2 pts[kBndCap];
  const int count = words[kWordChunk];
  for (int w = (int)blockIdx.x; w < count; w += (int)gridDim.x) lds_cell(xy, s, list[w], pts, counters);
}

// ---------------------------------------------------------------- host ---
// cell_rings.h's head, then the list of the chunked route: a cell of it has more than kBndCap rows
struct BndLayout { CellRingsLayout head; size_t list_chunk, total; };

BndLayout bnd_layout(int64_t n_rows, int64_t n_cells) {
  BndLayout l;
  Carver c;
  l.head = take_cell_rings(c, n_rows, n_cells);
  l.list_chunk = c.take(((size_t)(n_rows > 0 ? n_rows : 1) / (kBndCap + 1) + 1) * 4);
  l.total = c.total();
  return l;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_cell_boundaries_workspace_bytes(int64_t n_rows, int64_t n_cells) {
  const int rc = bnd_check_sizes("segger_cell_boundaries_workspace_bytes", n_rows, n_cells);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)bnd_layout(n_rows, n_cells).total;
}

extern "C" int segger_cell_boundaries(const double* xy, const int32_t* cell, const uint8_t* keep, int64_t n_rows, int64_t n_cells,
                                      int32_t smoothing, int64_t* ring_offsets, double* xy_out, int64_t xy_capacity,
                                      int32_t* cell_ids, int64_t* n_transcripts, uint64_t* counters, void* workspace,
                                      int64_t workspace_bytes, segger_stream_t stream_) {
  const char* who = "segger_cell_boundaries";
  hipStream_t stream = (hipStream_t)stream_;
  const CellRingsCall a{xy, cell, keep, n_rows, n_cells, smoothing, ring_offsets, xy_out, xy_capacity, cell_ids, n_transcripts,
                        counters, workspace, workspace_bytes};
  int rc = bnd_check_sizes(who, n_rows, n_cells);
  if (rc != SEGGER_OK) return rc;
  const BndLayout l = bnd_layout(n_rows, n_cells);
  bool empty = false;
  rc = check_cell_rings_call(who, a, l.total, [] { return SEGGER_OK; }, &empty);
  if (rc != SEGGER_OK || empty) return rc;

  const CellRingsViews v = cell_rings_views(a, l.head);
  int32_t* list_chunk = at<int32_t>(workspace, l.list_chunk);
  const BndSegs& s = v.s;
  const int cus = cu_count_or_default();
  const int64_t cap = l.head.cells_cap;

  rc = launch_cell_rings_front(a, l.head, v, SEGGER_BOUNDARY_COUNTERS, cus, stream);
  if (rc != SEGGER_OK) return rc;
  hipLaunchKernelGGL(bnd_bin_kernel, dim3(grid_stride_blocks(cap, kBndThreads, (int64_t)cus * 8)), dim3(kBndThreads), 0, stream, s,
                     (const unsigned long long*)v.cnt, v.words, v.list_short, v.list_long, list_chunk);
  SEGGER_LAUNCH_CHECK("bnd_bin_kernel");
  hipLaunchKernelGGL(bnd_short_kernel, dim3(grid_stride_blocks(cap, kBndWaves, (int64_t)cus * 8)), dim3(kBndThreads), 0, stream, xy, s,
                     (const int32_t*)v.words, (const int32_t*)v.list_short);
  SEGGER_LAUNCH_CHECK("bnd_short_kernel");
  hipLaunchKernelGGL(bnd_long_kernel, dim3(grid_stride_blocks(ceil_div(n_rows, kWave + 1), 1, (int64_t)cus * 2)), dim3(kWave), 0,
                     stream, xy, s, (const int32_t*)v.words, (const int32_t*)v.list_long, v.cnt);
  SEGGER_LAUNCH_CHECK("bnd_long_kernel");
  hipLaunchKernelGGL(bnd_chunk_kernel, dim3(grid_stride_blocks(n_rows / (kBndCap + 1), 1, (int64_t)cus * 2)), dim3(kWave), 0, stream,
                     xy, s, (const int32_t*)v.words, (const int32_t*)list_chunk, v.cnt);
  SEGGER_LAUNCH_CHECK("bnd_chunk_kernel");
  return launch_cell_rings_back(a, l.head, v, cus, stream);
}
