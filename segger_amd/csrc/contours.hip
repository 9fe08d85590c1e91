// segger_label_contours: boundary polygons from a label image -- per label the border with the most vertices, as the ring
// CSR the morphology and polygon-join units read.  The reference's masks_to_contours (src/segger/io/utils.py:8-41) driven by
// its CosMx intake (src/segger/io/cosmx.py:79-107), with np.where(np.isin(compartment, codes), labels, 0) fused into the
// read.  include/segger_amd.h has the contract; DESIGN.md 3.5l the reasoning.  Integer-only up to the final conversion.
//
// The frame.  The reference hands cv2 the transposed crop, so the raster scan runs x-major: "row" = x, "column" = y.  The
// eight directions are numbered counter-clockwise in that frame from "column - 1":
//     c        0   1   2   3   4   5   6   7
//     (dx,dy) 0,-1 1,-1 1,0 1,1 0,1 -1,1 -1,0 -1,-1
// A STATE is (pixel p, direction c of the pixel the chain came from).  Its successor: sweep the neighbours of p
// counter-clockwise from c + 1; the first foreground neighbour, in direction e, is the next pixel, and the new state is
// (p + e, e + 4).  This map is a bijection on states, so the states fall into cycles; the cycles in which some sweep passes
// over a background 4-neighbour are the borders of Suzuki and Abe's border following with 8-connected foreground, outer
// and hole borders alike, each exactly once.  Every border has a state whose sweep passes over a background pixel in
// direction 0 (an outer border at its first pixel of the scan, a hole border right of the hole's last pixel), and a pixel
// has at most one such state: these are the CANDIDATES, one per pixel that has background at "column - 1".
//
//   ct_scan_kernel   pass A, one read of the image (and of the compartment plane): per label the bounding box and the
//                    pixel count.  Runs of equal labels inside a wave are folded before the integer atomics.
//   rocprim::select  the present labels, ascending.
//   ct_trace_kernel  pass B, one single-wave workgroup per present label.  The crop is staged as a bit mask in LDS when
//                    its padded bits fit lds_max_bits, else the image itself is read (the global route: the same code
//                    over another pixel accessor; a mask in the workspace would need the summed crop areas, which no
//                    bound short of labels x pixels covers).  The lanes collect candidates 64 at a time.  A lane walks
//                    back to the previous candidate of its border and forward to the next: if either has a smaller scan
//                    index the lane gives up (pruning only); otherwise it follows the border and gives up at the first
//                    smaller candidate, so exactly the smallest candidate of a border completes the cycle.  On the way
//                    it counts the kept points (CHAIN_APPROX_SIMPLE: the step in differs from the step out) and finds
//                    the canonical start, the smallest (scan index, clockwise code of the previous pixel).  The winner:
//                    most kept points, then the smaller canonical start.
//   ct_offsets_kernel  one workgroup: the labels with more than 2 points, compacted; ring_offsets; the counters (the scan
//                      of vertices and kept labels is post_common.h's GroupScan; the longest ring is a maximum beside it).
//   ct_emit_kernel   one thread per kept label follows the winner from its canonical start over the image and writes xy.
// Nothing depends on the order in which threads arrive: atomics are integer min, max and add.
// Every loop is bounded before it is entered: a border has at most 8 states per pixel of the crop.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel; ct_trace_kernel 4608 B of LDS.
#include "common.h"
#include "post_common.h"

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#pragma clang fp contract(off)

namespace segger {
namespace {

constexpr int kCtThreads = 256, kCtOffThreads = 1024, kCtOffWaves = kCtOffThreads / kWave;
constexpr int kCtLdsWords = SEGGER_CONTOUR_LDS_BITS / 32;
constexpr int kCtQueue = 2 * kWave;
enum { kCtPresent = 0, kCtKept, kCtVertices, kCtDropped, kCtBorders, kCtLongest, kCtTies, kCtBadLabel, kCtOverflow, kCtGlobal };
static_assert(kCtGlobal + 1 == SEGGER_CONTOUR_COUNTERS, "the header documents the block");

struct CtImage {
  const int32_t* labels;
  const uint8_t* comp;                                               // or NULL
  unsigned long long v0, v1, v2, v3;                                 // the valid compartment codes, bit c of 256
  int W, H;
};

struct CtTables { int32_t *minx, *miny, *maxx, *maxy, *count; };

// per present label j: the winner's kept points and canonical start state
struct CtWinners { int32_t *present, *cnt, *sx, *sy, *sprev; };

__device__ __forceinline__ int ct_label(const CtImage& im, int64_t i) {
  int l = im.labels[i];
  if (im.comp) {
    const unsigned c = im.comp[i];
    // all four words are read and masked: a select among them would become an indexed read of a copy in scratch
    const unsigned s = c & 63u, q = c >> 6;
    const unsigned long long w = ((im.v0 >> s) & (unsigned long long)(q == 0)) | ((im.v1 >> s) & (unsigned long long)(q == 1)) |
                                 ((im.v2 >> s) & (unsigned long long)(q == 2)) | ((im.v3 >> s) & (unsigned long long)(q == 3));
    if (!(w & 1ull)) l = 0;
  }
  return l;
}

__device__ __forceinline__ int ct_dx(int c) { return (int)((0x01A9u >> (2 * c)) & 3u) - 1; }
__device__ __forceinline__ int ct_dy(int c) { return (int)((0x1A90u >> (2 * c)) & 3u) - 1; }

// ---------------------------------------------------------------- pass A ---
__global__ __launch_bounds__(kCtThreads) void ct_scan_kernel(CtImage im, int64_t n_pix, int32_t max_label, CtTables t,
                                                             unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kCtThreads;
  for (int64_t base = (int64_t)blockIdx.x * kCtThreads + (threadIdx.x & ~(kWave - 1)); base < n_pix; base += stride) {
    const int64_t i = base + lane;
    int lab = i < n_pix ? ct_label(im, i) : 0;
    if (lab < 0 || lab > max_label) { atomicAdd(counters + kCtBadLabel, 1ull); lab = 0; }
    const int b = __builtin_amdgcn_readfirstlane((int)base);         // n_pix < 2^31
    int y = b / im.W, x = b - y * im.W + lane;
    while (x >= im.W) { x -= im.W; ++y; }
    const int left = __shfl_up(lab, 1, kWave);
    const bool brk = lane == 0 || x == 0 || left != lab;             // a run of one label in one row starts here
    const unsigned long long breaks = __ballot(brk);
    if (brk && lab != 0) {
      const unsigned long long rest = lane == kWave - 1 ? 0ull : breaks >> (lane + 1);
      const int len = rest ? (int)__builtin_ctzll(rest) + 1 : kWave - lane;
      atomicMin(t.minx + lab, x);
      atomicMax(t.maxx + lab, x + len - 1);
      atomicMin(t.miny + lab, y);
      atomicMax(t.maxy + lab, y);
      atomicAdd(t.count + lab, len);
    }
  }
}

struct CtIsPresent {
  const int32_t* count;
  __device__ bool operator()(int32_t l) const { return count[l] > 0; }
};

// ---------------------------------------------------------------- the crop of one label ---
struct CtCrop { int x0, y0, cw, ch; };

struct CtLdsMask {                                                   // bit (yy, xx) at word yy * stride + xx / 32
  const uint32_t* words;
  int stride, cw, ch;
  __device__ __forceinline__ bool fg(int xx, int yy) const {
    if ((unsigned)xx >= (unsigned)cw || (unsigned)yy >= (unsigned)ch) return false;
    return (words[yy * stride + (xx >> 5)] >> (xx & 31)) & 1u;
  }
};

struct CtImageMask {                                                 // the image itself; the crop lies inside it
  CtImage im;
  int label, x0, y0, cw, ch;
  __device__ __forceinline__ bool fg(int xx, int yy) const {
    if ((unsigned)xx >= (unsigned)cw || (unsigned)yy >= (unsigned)ch) return false;
    return ct_label(im, (int64_t)(y0 + yy) * im.W + (x0 + xx)) == label;
  }
};

// one state and its sweep: e the direction of the next pixel, k how far the sweep went (1 .. 8)
template <typename M>
__device__ __forceinline__ void ct_sweep(const M& m, int x, int y, int prev, int& e, int& k) {
  e = prev; k = 8;                                                   // the previous pixel is foreground: the sweep ends there at the latest
#pragma unroll
  for (int q = 1; q < 8; ++q) {
    const int c = (prev + q) & 7;
    if (k == 8 && m.fg(x + ct_dx(c), y + ct_dy(c))) { e = c; k = q; }
  }
}

// does the sweep of (prev, k) pass over direction 0?  Then the pixel there is background and this state is a candidate.
__device__ __forceinline__ bool ct_over_zero(int prev, int k) {
  const int k0 = (8 - prev) & 7;
  return k0 != 0 && k0 < k;
}

struct CtBest {
  int cnt;
  unsigned long long key;
  int tie;
};

__device__ __forceinline__ void ct_merge(CtBest& a, int cnt, unsigned long long key, int tie) {
  if (cnt > a.cnt) { a.cnt = cnt; a.key = key; a.tie = tie; }
  else if (cnt == a.cnt && cnt > 0) { a.tie = 1; if (key < a.key) a.key = key; }
}

// The candidate at (x, y) -- foreground with background in direction 0: if it is the smallest candidate of its border,
// the border's kept points and canonical start go into `best` and 1 is returned; else 0.
template <typename M>
__device__ __forceinline__ int ct_follow(const M& m, int x0, int y0, long long max_steps, CtBest& best) {
  const int ch = m.ch;
  const long long start = (long long)x0 * ch + y0;
  int prev = -1;
#pragma unroll
  for (int q = 7; q >= 1; --q)                                       // clockwise from direction 0: 7, 6, .. 1
    if (prev < 0 && m.fg(x0 + ct_dx(q), y0 + ct_dy(q))) prev = q;
  if (prev < 0) {                                                    // an isolated pixel: one point
    ct_merge(best, 1, (unsigned long long)start << 3, 0);
    return 1;
  }
  const int prev0 = prev;
  // pruning: back to the previous candidate of this border
  {
    int x = x0, y = y0, p = prev0;
    for (long long s = 0; s < max_steps; ++s) {
      // the predecessor of (x, y, p): at q = (x, y) + p, the first foreground clockwise from the direction back here
      const int qx = x + ct_dx(p), qy = y + ct_dy(p), f = (p + 4) & 7;
      int c = f, k = 8;
#pragma unroll
      for (int r = 1; r < 8; ++r) {
        const int d = (f - r) & 7;
        if (k == 8 && m.fg(qx + ct_dx(d), qy + ct_dy(d))) { c = d; k = r; }
      }
      x = qx; y = qy; p = c;
      if (ct_over_zero(p, k)) {
        const long long key = (long long)x * ch + y;
        if (key < start) return 0;
        break;                                                       // itself or a larger one: no verdict
      }
    }
  }
  int x = x0, y = y0, cnt = 0;
  unsigned long long lo = ~0ull;
  for (long long s = 0; s < max_steps; ++s) {
    int e, k;
    ct_sweep(m, x, y, prev, e, k);
    if (ct_over_zero(prev, k)) {
      const long long key = (long long)x * ch + y;
      if (key < start) return 0;
      if (key == start && s > 0) {                                   // closed
        ct_merge(best, cnt, lo, 0);
        return 1;
      }
    }
    cnt += e != ((prev + 4) & 7);
    const unsigned long long st = ((unsigned long long)((long long)x * ch + y) << 3) | (unsigned long long)((8 - prev) & 7);
    lo = st < lo ? st : lo;
    x += ct_dx(e); y += ct_dy(e); prev = (e + 4) & 7;
  }
  return 0;                                                          // not reached: a cycle has at most 8 states per pixel
}

// all borders of one label; every lane of the wave calls this.  queue: kCtQueue ints of LDS.
template <typename M>
__device__ __forceinline__ void ct_label_borders(const M& m, int* queue, CtBest& best, int& borders) {
  const int lane = threadIdx.x;
  const int cw = m.cw, ch = m.ch;
  const long long total = (long long)cw * ch, max_steps = 8 * total + 2;
  int qn = 0;                                                        // below kWave at the top of every trip
  for (long long base = 0; base < total; base += kWave) {
    const long long s = base + lane;
    bool cand = false;
    if (s < total) {
      const int xx = (int)(s / ch), yy = (int)(s - (long long)xx * ch);
      cand = m.fg(xx, yy) && !m.fg(xx, yy - 1);
    }
    const unsigned long long mask = __ballot(cand);
    if (cand) queue[qn + (int)__popcll(mask & ((1ull << lane) - 1ull))] = (int)s;
    qn += (int)__popcll(mask);
    __syncthreads();
    if (qn >= kWave) {                                               // a full wave of candidates
      const int c = queue[lane];
      const int xx = c / ch;
      borders += ct_follow(m, xx, c - xx * ch, max_steps, best);
      const int moved = lane + kWave < qn ? queue[lane + kWave] : 0;
      __syncthreads();
      queue[lane] = moved;
      qn -= kWave;
      __syncthreads();
    }
  }
  if (lane < qn) {
    const int c = queue[lane];
    const int xx = c / ch;
    borders += ct_follow(m, xx, c - xx * ch, max_steps, best);
  }
}

// ---------------------------------------------------------------- pass B ---
__global__ __launch_bounds__(kWave) void ct_trace_kernel(CtImage im, CtTables t, CtWinners w, int lds_words_max,
                                                         unsigned long long* __restrict__ counters) {
  __shared__ uint32_t words[kCtLdsWords];
  __shared__ int queue[kCtQueue];
  const int lane = threadIdx.x;
  const int present = (int)counters[kCtPresent];
  for (int j = (int)blockIdx.x; j < present; j += (int)gridDim.x) {
    const int label = w.present[j];
    const CtCrop c{t.minx[label], t.miny[label], t.maxx[label] - t.minx[label] + 1, t.maxy[label] - t.miny[label] + 1};
    const int stride = (c.cw + 31) >> 5;
    const long long need = (long long)stride * c.ch;
    CtBest best{0, ~0ull, 0};
    int borders = 0;
    __syncthreads();                                                 // the previous label's readers are done
    if (need <= (long long)lds_words_max) {
      const int per_row = (c.cw + kWave - 1) / kWave;
      for (int u = 0; u < per_row * c.ch; ++u) {
        const int row = u / per_row, part = u - row * per_row;
        const int xx = part * kWave + lane;
        const bool on = xx < c.cw && ct_label(im, (int64_t)(c.y0 + row) * im.W + (c.x0 + xx)) == label;
        const unsigned long long bits = __ballot(on);
        if (lane == 0) words[row * stride + 2 * part] = (uint32_t)bits;
        if (lane == 1 && 2 * part + 1 < stride) words[row * stride + 2 * part + 1] = (uint32_t)(bits >> 32);
      }
      __syncthreads();
      const CtLdsMask m{words, stride, c.cw, c.ch};
      ct_label_borders(m, queue, best, borders);
    } else {
      const CtImageMask m{im, label, c.x0, c.y0, c.cw, c.ch};
      ct_label_borders(m, queue, best, borders);
      if (lane == 0) atomicAdd(counters + kCtGlobal, 1ull);
    }
    // the wave's winner: most points, then the smaller canonical start
#pragma unroll
    for (int q = 1; q < kWave; q <<= 1) {
      const int oc = __shfl_xor(best.cnt, q, kWave), ot = __shfl_xor(best.tie, q, kWave);
      const unsigned long long ok = shfl_xor64(best.key, q);
      ct_merge(best, oc, ok, ot);
    }
    borders = wave_sum_i32(borders);
    if (lane == 0) {
      const long long scan = (long long)(best.key >> 3);
      const int xx = (int)(scan / c.ch);
      w.cnt[j] = best.cnt;
      w.sx[j] = c.x0 + xx;
      w.sy[j] = c.y0 + (int)(scan - (long long)xx * c.ch);
      w.sprev[j] = (8 - (int)(best.key & 7ull)) & 7;
      atomicAdd(counters + kCtBorders, (unsigned long long)borders);
      if (best.tie) atomicAdd(counters + kCtTies, 1ull);
    }
  }
}

// ---------------------------------------------------------------- offsets ---
// One workgroup.  kept[k] = the k-th present label with more than 2 points; the caller's arrays past the kept count and
// the vertices past xy_capacity are never written.
__global__ __launch_bounds__(kCtOffThreads) void ct_offsets_kernel(CtTables t, CtWinners w, int32_t* __restrict__ kept,
                                                                   int64_t* __restrict__ ring_offsets, int32_t* __restrict__ label_ids,
                                                                   int64_t* __restrict__ n_pixels, int64_t xy_capacity,
                                                                   unsigned long long* __restrict__ counters) {
  __shared__ ScanPair totals[kCtOffWaves];
  __shared__ int sl[kCtOffWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int present = (int)counters[kCtPresent];
  GroupScan<kCtOffThreads, ScanPair> scan{totals, ScanPair{0, 0}};   // vertices and kept labels before
  int longest = 0;                                                   // of this thread's labels; combined after the loop
  for (int base = 0; base < present; base += kCtOffThreads) {
    const int j = base + tid;
    const int cnt = j < present ? w.cnt[j] : 0;
    const int keep = cnt > 2;
    longest = max(longest, keep ? cnt : 0);
    const ScanPair before = scan.step(ScanPair{keep ? cnt : 0, keep});
    if (keep) {
      const int at = before.k;
      const int label = w.present[j];
      kept[at] = j;
      ring_offsets[at] = before.v;
      label_ids[at] = label;
      n_pixels[at] = t.count[label];
    }
  }
#pragma unroll
  for (int q = 1; q < kWave; q <<= 1) longest = max(longest, __shfl_xor(longest, q, kWave));
  if (lane == 0) sl[wave] = longest;
  __syncthreads();
  if (tid == 0) {
    for (int q = 0; q < kCtOffWaves; ++q) longest = max(longest, sl[q]);
    const long long v_base = scan.carry.v;
    const int k_base = scan.carry.k;
    ring_offsets[k_base] = v_base;
    counters[kCtKept] = (unsigned long long)k_base;
    counters[kCtVertices] = (unsigned long long)v_base;
    counters[kCtDropped] = (unsigned long long)(present - k_base);
    counters[kCtLongest] = (unsigned long long)longest;
    counters[kCtOverflow] = v_base > xy_capacity ? 1ull : 0ull;
  }
}

// ---------------------------------------------------------------- emit ---
struct CtAffine { double sx, sy, tx, ty; };

__global__ __launch_bounds__(kCtThreads) void ct_emit_kernel(CtImage im, CtWinners w, const int32_t* __restrict__ kept,
                                                             const int64_t* __restrict__ ring_offsets, CtAffine a,
                                                             double2* __restrict__ xy_out, int64_t xy_capacity,
                                                             const unsigned long long* __restrict__ counters) {
  const int n_kept = (int)counters[kCtKept];
  for (int q = (int)(blockIdx.x * kCtThreads + threadIdx.x); q < n_kept; q += (int)(gridDim.x * kCtThreads)) {
    const int j = kept[q];
    const int cnt = w.cnt[j], x0 = w.sx[j], y0 = w.sy[j], prev0 = w.sprev[j];
    const int64_t at0 = ring_offsets[q];
    const CtImageMask m{im, w.present[j], 0, 0, im.W, im.H};
    int x = x0, y = y0, prev = prev0, h = 0;
    const long long max_steps = 8ll * im.W * im.H + 2;
    for (long long s = 0; s < max_steps && h < cnt; ++s) {           // the cycle has exactly cnt kept points
      int e, k;
      ct_sweep(m, x, y, prev, e, k);
      if (e != ((prev + 4) & 7)) {
        if (at0 + h < xy_capacity) xy_out[at0 + h] = double2{(double)x * a.sx + a.tx, (double)y * a.sy + a.ty};
        ++h;
      }
      x += ct_dx(e); y += ct_dy(e); prev = (e + 4) & 7;
    }
  }
}

// ---------------------------------------------------------------- host ---
struct CtLayout {
  size_t minx, miny, maxx, maxy, count, present, cnt, sx, sy, sprev, kept, temp, total;
  size_t temp_bytes;
  int64_t labels_cap;
};

CtLayout ct_layout(int64_t n_pix, int64_t max_label) {
  CtLayout l;
  const size_t table = (size_t)(max_label + 1) * 4;
  l.labels_cap = max_label < n_pix ? max_label : n_pix;
  if (l.labels_cap < 1) l.labels_cap = 1;
  const size_t c4 = (size_t)l.labels_cap * 4;
  Carver c;
  l.minx = c.take(table);
  l.miny = c.take(table);
  l.maxx = c.take(table);
  l.maxy = c.take(table);
  l.count = c.take(table);
  l.present = c.take(c4);
  l.cnt = c.take(c4);
  l.sx = c.take(c4);
  l.sy = c.take(c4);
  l.sprev = c.take(c4);
  l.kept = c.take(c4);
  size_t b = 0;
  int32_t* i32 = nullptr;
  size_t* n = nullptr;
  (void)rocprim::select(nullptr, b, rocprim::counting_iterator<int32_t>(0), i32, n, (size_t)(max_label + 1), CtIsPresent{nullptr},
                        (hipStream_t)0);
  l.temp_bytes = b;
  l.temp = c.take(b > 0 ? b : 1);
  l.total = c.total();
  return l;
}

int ct_check_sizes(const char* who, int64_t height, int64_t width, int64_t max_label) {
  SEGGER_REQUIRE(height >= 0 && width >= 0, "%s: negative height or width", who);
  const int64_t lim = (int64_t)1 << 31;
  SEGGER_REQUIRE(height < lim && width < lim && height * width < lim, "%s: height * width = %lld * %lld is 2^31 or more", who,
                 (long long)height, (long long)width);
  SEGGER_REQUIRE(max_label >= 0 && max_label <= SEGGER_CONTOUR_MAX_LABEL, "%s: max_label = %lld outside 0 .. %d", who,
                 (long long)max_label, SEGGER_CONTOUR_MAX_LABEL);
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_label_contours_workspace_bytes(int64_t height, int64_t width, int64_t max_label) {
  const int rc = ct_check_sizes("segger_label_contours_workspace_bytes", height, width, max_label);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)ct_layout(height * width, max_label).total;
}

extern "C" int segger_label_contours(const int32_t* labels, const uint8_t* compartment, uint64_t valid0, uint64_t valid1,
                                     uint64_t valid2, uint64_t valid3, int64_t height, int64_t width, int64_t max_label,
                                     double scale_x, double scale_y, double trans_x, double trans_y, int64_t* ring_offsets,
                                     double* xy_out, int64_t xy_capacity, int32_t* label_ids, int64_t* n_pixels, uint64_t* counters,
                                     void* workspace, int64_t workspace_bytes, int32_t lds_max_bits, segger_stream_t stream_) {
  const char* who = "segger_label_contours";
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = ct_check_sizes(who, height, width, max_label);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(lds_max_bits >= 0 && lds_max_bits <= SEGGER_CONTOUR_LDS_BITS, "%s: lds_max_bits = %d outside 0 .. %d", who,
                 (int)lds_max_bits, SEGGER_CONTOUR_LDS_BITS);
  SEGGER_REQUIRE(scale_x - scale_x == 0.0 && scale_y - scale_y == 0.0 && trans_x - trans_x == 0.0 && trans_y - trans_y == 0.0,
                 "%s: scale and translation must be finite", who);
  SEGGER_REQUIRE(workspace_bytes >= 0 && xy_capacity >= 0, "%s: negative workspace_bytes or xy_capacity", who);
  const int64_t n_pix = height * width;
  if (n_pix == 0 || max_label == 0) {              // nothing launched: the caller's zeroed counters and ring_offsets[0] stand
    SEGGER_REQUIRE(counters && ring_offsets, "%s: NULL pointer", who);
    return SEGGER_OK;
  }
  SEGGER_REQUIRE(labels && ring_offsets && label_ids && n_pixels && counters && workspace, "%s: NULL pointer", who);
  SEGGER_REQUIRE(xy_out || xy_capacity == 0, "%s: NULL xy_out with xy_capacity > 0", who);
  SEGGER_REQUIRE(is_aligned(xy_out, 16), "%s: xy_out must be 16-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(ring_offsets, 8) && is_aligned(n_pixels, 8) && is_aligned(counters, 8),
                 "%s: ring_offsets, n_pixels and counters must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(labels, 4) && is_aligned(label_ids, 4), "%s: labels and label_ids must be 4-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(workspace, 256), "%s: workspace must be 256-byte aligned", who);
  const CtLayout l = ct_layout(n_pix, max_label);
  SEGGER_REQUIRE((size_t)workspace_bytes >= l.total, "%s: workspace %lld < %zu bytes", who, (long long)workspace_bytes, l.total);

  const CtImage im{labels, compartment, valid0, valid1, valid2, valid3, (int)width, (int)height};
  const CtTables t{at<int32_t>(workspace, l.minx), at<int32_t>(workspace, l.miny), at<int32_t>(workspace, l.maxx),
                   at<int32_t>(workspace, l.maxy), at<int32_t>(workspace, l.count)};
  const CtWinners w{at<int32_t>(workspace, l.present), at<int32_t>(workspace, l.cnt), at<int32_t>(workspace, l.sx),
                    at<int32_t>(workspace, l.sy), at<int32_t>(workspace, l.sprev)};
  int32_t* kept = at<int32_t>(workspace, l.kept);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  const int cus = cu_count_or_default();
  const size_t table = (size_t)(max_label + 1) * 4;

  SEGGER_HIP(hipMemsetAsync(cnt, 0, SEGGER_CONTOUR_COUNTERS * sizeof(unsigned long long), stream));
  SEGGER_HIP(hipMemsetAsync(t.minx, 0x7f, table, stream));
  SEGGER_HIP(hipMemsetAsync(t.miny, 0x7f, table, stream));
  SEGGER_HIP(hipMemsetAsync(t.maxx, 0, table, stream));
  SEGGER_HIP(hipMemsetAsync(t.maxy, 0, table, stream));
  SEGGER_HIP(hipMemsetAsync(t.count, 0, table, stream));
  hipLaunchKernelGGL(ct_scan_kernel, dim3(grid_stride_blocks(n_pix, kCtThreads, (int64_t)cus * 32)), dim3(kCtThreads), 0, stream, im,
                     n_pix, (int32_t)max_label, t, cnt);
  SEGGER_LAUNCH_CHECK("ct_scan_kernel");
  size_t temp_bytes = l.temp_bytes;
  SEGGER_HIP(rocprim::select(at<char>(workspace, l.temp), temp_bytes, rocprim::counting_iterator<int32_t>(0), w.present,
                             reinterpret_cast<size_t*>(cnt + kCtPresent), (size_t)(max_label + 1), CtIsPresent{t.count}, stream));
  hipLaunchKernelGGL(ct_trace_kernel, dim3(grid_stride_blocks(l.labels_cap, 1, (int64_t)cus * 32)), dim3(kWave), 0, stream, im, t, w,
                     (int)(lds_max_bits / 32), cnt);
  SEGGER_LAUNCH_CHECK("ct_trace_kernel");
  hipLaunchKernelGGL(ct_offsets_kernel, dim3(1), dim3(kCtOffThreads), 0, stream, t, w, kept, ring_offsets, label_ids, n_pixels,
                     xy_capacity, cnt);
  SEGGER_LAUNCH_CHECK("ct_offsets_kernel");
  hipLaunchKernelGGL(ct_emit_kernel, dim3(grid_stride_blocks(l.labels_cap, kCtThreads, (int64_t)cus * 8)), dim3(kCtThreads), 0, stream,
                     im, w, kept, ring_offsets, CtAffine{scale_x, scale_y, trans_x, trans_y}, reinterpret_cast<double2*>(xy_out),
                     xy_capacity, cnt);
  SEGGER_LAUNCH_CHECK("ct_emit_kernel");
  return SEGGER_OK;
}
