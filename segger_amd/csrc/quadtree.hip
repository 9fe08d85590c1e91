// segger_quadtree_build / segger_quadtree_label: the adaptive tiling of a slide (include/segger_amd.h has the contract).
// Per point: one Morton key (float2 load, exact float64 arithmetic) and one label; in between a radix sort of the keys.
// The tree itself is tiny: a node's population is the difference of two binary searches on the sorted keys, so the leaves
// come from one small work-list kernel per depth over the nodes that were split one depth up.
#include "common.h"
#include "post_common.h"
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>

namespace segger {
namespace {

constexpr int kQtMaxDepth = 15;                 // 2 bits per level: keys stay below 2^30
constexpr uint32_t kQtNoLeaf = 0xffffffffu;     // Morton-table padding: sorts behind every real range start

struct QtFrame {                                // root frame of the tree, all exact in float64
  double x0, y0, x1, y1;                        // label: points outside [x0, x1] x [y0, y1] get -1 (build: x1 = y1 = +inf)
  double inv_cell;                              // 1 / cell, a power of two: the product below is the exact quotient
  int depth;
};

__device__ __forceinline__ uint32_t qt_spread(uint32_t v) {      // bit i of a 15-bit value -> bit 2 i
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// Morton key at depth f.depth (x in the even bits, y in the odd bits); false for a point outside the frame (or NaN)
__device__ __forceinline__ bool qt_key(float2 p, const QtFrame& f, uint32_t& key) {
  const double x = (double)p.x, y = (double)p.y;
  const double top = (double)((1 << f.depth) - 1);
  // clamped in float64 before the conversion (fmax(NaN, 0) = 0): any input gives a cell inside the grid
  const double fx = fmin(fmax(floor((x - f.x0) * f.inv_cell), 0.0), top);
  const double fy = fmin(fmax(floor((y - f.y0) * f.inv_cell), 0.0), top);
  key = qt_spread((uint32_t)(int)fx) | (qt_spread((uint32_t)(int)fy) << 1);
  return x >= f.x0 && x <= f.x1 && y >= f.y0 && y <= f.y1;
}

__global__ __launch_bounds__(256) void quadtree_keys_kernel(const float2* __restrict__ points, int64_t n, QtFrame f,
                                                           uint32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t k;
  (void)qt_key(points[i], f, k);
  keys[i] = k;
}

// first position whose key is >= v (v may be 2^30, one past the largest key)
__device__ __forceinline__ int64_t qt_lower_bound(const uint32_t* __restrict__ keys, int64_t n, uint32_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One thread per child of a node that was split at depth d - 1 (split_in == NULL: the root, which is always split).
// A non-empty child becomes a leaf (count <= max_size, or the depth cap) or joins the work list of depth d.  Both lists
// are filled through a counter and refuse to write past their capacity; the counters keep counting, so an overflow shows.
__global__ __launch_bounds__(256) void quadtree_nodes_kernel(const uint32_t* __restrict__ keys, int64_t n, int d, int depth,
                                                            int64_t max_size, const uint32_t* __restrict__ split_in,
                                                            const int32_t* __restrict__ n_split_in, int64_t split_cap,
                                                            uint32_t* __restrict__ split_out, int32_t* __restrict__ n_split_out,
                                                            uint64_t* __restrict__ leaf_code, int32_t* __restrict__ leaf_cnt,
                                                            int32_t* __restrict__ n_leaf, int64_t leaf_cap) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t node = t >> 2;
  int64_t n_nodes = 1;
  if (split_in) {
    n_nodes = *n_split_in;
    if (n_nodes > split_cap) n_nodes = split_cap;
  }
  if (node >= n_nodes) return;
  const uint32_t parent = split_in ? split_in[node] : 0u;
  const uint32_t child = parent * 4u + (uint32_t)(t & 3);
  const int shift = 2 * (depth - d);
  const int64_t b = qt_lower_bound(keys, n, child << shift);
  const int64_t e = qt_lower_bound(keys, n, (child + 1u) << shift);
  const int64_t cnt = e - b;
  if (cnt == 0) return;                                      // empty quadrants are not tiles
  if (cnt <= max_size || d == depth) {
    const int64_t slot = atomicAdd(n_leaf, 1);
    if (slot < leaf_cap) {
      leaf_code[slot] = ((uint64_t)d << 32) | child;         // sorts by (depth, prefix)
      leaf_cnt[slot] = (int32_t)cnt;
    }
  } else {
    const int64_t slot = atomicAdd(n_split_out, 1);
    if (slot < split_cap) split_out[slot] = child;
  }
}

// the leaf table in (depth, prefix) order -> the caller's three columns and the unsorted Morton table (range start, id)
__global__ __launch_bounds__(256) void quadtree_unpack_kernel(const uint64_t* __restrict__ leaf_code, const int32_t* __restrict__ n_leaf,
                                                             int64_t leaf_cap, int depth, int32_t* __restrict__ leaf_key,
                                                             int32_t* __restrict__ leaf_depth, int32_t* __restrict__ leaf_count,
                                                             uint32_t* __restrict__ morton_lo, int32_t* __restrict__ morton_id) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= leaf_cap) return;
  int64_t T = *n_leaf;
  if (T > leaf_cap) T = leaf_cap;
  if (i < T) {
    const uint64_t c = leaf_code[i];
    const int d = (int)(c >> 32);
    const uint32_t prefix = (uint32_t)c;
    leaf_key[i] = (int32_t)prefix;
    leaf_depth[i] = d;
    morton_lo[i] = prefix << (2 * (depth - d));
    morton_id[i] = (int32_t)i;
  } else {
    leaf_key[i] = -1;
    leaf_depth[i] = 0;
    leaf_count[i] = 0;
    morton_lo[i] = kQtNoLeaf;
    morton_id[i] = -1;
  }
}

// label = the leaf whose key range holds the point's key: the leaves' ranges are disjoint, so the candidate is the last
// range start <= key, and it matches if its prefix is the key's prefix at its depth
__global__ __launch_bounds__(256) void quadtree_label_kernel(const float2* __restrict__ points, int64_t n, QtFrame f,
                                                            const int32_t* __restrict__ leaf_key, const int32_t* __restrict__ leaf_depth,
                                                            const uint32_t* __restrict__ morton_lo, const int32_t* __restrict__ morton_id,
                                                            const int32_t* __restrict__ n_leaf_dev, int64_t n_leaf,
                                                            int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t T = n_leaf;                                        // a build passes the capacity here and the count on the device
  if (n_leaf_dev) {
    const int64_t t_dev = *n_leaf_dev;
    if (t_dev < T) T = t_dev;
  }
  uint32_t key;
  const bool inside = qt_key(points[i], f, key);
  int32_t lab = -1;
  if (inside && T > 0) {
    int64_t lo = 0, hi = T;                                  // number of range starts <= key
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (morton_lo[mid] <= key) lo = mid + 1; else hi = mid;
    }
    if (lo > 0) {
      const int32_t id = morton_id[lo - 1];
      const int d = leaf_depth[id];
      if ((key >> (2 * (f.depth - d))) == (uint32_t)leaf_key[id]) lab = id;
    }
  }
  labels[i] = lab;
}

int qt_key_bits(int depth) { return 2 * depth; }

size_t qt_sort_temp_bytes(int64_t n, int depth, int64_t leaf_cap) {
  size_t a = 0, b = 0, c = 0;
  uint32_t* k32 = nullptr;
  uint64_t* k64 = nullptr;
  int32_t* v = nullptr;
  (void)rocprim::radix_sort_keys(nullptr, a, k32, k32, (size_t)n, 0, qt_key_bits(depth), (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, b, k64, k64, v, v, (size_t)leaf_cap, 0, 36, (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, c, k32, k32, v, v, (size_t)leaf_cap, 0, 32, (hipStream_t)0);
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

int64_t qt_split_cap(int64_t n, int64_t max_size) {         // split nodes of one depth: disjoint, > max_size points each
  return max_size >= n ? 0 : n / (max_size + 1);
}

bool qt_power_of_two(double v) {
  int e = 0;
  return std::isfinite(v) && v > 0.0 && std::frexp(v, &e) == 0.5;
}

int qt_check_sizes(const char* who, int64_t n, int32_t depth, int64_t max_size, int64_t leaf_cap) {
  SEGGER_REQUIRE(n >= 1, "%s: needs at least one point", who);
  SEGGER_REQUIRE(n <= 0x7fffffffLL, "%s: 2^31 points or more in one tree", who);
  SEGGER_REQUIRE(depth >= 1 && depth <= kQtMaxDepth, "%s: depth must be in [1, 15]", who);
  SEGGER_REQUIRE(max_size >= 1, "%s: max_size must be at least 1", who);
  SEGGER_REQUIRE(leaf_cap >= 1 && leaf_cap <= 0x7fffffffLL, "%s: leaf capacity must be in [1, 2^31)", who);
  return SEGGER_OK;
}

struct QtLayout {
  size_t keys_a, keys_b, split_a, split_b, counters, code_a, code_b, cnt_a, mlo_a, mid_a, temp, total;
  size_t temp_bytes;
  int64_t split_cap;
};

QtLayout qt_layout(int64_t n, int depth, int64_t max_size, int64_t leaf_cap) {
  QtLayout L;
  L.split_cap = qt_split_cap(n, max_size);
  const size_t split_bytes = align256((size_t)(L.split_cap > 0 ? L.split_cap : 1) * 4);
  Carver ws;
  L.keys_a = ws.take((size_t)n * 4);
  L.keys_b = ws.take((size_t)n * 4);
  L.split_a = ws.take(split_bytes);
  L.split_b = ws.take(split_bytes);
  L.counters = ws.take((size_t)(kQtMaxDepth + 1) * 4);
  L.code_a = ws.take((size_t)leaf_cap * 8);
  L.code_b = ws.take((size_t)leaf_cap * 8);
  L.cnt_a = ws.take((size_t)leaf_cap * 4);
  L.mlo_a = ws.take((size_t)leaf_cap * 4);
  L.mid_a = ws.take((size_t)leaf_cap * 4);
  L.temp_bytes = qt_sort_temp_bytes(n, depth, leaf_cap);
  L.temp = ws.take(L.temp_bytes > 0 ? L.temp_bytes : 1);
  L.total = ws.total();
  return L;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int64_t segger_quadtree_workspace_bytes(int64_t n_points, int32_t depth, int64_t max_size, int64_t leaf_cap) {
  const int rc = qt_check_sizes("segger_quadtree_workspace_bytes", n_points, depth, max_size, leaf_cap);
  if (rc != SEGGER_OK) return rc;
  return (int64_t)qt_layout(n_points, depth, max_size, leaf_cap).total;
}

extern "C" int segger_quadtree_build(const float* points, int64_t n_points, double x0, double y0, double cell, int32_t depth,
                                     int64_t max_size, int64_t leaf_cap, int32_t* leaf_key, int32_t* leaf_depth,
                                     int32_t* leaf_count, int32_t* morton_lo, int32_t* morton_id, int32_t* n_leaf,
                                     int32_t* labels, void* workspace, size_t workspace_bytes, segger_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = qt_check_sizes("segger_quadtree_build", n_points, depth, max_size, leaf_cap);
  if (rc != SEGGER_OK) return rc;
  SEGGER_REQUIRE(points && leaf_key && leaf_depth && leaf_count && morton_lo && morton_id && n_leaf && labels,
                 "segger_quadtree_build: NULL pointer");
  SEGGER_REQUIRE(is_aligned(points, 8), "segger_quadtree_build: points must be 8-byte aligned");
  SEGGER_REQUIRE(std::isfinite(x0) && std::isfinite(y0), "segger_quadtree_build: origin is not finite");
  SEGGER_REQUIRE(qt_power_of_two(cell) && cell >= 1.0, "segger_quadtree_build: cell must be a power of two >= 1");
  const QtLayout L = qt_layout(n_points, depth, max_size, leaf_cap);
  if (workspace == nullptr || workspace_bytes < L.total)
    return workspace_too_small("segger_quadtree_build", workspace_bytes, L.total);
  uint32_t* keys_a = at<uint32_t>(workspace, L.keys_a);
  uint32_t* keys_b = at<uint32_t>(workspace, L.keys_b);
  uint32_t* split[2] = {at<uint32_t>(workspace, L.split_a), at<uint32_t>(workspace, L.split_b)};
  int32_t* n_split = at<int32_t>(workspace, L.counters);        // [d]: nodes split at depth d
  uint64_t* code_a = at<uint64_t>(workspace, L.code_a);
  uint64_t* code_b = at<uint64_t>(workspace, L.code_b);
  int32_t* cnt_a = at<int32_t>(workspace, L.cnt_a);
  uint32_t* mlo_a = at<uint32_t>(workspace, L.mlo_a);
  int32_t* mid_a = at<int32_t>(workspace, L.mid_a);
  void* temp = at<char>(workspace, L.temp);
  size_t temp_bytes = L.temp_bytes;

  const QtFrame f{x0, y0, INFINITY, INFINITY, 1.0 / cell, (int)depth};
  const float2* pts = reinterpret_cast<const float2*>(points);
  const unsigned pblk = (unsigned)((n_points + 255) / 256);
  hipLaunchKernelGGL(quadtree_keys_kernel, dim3(pblk), dim3(256), 0, stream, pts, n_points, f, keys_a);
  SEGGER_LAUNCH_CHECK("quadtree_keys_kernel");
  SEGGER_HIP(rocprim::radix_sort_keys(temp, temp_bytes, keys_a, keys_b, (size_t)n_points, 0, qt_key_bits(depth), stream));

  SEGGER_HIP(hipMemsetAsync(n_split, 0, (size_t)(kQtMaxDepth + 1) * 4, stream));
  SEGGER_HIP(hipMemsetAsync(n_leaf, 0, sizeof(int32_t), stream));
  SEGGER_HIP(hipMemsetAsync(code_a, 0xff, (size_t)leaf_cap * 8, stream));       // padding sorts behind every leaf
  SEGGER_HIP(hipMemsetAsync(cnt_a, 0, (size_t)leaf_cap * 4, stream));
  for (int d = 1; d <= depth; ++d) {
    // host-side bound of the nodes split at depth d - 1 (the device-side count decides which threads work)
    int64_t parents = 1;
    if (d > 1) {
      parents = L.split_cap;
      if (2 * (d - 1) < 62 && parents > (1LL << (2 * (d - 1)))) parents = 1LL << (2 * (d - 1));
    }
    if (parents == 0) break;
    const int64_t blocks = (parents * 4 + 255) / 256;
    hipLaunchKernelGGL(quadtree_nodes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, keys_b, n_points, d, (int)depth,
                       max_size, d > 1 ? split[(d - 1) & 1] : (const uint32_t*)nullptr, n_split + (d - 1), L.split_cap,
                       split[d & 1], n_split + d, code_a, cnt_a, n_leaf, leaf_cap);
    SEGGER_LAUNCH_CHECK("quadtree_nodes_kernel");
  }
  temp_bytes = L.temp_bytes;
  SEGGER_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, code_a, code_b, cnt_a, leaf_count, (size_t)leaf_cap, 0, 36, stream));
  const unsigned lblk = (unsigned)((leaf_cap + 255) / 256);
  hipLaunchKernelGGL(quadtree_unpack_kernel, dim3(lblk), dim3(256), 0, stream, code_b, n_leaf, leaf_cap, (int)depth, leaf_key,
                     leaf_depth, leaf_count, mlo_a, mid_a);
  SEGGER_LAUNCH_CHECK("quadtree_unpack_kernel");
  temp_bytes = L.temp_bytes;
  SEGGER_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, mlo_a, reinterpret_cast<uint32_t*>(morton_lo), mid_a, morton_id,
                                       (size_t)leaf_cap, 0, 32, stream));
  hipLaunchKernelGGL(quadtree_label_kernel, dim3(pblk), dim3(256), 0, stream, pts, n_points, f, leaf_key, leaf_depth,
                     reinterpret_cast<const uint32_t*>(morton_lo), morton_id, n_leaf, leaf_cap, labels);
  SEGGER_LAUNCH_CHECK("quadtree_label_kernel");
  return SEGGER_OK;
}

extern "C" int segger_quadtree_label(const float* points, int64_t n_points, double x0, double y0, double x1, double y1,
                                     double cell, int32_t depth, const int32_t* leaf_key, const int32_t* leaf_depth,
                                     const int32_t* morton_lo, const int32_t* morton_id, int64_t n_leaf, int32_t* labels,
                                     segger_stream_t stream) {
  SEGGER_REQUIRE(n_points >= 0, "segger_quadtree_label: negative size");
  SEGGER_REQUIRE(n_points <= 0x7fffffffLL, "segger_quadtree_label: 2^31 points or more in one call");
  SEGGER_REQUIRE(depth >= 1 && depth <= kQtMaxDepth, "segger_quadtree_label: depth must be in [1, 15]");
  SEGGER_REQUIRE(n_leaf >= 1 && n_leaf <= 0x7fffffffLL, "segger_quadtree_label: leaf count must be in [1, 2^31)");
  SEGGER_REQUIRE(std::isfinite(x0) && std::isfinite(y0) && x1 >= x0 && y1 >= y0, "segger_quadtree_label: bad root box");
  SEGGER_REQUIRE(qt_power_of_two(cell) && cell >= 1.0, "segger_quadtree_label: cell must be a power of two >= 1");
  if (n_points == 0) return SEGGER_OK;
  SEGGER_REQUIRE(points && leaf_key && leaf_depth && morton_lo && morton_id && labels, "segger_quadtree_label: NULL pointer");
  SEGGER_REQUIRE(is_aligned(points, 8), "segger_quadtree_label: points must be 8-byte aligned");
  const QtFrame f{x0, y0, x1, y1, 1.0 / cell, (int)depth};
  hipLaunchKernelGGL(quadtree_label_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2*>(points), n_points, f, leaf_key, leaf_depth,
                     reinterpret_cast<const uint32_t*>(morton_lo), morton_id, (const int32_t*)nullptr, n_leaf, labels);
  SEGGER_LAUNCH_CHECK("quadtree_label_kernel");
  return SEGGER_OK;
}
