// Host-side scaffolding shared by the translation units (included after common.h): the predicates that decide whether a
// pointer may be dereferenced, the rule that places the scratch arrays inside a caller's workspace, the step from a dtype
// code to an element type, and the integer helpers of the post-processing kernels: the whole-wave sums, the one-workgroup
// scan (GroupScan, and the counts-to-offsets kernel made of it alone) and the slot of a hit in a count / fill traversal.
// One definition each: a fix to the carving rule, to an alignment check or to the scan is made here and nowhere else.
#pragma once
#include <type_traits>
#include "common.h"

namespace segger {

// ---------------------------------------------------------------- host: sizes and pointers ---
// bytes is a power of two.  NULL counts as aligned: optional pointers pass, and are rejected (or not) by the NULL checks.
inline bool is_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int bit_length(unsigned long long v) {
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}

// grid of a grid-stride kernel: one thread per item up to max_blocks blocks, never an empty grid
inline unsigned grid_stride_blocks(int64_t n_items, int threads, int64_t max_blocks) {
  const int64_t blocks = ceil_div(n_items, threads);
  return (unsigned)(blocks < 1 ? 1 : (blocks < max_blocks ? blocks : max_blocks));
}

// the compute units that size a persistent grid; a guess where the device does not say
inline int cu_count_or_default() { return device_cu_count() > 0 ? device_cu_count() : 256; }

// The regions of a workspace, first to last: every region starts on a 256-byte boundary of a 256-byte aligned base.
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t start = off;
    off += align256(bytes);
    return start;
  }
  size_t total() const { return off; }
};

template <typename T>
inline T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

inline int workspace_too_small(const char* who, size_t have, size_t need) {
  set_error("%s: workspace %zu < %zu bytes", who, have, need);
  return SEGGER_EWORKSPACE;
}

// ---------------------------------------------------------------- host: element types ---
inline size_t esize(int dtype) { return dtype == SEGGER_F32 ? sizeof(float) : sizeof(bf16_t); }

// a generic lambda's compile-time arguments: `using T = elem_t<decltype(t)>;`, `constexpr int N = decltype(n)::value;`
template <typename T> struct dtype_tag { using type = T; };
template <typename Tag> using elem_t = typename Tag::type;
template <int N> using int_c = std::integral_constant<int, N>;

// The one place a SEGGER_* dtype code becomes an element type: returns f(dtype_tag<float | bf16_t | f16_t>{}), or refuses
// any other code in `who`'s name.  The translation units that support fewer types on purpose keep their own switch.
template <typename F>
int dispatch_dtype(int dtype, const char* who, F&& f) {
  switch (dtype) {
    case SEGGER_F32:  return f(dtype_tag<float>{});
    case SEGGER_BF16: return f(dtype_tag<bf16_t>{});
    case SEGGER_F16:  return f(dtype_tag<f16_t>{});
    default: set_error("%s: unknown dtype %d", who, dtype); return SEGGER_EINVAL;
  }
}

// ---------------------------------------------------------------- device: whole-wave integer sums ---
// every lane returns the total
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, kWave);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, kWave);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, kWave);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, kWave);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += (int64_t)shfl_xor64((uint64_t)v, m);
  return v;
}

// ---------------------------------------------------------------- device: the one-workgroup scan ---
// What a scan adds up: an int64, or an int64 and an int scanned together in one pass (vertices and kept rings).
struct ScanPair { int64_t v; int k; };
__device__ __forceinline__ ScanPair operator+(ScanPair a, ScanPair b) { return ScanPair{a.v + b.v, a.k + b.k}; }
__device__ __forceinline__ ScanPair operator-(ScanPair a, ScanPair b) { return ScanPair{a.v - b.v, a.k - b.k}; }
__device__ __forceinline__ int64_t scan_shfl(int64_t a, int src) { return (int64_t)shfl64((uint64_t)a, src); }
__device__ __forceinline__ ScanPair scan_shfl(ScanPair a, int src) { return ScanPair{scan_shfl(a.v, src), __shfl(a.k, src, kWave)}; }

constexpr int kScanThreads = 1024;                                   // the workgroup of the scan kernels

// A scan over more items than the workgroup has threads, kThreads items a chunk: an inclusive shuffle scan per wave, the
// waves' totals in LDS (`totals`, kThreads / kWave entries), a linear sum over the waves, and the carry of the chunks
// before.  step(mine), called by every thread of the workgroup with its item's value (zero past the end), returns the
// carry plus the values of the chunk's earlier threads -- the exclusive sum at the item -- and moves the carry on.  Two
// barriers a step, whatever T; after the last step `carry` is the total, in every thread.  Integer sums: no order shows.
template <int kThreads, class T>
struct GroupScan {
  T* totals;
  T carry;
  __device__ __forceinline__ T step(T mine) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    T v = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {                            // inclusive scan of the wave
      const T o = scan_shfl(v, lane >= d ? lane - d : lane);
      if (lane >= d) v = v + o;
    }
    if (lane == kWave - 1) totals[wave] = v;
    __syncthreads();
    T before = carry, all = carry;
    for (int w = 0; w < kThreads / kWave; ++w) {
      const T t = totals[w];
      if (w < wave) before = before + t;
      all = all + t;
    }
    carry = all;
    __syncthreads();                                                 // the totals are rewritten by the next step
    return before + v - mine;
  }
};

namespace {
// v[1 .. n] holds counts; afterwards v[i] = the counts before i, v[n] the total (v[0] = 0 is written); *total, if given, too.
// One workgroup.  Every including unit that launches it gets its own copy, as with cell_rings.h's kernels.
template <class T>
__global__ __launch_bounds__(kScanThreads) void counts_to_offsets_kernel(T* __restrict__ v, int64_t n, int64_t* __restrict__ total) {
  __shared__ int64_t totals[kScanThreads / kWave];
  GroupScan<kScanThreads, int64_t> scan{totals, 0};
  for (int64_t base = 0; base < n; base += kScanThreads) {
    const int64_t i = base + threadIdx.x;
    const int64_t mine = i < n ? (int64_t)v[i + 1] : 0;
    const int64_t before = scan.step(mine);
    if (i < n) v[i + 1] = (T)(before + mine);
  }
  if (threadIdx.x == 0) {
    v[0] = 0;
    if (total) *total = scan.carry;
  }
}
}  // namespace

// ---------------------------------------------------------------- device: the slot of a hit, count / fill ---
// A traversal that a count pass and a fill pass walk alike, one wave, 64 candidates a step.  Every lane calls this once a
// step: `found` is the hits of the steps before and moves on by this step's; the slot of a lane with a hit is begin + found
// + the hit lanes below it, and write(slot) runs if that is in [0, end) (kWrite = false: the count pass, never).  No atomic
// decides a slot, so the order of a list is the traversal's whatever the scheduling, and the same call gives the same bytes.
template <bool kWrite = true, class F>
__device__ __forceinline__ void hit_slot(bool hit, int64_t begin, int64_t end, int64_t& found, F&& write) {
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long m = __ballot(hit);
  if (kWrite && hit) {
    const int64_t slot = begin + found + (int64_t)__popcll(m & ((1ull << lane) - 1));
    if (slot >= 0 && slot < end) write(slot);
  }
  found += (int64_t)__popcll(m);
}

// float bits whose unsigned order is the float order: -0.0 sorts just below +0.0 as a value of its own and NaNs are the
// caller's business (csrc/assign.hip's mapping canonicalises both and is a different function)
__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace segger
