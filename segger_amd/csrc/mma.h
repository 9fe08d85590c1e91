// Device toolkit of the matrix-core kernels (gfx950 only, wave64): the register vectors of the MFMA operands, the MFMA
// wrappers per element type, the transposing LDS read, the counted waits and LDS-only barriers the pipelined kernels
// rest on, and the compile-time loop.  A new kernel takes these from here; nothing in this header launches anything.
#pragma once
#include <type_traits>
#include "common.h"

namespace segger {

// ------------------------------------------------------- register vectors --
typedef __bf16   bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8  __attribute__((ext_vector_type(8)));
typedef __bf16   bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2  __attribute__((ext_vector_type(2)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2  __attribute__((ext_vector_type(2)));
typedef short    s16x4  __attribute__((ext_vector_type(4)));
typedef int32_t  i32x4  __attribute__((ext_vector_type(4)));

// ------------------------------------------------------- matrix cores ------
// run: v_mfma_f32_32x32x16 (lane (r, h) supplies 8 consecutive k of row r per operand), run16: v_mfma_f32_16x16x32,
// sum2: c + lo(a) + hi(a) by v_dot2 against a pair of ones.  Operands travel as u32x4 (8 packed 16-bit elements).
template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
  static __device__ __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 run16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float sum2(uint32_t a, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, 0x3f803f80u), c, false);
  }
};
template <> struct Mfma<f16_t> {
  static __device__ __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 run16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float sum2(uint32_t a, float c) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, 0x3c003c00u), c, false);
  }
};
// exact fp32, v_mfma_f32_32x32x2_f32: lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31], one float each
__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------- LDS ---------------
// 4 rows x 16 columns of 16-bit elements, transposed: lane i of a 16-lane group receives column i of the 4 rows
__device__ __forceinline__ u32x2 lds_read_tr(const unsigned char* p) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(const_cast<unsigned char*>(p)));
  return __builtin_bit_cast(u32x2, v);
}

// ------------------------------------------------------- waits and barriers
// s_waitcnt on gfx9: vmcnt in bits 3:0 and 15:14, expcnt in 6:4, lgkmcnt in 11:8; a field of all ones does not wait.
// The two encodings are spelled here and nowhere else.
constexpr int kWaitVmcnt0 = 0x0F70;       // vmcnt(0); expcnt and lgkmcnt not waited for
constexpr int kWaitLgkmcnt0 = 0xC07F;     // lgkmcnt(0); vmcnt and expcnt not waited for
template <int N> __device__ __forceinline__ void wait_vmcnt() {   // at most N vector-memory operations outstanding
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  __builtin_amdgcn_s_waitcnt(kWaitVmcnt0 | (N & 15) | ((N >> 4) << 14));
}
__device__ __forceinline__ void wait_lgkmcnt0() {                 // this wave's LDS (and scalar-memory) operations are done
  __builtin_amdgcn_s_waitcnt(kWaitLgkmcnt0);
}

// A workgroup barrier that orders LDS traffic only: this wave's LDS operations have completed (lgkmcnt(0)), then s_barrier.
// __syncthreads() is a release fence as well -- s_waitcnt vmcnt(0): every global load in flight (the prefetch these kernels
// live on) and every output store would have to drain at each barrier.
// lds_barrier(): for kernels whose global loads are visible to the compiler (linear_f32_split.hip) -- fenced, so that it
// moves no memory access across.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("" ::: "memory");                         // (compiler: no memory access moves across)
  wait_lgkmcnt0();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// lds_barrier_unfenced(): for linear_wgrad.hip's LDS-DMA rings -- the asm DMA statement behind each barrier is the compiler's
// fence there, and two more reschedule the data-gradient and positional-backward kernels (measured as they are, without).
__device__ __forceinline__ void lds_barrier_unfenced() {
  wait_lgkmcnt0();
  __builtin_amdgcn_s_barrier();
}

// ------------------------------------------------------- compile-time loop -
// f(integral_constant<int, 0>{}) .. f(integral_constant<int, N - 1>{}): a loop whose counter is a constant expression in
// its body
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

}  // namespace segger
