// One wave sorts an array in LDS: the bitonic compare-exchange network of repair.hip (the angular re-sort of a ring) and
// buffered_counts.hip (the genes a polygon touched), once.  A compare-exchange network only ever swaps two entries, so
// whatever `before` answers the result is a permutation of the input and every write stays inside v[0 .. padded).
#pragma once
#include "common.h"

namespace segger {

// What separates two stages of the network: every lane's LDS writes of the stage are visible to every lane of the wave.
// BlockSync: the wave is the whole workgroup.  WaveSync: the wave is one of several and the array is private to it -- one
// wave's LDS operations stay in order, so the compiler is all that has to be told.
struct BlockSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };
struct WaveSync {
  __device__ __forceinline__ void operator()() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

// Sorts v[0 .. padded) ascending by before(a, b) ("a comes before b", a strict total order), padded a power of two >= 2;
// every lane of the wave calls it, the entries are visible on entry and on return.
template <class T, class Before, class Sync>
__device__ __forceinline__ void wave_bitonic_sort(T* v, int padded, Before&& before, Sync&& sync) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int k = 2; k <= padded; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (padded >> 1); t += kWave) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;            // every pair of the stage once
        const T x = v[i], y = v[l];
        const bool swap = (i & k) == 0 ? before(y, x) : before(x, y);
        if (swap) { v[i] = y; v[l] = x; }
      }
      sync();
    }
  }
}

}  // namespace segger
