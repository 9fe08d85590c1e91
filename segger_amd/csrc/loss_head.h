// What the two loss-head translation units share (loss_head.hip: the chained route with its hot rows; loss_head_ordered.hip:
// the ordered, atomic-free backward): the row layout, the launch parameters, the backward scale factors and the one-
// workgroup finish of the forward.  Included after common.h and post_common.h.
#pragma once
#include "common.h"
#include "post_common.h"

namespace segger {
namespace {

constexpr int kItemsPerBlock = 64;                 // rows / triplets per 256-thread block: 4 waves x 4 groups x 4 rounds

// ---- CPL consecutive channels as fp32 ---------------------------------------------------------------------------
// (CPL in {2, 4, 8}: common.h's load2, load4 and Vec8<T>::load; the stores have this one user)
template <typename T, int CPL> struct Row {
  static_assert(CPL == 2 || CPL == 4 || CPL == 8, "a lane owns 2, 4 or 8 channels");
  static __device__ __forceinline__ void load(const T* p, float (&f)[CPL]) {
    if constexpr (CPL == 2) load2(p, f[0], f[1]);
    else if constexpr (CPL == 4) load4(p, f);
    else Vec8<T>::load(p, f);
  }
  static __device__ __forceinline__ void store(T* p, const float (&f)[CPL]) {
    if constexpr (CPL == 8) Vec8<T>::store(p, f);
    else if constexpr (sizeof(T) == 4) {
      if constexpr (CPL == 2) *reinterpret_cast<float2*>(p) = float2{f[0], f[1]};
      else *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
    } else {
      if constexpr (CPL == 2) *reinterpret_cast<uint32_t*>(p) = Vec8<T>::pack(f[0], f[1]);
      else *reinterpret_cast<uint2*>(p) = uint2{Vec8<T>::pack(f[0], f[1]), Vec8<T>::pack(f[2], f[3])};
    }
  }
};

struct LossHeadParams {
  const void* ztx; int64_t ld_ztx; int64_t n_tx;
  const void* zbd; int64_t ld_zbd; int64_t n_bd;
  const int64_t* tx_pos; const int64_t* tx_neg; float tx_margin, tx_eps;
  const int64_t* bd_pos; const int64_t* bd_neg; const float* bd_dpos; const float* bd_dneg; const float* bd_w; float bd_eps;
  const int64_t* sg_src; const int64_t* sg_pos; const int64_t* sg_neg; int64_t n_sg; float sg_margin, sg_eps; int sg_kind;
  const int64_t* sg_indptr; const int32_t* sg_eid; const int32_t* sg_of_tx;
  const float* a; const float* b; const float* gout; float* out; float* graw;
  float* tx_w; int32_t* state; int32_t* next;     // state: [n_tx][2] = (chain head code + 1, contributions), then the hot-row counter
  int32_t* hot_id; float* hot_acc; int64_t max_hot;
  const void* ytx; int64_t ld_ytx; float norm_eps;
  void* gtx; int64_t ld_gtx; float* gbd;
  float* partial; int32_t* ticket;
  int nb_tx, nb_bd, nb_sg;
  int nb_sg_fin;             // loss_sg blocks of the FORWARD launch (the backward's nb_sg is one block per boundary)
  int defer;                 // the forward left the finishing to the backward launch (segger_loss_head_args.reserved_ & 1)
};

// d loss / d (raw mean i): what segger_loss_combine_bwd computes; with `defer` from the hinted gradient directly (the
// finishing launch that would have written graw did not run)
__device__ __forceinline__ float graw_of(const LossHeadParams& p, int i) {
  return p.defer ? (p.gout[3] * p.b[i] + p.gout[i]) * p.a[i] : p.graw[i];
}

// The three means in a fixed order, the weighted total and -- the incoming gradient of a training step being known -- the
// three backward scale factors: one workgroup, launched right behind the forward kernel.  (Round 4 first let the LAST block
// of the forward do this, found by a ticket counter behind a __threadfence(): on this part a device-scope release writes
// back the whole L2 of the XCD, once per block -- 0.76 of the forward's 0.90 ms at C2 (22k blocks), 30 of 44 us at 44k rows;
// tools/bench_loss_head.py, profiles/r04_loss_head_modes_c2.txt.)
__device__ __forceinline__ void loss_head_finish_body(const LossHeadParams& p) {
  __shared__ float wsum[4];
  __shared__ float raw[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 3; ++r) {      // (no arrays indexed by r: they would live in scratch memory)
    const int lo = r == 0 ? 0 : (r == 1 ? p.nb_tx : p.nb_tx + p.nb_bd);
    const int hi = r == 0 ? p.nb_tx : (r == 1 ? p.nb_tx + p.nb_bd : p.nb_tx + p.nb_bd + p.nb_sg_fin);
    const float scale = r == 0 ? (p.n_tx > 0 ? 1.0f / (float)p.n_tx : 0.f)
                      : r == 1 ? 1.0f
                               : (p.n_sg > 0 ? (p.sg_kind == SEGGER_LOSS_BCE ? 0.5f : 1.0f) / (float)p.n_sg : 0.f);
    float s = 0.f;
    for (int k = lo + (int)threadIdx.x; k < hi; k += 256) s += p.partial[k];
    s = wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) raw[r] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * scale;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float t = raw[i] * p.a[i];
      p.out[i] = t;
      total = fmaf(t, p.b[i], total);
    }
    p.out[3] = total;
    if (p.gout != nullptr && p.graw != nullptr) {
#pragma unroll
      for (int i = 0; i < 3; ++i) p.graw[i] = (p.gout[3] * p.b[i] + p.gout[i]) * p.a[i];
    }
  }
}

inline int64_t blocks_of(int64_t n) { return (n + kItemsPerBlock - 1) / kItemsPerBlock; }

}  // namespace
}  // namespace segger
