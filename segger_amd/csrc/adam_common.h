// What the optimizer translation units share (adam.hip: the plain and the guarded update, the gradient guard;
// grad_accum.hip: gradient accumulation over a window and the windowed guard / update): the (tensor, offset) launch table,
// the update and the guard's second pass as templates whose extra arguments select the variant, the guard's first pass.
// Everything sits in an unnamed namespace: each unit instantiates what it launches.
#pragma once
#include "common.h"
#include "post_common.h"

namespace segger {
namespace {

constexpr int kAdamMaxTensors = 64;
constexpr int kAdamElemsPerBlock = 2048;          // 256 threads x 2 x float4

struct AdamBatch {
  segger_adam_tensor t[kAdamMaxTensors];
  int32_t first_block[kAdamMaxTensors + 1];       // prefix sums of the tensors' block counts
  int32_t n;
  double lr, beta1, beta2, eps;                   // torch keeps them as Python floats and evaluates 1 - beta, beta^step in double
  int64_t* counter; int64_t counter_inc;          // optional: *counter += counter_inc by the first workgroup (nobody reads it here)
  const double* hyper;                            // optional DEVICE {lr, beta1, beta2, eps}: overrides the four values above
};

// last tensor of the batch with first_block <= blk
__device__ __forceinline__ int adam_tensor_of_block(const AdamBatch& b, int blk) {
  int lo = 0, hi = b.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b.first_block[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// Were all four arrays of a tensor read as float4?  (What the update decides, the guard's sum of squares follows: the
// same loads of the same gradient bytes.)
__device__ __forceinline__ bool adam_vec(const segger_adam_tensor& t) {
  return (t.numel % 4 == 0) &&
         (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15u) == 0;
}

// The guard argument of adam_kernel<G...>: none for the plain update, one `const segger_guard_state*` for the guarded one.
__device__ __forceinline__ const segger_guard_state* guard_of() { return nullptr; }
__device__ __forceinline__ const segger_guard_state* guard_of(const segger_guard_state* g) { return g; }
// ... and a second one, `const segger_accum_window*`, for the update behind an accumulation window (the guard may then be NULL)
__device__ __forceinline__ const segger_guard_state* guard_of(const segger_guard_state* g, const segger_accum_window*) { return g; }
__device__ __forceinline__ const segger_accum_window* window_of(const segger_guard_state*, const segger_accum_window* w) { return w; }

// The update of one block.  adam_kernel<>(b) is the plain update, with the kernel arguments and the code it always had;
// adam_kernel<const segger_guard_state*>(b, guard) multiplies every gradient by guard->coef first (the clip factor over the
// loss scale, written by grad_guard_finish_kernel) and writes no tensor byte on a skipped step (guard->skip); the dropout /
// sampling counter moves on either way, so that the next step draws fresh numbers.
// adam_kernel<const segger_guard_state*, const segger_accum_window*>(b, guard, window) is the update at the end of every
// micro-step of an accumulation window: it writes no tensor byte unless window->close is set (the counter still moves on:
// every micro-batch draws fresh numbers), and applies the guard when there is one.
template <class... G>
__global__ __launch_bounds__(256) void adam_kernel(AdamBatch b, G... guard_) {
  constexpr bool kGuarded = sizeof...(G) != 0;
  constexpr bool kWindowed = sizeof...(G) == 2;
  const int blk = blockIdx.x;
  int lo = 0, hi = b.n;                            // last tensor with first_block <= blk
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b.first_block[mid] <= blk) lo = mid; else hi = mid;
  }
  if (blk == 0 && threadIdx.x == 0 && b.counter != nullptr) *b.counter += b.counter_inc;
  float coef = 1.0f;
  if constexpr (kWindowed) {
    if (window_of(guard_...)->close == 0) return;
  }
  if constexpr (kGuarded) {
    const segger_guard_state* guard = guard_of(guard_...);
    if (!kWindowed || guard != nullptr) {
      if (guard->skip != 0) return;
      coef = guard->coef;
    }
  }
  const segger_adam_tensor& t = b.t[lo];
  const int64_t base = (int64_t)(blk - b.first_block[lo]) * kAdamElemsPerBlock;
  // torch/optim/adam.py (capturable, fused=False formulas; the fused kernel evaluates the same expressions in fp32):
  //   exp_avg = lerp(exp_avg, grad, 1 - beta1);  exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * grad^2
  //   param -= (lr / (1 - beta1^step)) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)
  const double step = (double)*t.step;             // already advanced by adam_advance_kernel
  const double lr = b.hyper ? b.hyper[0] : b.lr, beta1_ = b.hyper ? b.hyper[1] : b.beta1;
  const double beta2_ = b.hyper ? b.hyper[2] : b.beta2, eps_ = b.hyper ? b.hyper[3] : b.eps;
  const float bc1 = (float)(1.0 - pow(beta1_, step));
  const float bc2 = (float)(1.0 - pow(beta2_, step));
  const float step_size = (float)lr / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  const float w1 = (float)(1.0 - beta1_), w2 = (float)(1.0 - beta2_), beta2 = (float)beta2_, eps = (float)eps_;
  auto one = [&](float& p, float g, float& m, float& v) {
    if constexpr (kGuarded) g = g * coef;
    m = m + (g - m) * w1;
    v = beta2 * v + w2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
  };
  const bool vec = (t.numel % 4 == 0) &&
                   (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15u) == 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int64_t i = base + ((int64_t)r * 256 + threadIdx.x) * 4;
    if (i >= t.numel) break;
    if (vec) {
      f32x4 p = *reinterpret_cast<f32x4*>(t.param + i);
      const f32x4 g = *reinterpret_cast<const f32x4*>(t.grad + i);
      f32x4 m = *reinterpret_cast<f32x4*>(t.exp_avg + i);
      f32x4 v = *reinterpret_cast<f32x4*>(t.exp_avg_sq + i);
      float pp[4] = {p.x, p.y, p.z, p.w}, mm[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
      const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) one(pp[k], gg[k], mm[k], vv[k]);
      p = f32x4{pp[0], pp[1], pp[2], pp[3]}; m = f32x4{mm[0], mm[1], mm[2], mm[3]}; v = f32x4{vv[0], vv[1], vv[2], vv[3]};
      *reinterpret_cast<f32x4*>(t.param + i) = p;
      *reinterpret_cast<f32x4*>(t.exp_avg + i) = m;
      *reinterpret_cast<f32x4*>(t.exp_avg_sq + i) = v;
    } else {
      for (int k = 0; k < 4 && i + k < t.numel; ++k) one(t.param[i + k], t.grad[i + k], t.exp_avg[i + k], t.exp_avg_sq[i + k]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ the gradient guard
// Between the backward and the update, on the device: the global L2 norm of ALL gradients and whether any of them is not
// finite, from which one workgroup derives what the update multiplies every gradient by, whether the step is skipped, and
// the next loss scale (include/segger_amd.h: segger_guard_state).  Two passes, no float atomics: every sum is taken in one
// fixed order, so the same gradients give the same bytes whatever the scheduling.
struct GuardSlot { double sum; int64_t nonfinite; };        // what pass 1 leaves per block

__device__ __forceinline__ bool guard_nonfinite(float g) { return (__float_as_uint(g) & 0x7f800000u) == 0x7f800000u; }

// Sum and OR over the workgroup's 256 threads in one fixed order: butterfly inside each wave (every lane ends with the same
// bits: a + b == b + a), then the four wave totals first to last.  Valid in thread 0.
__device__ __forceinline__ void guard_group_reduce(double& sum, int& bad, double* lds_sum, int* lds_bad) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    sum += __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(sum), m));
    bad |= __shfl_xor(bad, m, kWave);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) { lds_sum[wave] = sum; lds_bad[wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = lds_sum[0]; bad = lds_bad[0];
    for (int w = 1; w < 256 / kWave; ++w) { sum += lds_sum[w]; bad |= lds_bad[w]; }
  }
}

// Pass 1: one workgroup per block of adam_kernel's (tensor, offset) layout; slots[blockIdx.x] = {sum of grad^2 in float64,
// any non-finite}.  The first workgroup also files the batch's step-counter addresses for pass 2's rollback.  A batch
// without elements is launched with one workgroup, which writes no slot.
__global__ __launch_bounds__(256) void grad_guard_partial_kernel(AdamBatch b, GuardSlot* __restrict__ slots,
                                                                 float** __restrict__ steps) {
  __shared__ double lds_sum[256 / kWave];
  __shared__ int lds_bad[256 / kWave];
  const int blk = blockIdx.x;
  if (blk == 0) for (int i = threadIdx.x; i < b.n; i += 256) steps[i] = b.t[i].step;
  if (blk >= b.first_block[b.n]) return;
  const int lo = adam_tensor_of_block(b, blk);
  const segger_adam_tensor& t = b.t[lo];
  const int64_t base = (int64_t)(blk - b.first_block[lo]) * kAdamElemsPerBlock;
  const bool vec = adam_vec(t);
  double sum = 0.;
  int bad = 0;
  auto one = [&](float g) {
    sum += (double)g * (double)g;
    bad |= guard_nonfinite(g) ? 1 : 0;
  };
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int64_t i = base + ((int64_t)r * 256 + threadIdx.x) * 4;
    if (i >= t.numel) break;
    if (vec) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(t.grad + i);
      one(g.x); one(g.y); one(g.z); one(g.w);
    } else {
      for (int k = 0; k < 4 && i + k < t.numel; ++k) one(t.grad[i + k]);
    }
  }
  guard_group_reduce(sum, bad, lds_sum, lds_bad);
  if (threadIdx.x == 0) slots[blk] = GuardSlot{sum, (int64_t)bad};
}

struct GuardFinish {
  double max_norm, growth, backoff;
  int32_t growth_interval, flags;
  const GuardSlot* slots; int64_t n_slots;
  float* const* steps; int32_t n_steps;
  segger_guard_state* state;
};

// Pass 2: ONE workgroup.  Thread t adds slots t, t + 256, ... in that order, the workgroup's sums are added as in pass 1;
// thread 0 writes the state.  A skipped step whose counters were advanced at its head gets them back here, before the
// update launch exists: no update workgroup can read a counter while it is rewritten.
// grad_guard_finish_kernel<const segger_accum_window*>(a, window): the decision over an accumulated gradient -- taken, and
// the state touched, only by the micro-step that closes the window.
template <class... W>
__global__ __launch_bounds__(256) void grad_guard_finish_kernel(GuardFinish a, W... window_) {
  __shared__ double lds_sum[256 / kWave];
  __shared__ int lds_bad[256 / kWave];
  __shared__ int lds_skip;
  if constexpr (sizeof...(W) != 0) {
    if (window_of(nullptr, window_...)->close == 0) return;   // (the whole workgroup: nobody waits at a barrier below)
  }
  double sum = 0.;
  int bad = 0;
  for (int64_t i = threadIdx.x; i < a.n_slots; i += 256) {
    const GuardSlot s = a.slots[i];
    sum += s.sum;
    bad |= s.nonfinite != 0 ? 1 : 0;
  }
  guard_group_reduce(sum, bad, lds_sum, lds_bad);
  if (threadIdx.x == 0) {
    segger_guard_state st = *a.state;
    // torch.nn.utils.clip_grad_norm_ on the UNSCALED gradients (GradScaler.unscale_ first), then GradScaler.update
    const double scale = (double)st.scale;
    const double true_norm = sqrt(sum) / scale;
    const double clip = a.max_norm > 0. ? fmin(1., a.max_norm / (true_norm + 1e-6)) : 1.;
    st.skip = bad;
    st.coef = bad ? 0.f : (float)(clip / scale);
    st.norm = bad ? __longlong_as_double(0x7ff8000000000000LL) : true_norm;
    st.n_skipped += bad;
    st.n_clipped += (!bad && clip < 1.) ? 1 : 0;
    if (a.growth_interval > 0) {
      if (bad) {
        st.scale = (float)(scale * a.backoff);
        st.growth_tracker = 0;
      } else if (++st.growth_tracker == a.growth_interval) {
        st.scale = (float)(scale * a.growth);
        st.growth_tracker = 0;
      }
    }
    *a.state = st;
    lds_skip = bad;
  }
  __syncthreads();
  if (lds_skip != 0 && (a.flags & SEGGER_ADAM_STEPS_ADVANCED) != 0)
    for (int i = threadIdx.x; i < a.n_steps; i += 256) *a.steps[i] -= 1.0f;
}

// ------------------------------------------------------------------------------------------------ host side
// tensors[at ...] (at most kAdamMaxTensors of them) as one batch: the table, the prefix sums of the block counts
inline int adam_batch(const segger_adam_tensor* tensors, int32_t n_tensors, int32_t at, bool need_state, AdamBatch& b, int64_t& blocks) {
  b.n = n_tensors - at < kAdamMaxTensors ? n_tensors - at : kAdamMaxTensors;
  blocks = 0;
  for (int i = 0; i < b.n; ++i) {
    const segger_adam_tensor& t = tensors[at + i];
    SEGGER_REQUIRE(t.numel >= 0 && t.step, "segger_adam_step: tensor %d: bad size or NULL step", at + i);
    SEGGER_REQUIRE(t.numel == 0 || (t.grad && (!need_state || (t.param && t.exp_avg && t.exp_avg_sq))),
                   "segger_adam_step: tensor %d: NULL pointer", at + i);
    b.t[i] = t;
    b.first_block[i] = (int32_t)blocks;
    blocks += (t.numel + kAdamElemsPerBlock - 1) / kAdamElemsPerBlock;
    SEGGER_REQUIRE(blocks < 0x7fffffffLL, "segger_adam_step: too many elements");
  }
  b.first_block[b.n] = (int32_t)blocks;
  return SEGGER_OK;
}

inline size_t guard_workspace(int64_t n_tensors, int64_t total_blocks, size_t* steps_off) {
  Carver c;
  c.take((size_t)total_blocks * sizeof(GuardSlot));
  const size_t off = c.take((size_t)n_tensors * sizeof(float*));
  if (steps_off) *steps_off = off;
  return c.total();
}

// segger_grad_guard's checks and launches; W = one `const segger_accum_window*` for the guard over an accumulated gradient
template <class... W>
inline int grad_guard_launch(const segger_adam_tensor* tensors, int32_t n_tensors, const segger_guard_cfg* cfg,
                             segger_guard_state* state, void* workspace, int64_t workspace_bytes, segger_stream_t stream_,
                             W... window) {
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || tensors), "segger_grad_guard: NULL tensor table");
  SEGGER_REQUIRE(cfg != nullptr && is_aligned(cfg, 8), "segger_grad_guard: cfg is NULL or misaligned");
  SEGGER_REQUIRE(cfg->max_norm >= 0., "segger_grad_guard: max_norm %g is negative or NaN (0 = no clipping)", cfg->max_norm);
  SEGGER_REQUIRE(cfg->backoff > 0. && cfg->backoff < 1., "segger_grad_guard: backoff %g outside (0, 1)", cfg->backoff);
  SEGGER_REQUIRE(cfg->growth >= 1. && cfg->growth < HUGE_VAL, "segger_grad_guard: growth %g below 1 or not finite", cfg->growth);
  SEGGER_REQUIRE(cfg->growth_interval >= 0, "segger_grad_guard: negative growth_interval (0 = a static scale)");
  SEGGER_REQUIRE((cfg->flags & ~SEGGER_ADAM_STEPS_ADVANCED) == 0, "segger_grad_guard: unknown flags %d", cfg->flags);
  if (n_tensors == 0) return SEGGER_OK;                       // no gradient, no decision: the state stays as it is
  SEGGER_REQUIRE(state != nullptr && is_aligned(state, 8), "segger_grad_guard: state is NULL or misaligned");
  SEGGER_REQUIRE(workspace != nullptr && is_aligned(workspace, 256), "segger_grad_guard: workspace is NULL or not 256-byte aligned");
  SEGGER_REQUIRE(workspace_bytes >= 0, "segger_grad_guard: negative workspace_bytes");
  int64_t total = 0;
  for (int32_t i = 0; i < n_tensors; ++i) {
    SEGGER_REQUIRE(tensors[i].numel >= 0 && tensors[i].step, "segger_grad_guard: tensor %d: bad size or NULL step", i);
    SEGGER_REQUIRE(tensors[i].numel == 0 || tensors[i].grad, "segger_grad_guard: tensor %d: NULL pointer", i);
    total += (tensors[i].numel + kAdamElemsPerBlock - 1) / kAdamElemsPerBlock;
    SEGGER_REQUIRE(total < 0x7fffffffLL, "segger_grad_guard: too many elements");
  }
  size_t steps_off = 0;
  const size_t need = guard_workspace(n_tensors, total, &steps_off);
  if ((size_t)workspace_bytes < need) {
    set_error("segger_grad_guard: workspace %lld < %zu bytes", (long long)workspace_bytes, need);
    return SEGGER_EINVAL;
  }
  GuardSlot* slots = at<GuardSlot>(workspace, 0);
  float** steps = at<float*>(workspace, steps_off);
  int64_t slot0 = 0;
  for (int32_t at_ = 0; at_ < n_tensors; at_ += kAdamMaxTensors) {
    AdamBatch b{};
    int64_t blocks = 0;
    if (const int rc = adam_batch(tensors, n_tensors, at_, false, b, blocks)) return rc;
    hipLaunchKernelGGL(grad_guard_partial_kernel, dim3((unsigned)(blocks > 0 ? blocks : 1)), dim3(256), 0, stream, b,
                       slots + slot0, steps + at_);
    slot0 += blocks;
  }
  GuardFinish f{cfg->max_norm, cfg->growth, cfg->backoff, cfg->growth_interval, cfg->flags, slots, total, steps, n_tensors, state};
  hipLaunchKernelGGL(grad_guard_finish_kernel<W...>, dim3(1), dim3(256), 0, stream, f, window...);
  SEGGER_LAUNCH_CHECK("grad guard kernels");
  return SEGGER_OK;
}

}  // namespace
}  // namespace segger
