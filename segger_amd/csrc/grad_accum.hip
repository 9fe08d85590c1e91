// Gradient accumulation over a window of N micro-steps for the captured training step (Lightning's
// accumulate_grad_batches; include/segger_amd.h: segger_accum_window): the accumulate launch, and the guard / update that
// act only when the window closes -- instantiations of adam_common.h's templates with a window argument.
#include "adam_common.h"

namespace segger {
namespace {

// the same inside an accumulation window (segger_grad_accumulate): only the micro-step that closes the window counts as
// an optimizer step; `guard` may be NULL
__global__ __launch_bounds__(64) void adam_advance_windowed_kernel(AdamBatch b, const segger_guard_state* __restrict__ guard,
                                                                   const segger_accum_window* __restrict__ window) {
  if (window->close == 0 || (guard != nullptr && guard->skip != 0)) return;
  for (int i = threadIdx.x; i < b.n; i += 64) *b.t[i].step += 1.0f;
}

// ------------------------------------------------------------------------------------------------ gradient accumulation
// A window of N micro-steps (Lightning's accumulate_grad_batches): acc = first ? g * w : acc + g * w with w = 1 / N, for
// ALL tensors in one launch over the update's own (tensor, offset) blocks -- t.grad is the micro-step's gradient (read),
// t.param the fp32 accumulator (written).  `first` comes from the DEVICE-side window (window->pos == 0), so one captured
// graph serves every position of the window.  Every element is owned by one thread and gets one multiply and one add per
// micro-step, rounded separately (no contraction into an FMA): its sum is formed in micro-step order and nothing is added
// atomically -- the same gradients give the same bytes.  A streaming kernel: 8 (first) or 12 bytes per element, 128-bit
// loads and stores wherever a tensor allows them.
//
// kAdvance (the call's last launch): the window moves on here.  Each workgroup reads window->pos ONCE (thread 0, handed to
// the others through LDS), and takes an integer ticket when it is done; the workgroup that draws the last ticket -- by then
// every workgroup of the launch has read pos -- writes pos / close for the launches behind this one and puts the ticket
// counter back to 0.
template <bool kAdvance>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(AdamBatch b, float w, int32_t n_window,
                                                              segger_accum_window* __restrict__ window) {
  __shared__ int32_t lds_pos;
  if (threadIdx.x == 0) lds_pos = window->pos;
  __syncthreads();
  const int32_t pos = lds_pos;
  const bool first = pos == 0;
  const int blk = blockIdx.x;
  if (blk < b.first_block[b.n]) {
    const int lo = adam_tensor_of_block(b, blk);
    const segger_adam_tensor& t = b.t[lo];
    const int64_t base = (int64_t)(blk - b.first_block[lo]) * kAdamElemsPerBlock;
    const bool vec = (t.numel % 4 == 0) && (((uintptr_t)t.param | (uintptr_t)t.grad) & 15u) == 0;
    auto one = [&](float a, float g) { return first ? __fmul_rn(g, w) : __fadd_rn(a, __fmul_rn(g, w)); };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t i = base + ((int64_t)r * 256 + threadIdx.x) * 4;
      if (i >= t.numel) break;
      if (vec) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(t.grad + i);
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!first) a = *reinterpret_cast<const f32x4*>(t.param + i);
        a = f32x4{one(a.x, g.x), one(a.y, g.y), one(a.z, g.z), one(a.w, g.w)};
        *reinterpret_cast<f32x4*>(t.param + i) = a;
      } else {
        for (int k = 0; k < 4 && i + k < t.numel; ++k) t.param[i + k] = one(first ? 0.f : t.param[i + k], t.grad[i + k]);
      }
    }
  }
  if constexpr (kAdvance) {
    if (threadIdx.x == 0) {                        // (thread 0 has read pos: its own load above has long returned)
      __threadfence();
      const int ticket = atomicAdd(&window->arrived, 1);
      if (ticket == (int)gridDim.x - 1) {
        const int32_t summed = pos + 1;
        const int32_t close = summed >= n_window ? 1 : 0;
        window->arrived = 0;
        window->close = close;
        window->pos = close ? 0 : summed;
      }
    }
  }
}

// flush: phase 0 opens the close-only sequence (close = "something is summed"), phase 1 ends it (an empty window)
__global__ __launch_bounds__(64) void accum_window_flush_kernel(segger_accum_window* __restrict__ window, int32_t phase) {
  if (threadIdx.x != 0) return;
  if (phase == 0) {
    window->close = window->pos > 0 ? 1 : 0;
  } else {
    window->pos = 0;
    window->close = 0;
  }
}

}  // namespace
}  // namespace segger

using namespace segger;

// ------------------------------------------------------------------------------------------------ gradient accumulation
extern "C" int segger_grad_accumulate(const segger_adam_tensor* tensors, int32_t n_tensors, int32_t n_window,
                                      segger_accum_window* window, segger_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || tensors), "segger_grad_accumulate: NULL tensor table");
  SEGGER_REQUIRE(n_window >= 1 && n_window <= (1 << 24), "segger_grad_accumulate: a window of %d micro-steps", n_window);
  SEGGER_REQUIRE(window != nullptr && is_aligned(window, 4), "segger_grad_accumulate: window is NULL or misaligned");
  for (int32_t i = 0; i < n_tensors; ++i) {
    const segger_adam_tensor& t = tensors[i];
    SEGGER_REQUIRE(t.numel >= 0, "segger_grad_accumulate: tensor %d: negative size", i);
    SEGGER_REQUIRE(t.numel == 0 || (t.grad && t.param), "segger_grad_accumulate: tensor %d: NULL gradient or accumulator", i);
    SEGGER_REQUIRE(is_aligned(t.grad, 4) && is_aligned(t.param, 4), "segger_grad_accumulate: tensor %d: misaligned pointer", i);
    SEGGER_REQUIRE(t.numel == 0 || (const float*)t.param != t.grad, "segger_grad_accumulate: tensor %d: the accumulator is the gradient", i);
  }
  const float w = 1.0f / (float)n_window;
  int32_t at = 0;
  do {                                             // (an empty table still moves the window on: one workgroup)
    AdamBatch b{};
    b.n = n_tensors - at < kAdamMaxTensors ? n_tensors - at : kAdamMaxTensors;
    int64_t blocks = 0;
    for (int i = 0; i < b.n; ++i) {
      b.t[i] = tensors[at + i];
      b.first_block[i] = (int32_t)blocks;
      blocks += (b.t[i].numel + kAdamElemsPerBlock - 1) / kAdamElemsPerBlock;
      SEGGER_REQUIRE(blocks < 0x7fffffffLL, "segger_grad_accumulate: too many elements");
    }
    b.first_block[b.n] = (int32_t)blocks;
    const dim3 grid((unsigned)(blocks > 0 ? blocks : 1));
    at += kAdamMaxTensors;
    if (at >= n_tensors) hipLaunchKernelGGL(grad_accumulate_kernel<true>, grid, dim3(256), 0, stream, b, w, n_window, window);
    else hipLaunchKernelGGL(grad_accumulate_kernel<false>, grid, dim3(256), 0, stream, b, w, n_window, window);
  } while (at < n_tensors);
  SEGGER_LAUNCH_CHECK("grad accumulate kernel");
  return SEGGER_OK;
}

extern "C" int segger_accum_window_flush(segger_accum_window* window, int32_t phase, segger_stream_t stream_) {
  SEGGER_REQUIRE(window != nullptr && is_aligned(window, 4), "segger_accum_window_flush: window is NULL or misaligned");
  SEGGER_REQUIRE(phase == 0 || phase == 1, "segger_accum_window_flush: phase %d (0: begin, 1: end)", phase);
  hipLaunchKernelGGL(accum_window_flush_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, window, phase);
  SEGGER_LAUNCH_CHECK("accum window flush kernel");
  return SEGGER_OK;
}

// ------------------------------------------------------------------------------------------------ the windowed guard and update
extern "C" int segger_grad_guard_windowed(const segger_adam_tensor* tensors, int32_t n_tensors, const segger_guard_cfg* cfg,
                                          segger_guard_state* state, void* workspace, int64_t workspace_bytes,
                                          const segger_accum_window* window, segger_stream_t stream_) {
  SEGGER_REQUIRE(window != nullptr && is_aligned(window, 4), "segger_grad_guard_windowed: window is NULL or misaligned");
  SEGGER_REQUIRE(cfg == nullptr || (cfg->flags & SEGGER_ADAM_STEPS_ADVANCED) == 0,
                 "segger_grad_guard_windowed: inside a window the step counters are never advanced ahead of the update");
  return grad_guard_launch(tensors, n_tensors, cfg, state, workspace, workspace_bytes, stream_, window);
}

extern "C" int segger_adam_step_windowed(const segger_adam_tensor* tensors, int32_t n_tensors, const double* hyper, int32_t flags,
                                         int64_t* counter, int64_t counter_inc, const segger_guard_state* state,
                                         const segger_accum_window* window, segger_stream_t stream_) {
  SEGGER_REQUIRE(hyper != nullptr && is_aligned(hyper, 8), "segger_adam_step_windowed: hyper is NULL or misaligned");
  SEGGER_REQUIRE(state == nullptr || is_aligned(state, 8), "segger_adam_step_windowed: state is misaligned");
  SEGGER_REQUIRE(window != nullptr && is_aligned(window, 4), "segger_adam_step_windowed: window is NULL or misaligned");
  SEGGER_REQUIRE((flags & SEGGER_ADAM_STEPS_ADVANCED) == 0,
                 "segger_adam_step_windowed: the step counters move only when the window closes, in this call's own launch");
  hipStream_t stream = (hipStream_t)stream_;
  bool counter_done = counter == nullptr;
  SEGGER_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || tensors), "segger_adam_step_windowed: NULL tensor table");
  for (int32_t at = 0; at < n_tensors; at += kAdamMaxTensors) {
    AdamBatch b{};
    b.hyper = hyper;
    int64_t blocks = 0;
    if (const int rc = adam_batch(tensors, n_tensors, at, true, b, blocks)) return rc;
    hipLaunchKernelGGL(adam_advance_windowed_kernel, dim3(1), dim3(64), 0, stream, b, state, window);
    if (blocks > 0) {
      if (!counter_done) { b.counter = counter; b.counter_inc = counter_inc; counter_done = true; }
      hipLaunchKernelGGL((adam_kernel<const segger_guard_state*, const segger_accum_window*>), dim3((unsigned)blocks), dim3(256), 0,
                         stream, b, state, window);
    }
    SEGGER_LAUNCH_CHECK("windowed adam kernels");
  }
  if (!counter_done) return segger_step_advance(counter, counter_inc, nullptr, stream_);     // (nothing to update)
  return SEGGER_OK;
}
