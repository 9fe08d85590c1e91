// The optimizer step of the hot path (lightning_model.py:300-303: torch.optim.Adam, default betas / eps, no weight
// decay, no amsgrad) for ALL parameter tensors in one launch, on the optimizer's own state tensors.
//
// torch's fused multi-tensor Adam needs 3 launches for the ~60 small tensors of the encoder (one _foreach_add on the
// step counters + 2 chunked multi_tensor_apply launches: 4.8 + 24 + 14.5 us for 0.3 M parameters -- 3 % of a captured
// 1M-edge training step).  Here: one tiny launch that advances the step counters, one launch whose workgroups find
// their (tensor, offset) by a search over a prefix table carried in the kernel arguments.
#include "adam_common.h"

namespace segger {
namespace {

__global__ __launch_bounds__(64) void adam_advance_kernel(AdamBatch b) {
  for (int i = threadIdx.x; i < b.n; i += 64) *b.t[i].step += 1.0f;
}

// the same behind a gradient guard: a skipped step leaves the counters where they are
__global__ __launch_bounds__(64) void adam_advance_guarded_kernel(AdamBatch b, const segger_guard_state* __restrict__ guard) {
  if (guard->skip != 0) return;
  for (int i = threadIdx.x; i < b.n; i += 64) *b.t[i].step += 1.0f;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int segger_adam_step(const segger_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2,
                                double eps, segger_stream_t stream_) {
  return segger_adam_step_ex(tensors, n_tensors, lr, beta1, beta2, eps, 0, nullptr, 0, stream_);
}

static int adam_launch(const segger_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2, double eps,
                       const double* hyper, int32_t flags, int64_t* counter, int64_t counter_inc,
                       const segger_guard_state* guard, segger_stream_t stream_);

extern "C" int segger_adam_step_ex(const segger_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2,
                                   double eps, int32_t flags, int64_t* counter, int64_t counter_inc, segger_stream_t stream_) {
  SEGGER_REQUIRE(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.,
                 "segger_adam_step: lr / betas / eps out of range");
  return adam_launch(tensors, n_tensors, lr, beta1, beta2, eps, nullptr, flags, counter, counter_inc, nullptr, stream_);
}

extern "C" int segger_adam_step_dev(const segger_adam_tensor* tensors, int32_t n_tensors, const double* hyper, int32_t flags,
                                    int64_t* counter, int64_t counter_inc, segger_stream_t stream_) {
  SEGGER_REQUIRE(hyper != nullptr && is_aligned(hyper, 8), "segger_adam_step_dev: hyper is NULL or misaligned");
  return adam_launch(tensors, n_tensors, 0., 0., 0., 0., hyper, flags, counter, counter_inc, nullptr, stream_);
}

extern "C" int segger_adam_step_guarded(const segger_adam_tensor* tensors, int32_t n_tensors, const double* hyper, int32_t flags,
                                        int64_t* counter, int64_t counter_inc, const segger_guard_state* state,
                                        segger_stream_t stream_) {
  SEGGER_REQUIRE(hyper != nullptr && is_aligned(hyper, 8), "segger_adam_step_guarded: hyper is NULL or misaligned");
  SEGGER_REQUIRE(state != nullptr && is_aligned(state, 8), "segger_adam_step_guarded: state is NULL or misaligned");
  return adam_launch(tensors, n_tensors, 0., 0., 0., 0., hyper, flags, counter, counter_inc, state, stream_);
}

static int adam_launch(const segger_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2, double eps,
                       const double* hyper, int32_t flags, int64_t* counter, int64_t counter_inc,
                       const segger_guard_state* guard, segger_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool advanced = (flags & SEGGER_ADAM_STEPS_ADVANCED) != 0;
  bool counter_done = counter == nullptr;
  SEGGER_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || tensors), "segger_adam_step: NULL tensor table");
  for (int32_t at = 0; at < n_tensors; at += kAdamMaxTensors) {
    AdamBatch b{};
    b.lr = lr; b.beta1 = beta1; b.beta2 = beta2; b.eps = eps; b.hyper = hyper;
    int64_t blocks = 0;
    if (const int rc = adam_batch(tensors, n_tensors, at, true, b, blocks)) return rc;
    if (!advanced) {
      if (guard) hipLaunchKernelGGL(adam_advance_guarded_kernel, dim3(1), dim3(64), 0, stream, b, guard);
      else hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, stream, b);
    }
    if (blocks > 0) {
      if (!counter_done) { b.counter = counter; b.counter_inc = counter_inc; counter_done = true; }
      if (guard) hipLaunchKernelGGL(adam_kernel<const segger_guard_state*>, dim3((unsigned)blocks), dim3(256), 0, stream, b, guard);
      else hipLaunchKernelGGL(adam_kernel<>, dim3((unsigned)blocks), dim3(256), 0, stream, b);
    }
    SEGGER_LAUNCH_CHECK("adam kernels");
  }
  if (!counter_done) return segger_step_advance(counter, counter_inc, nullptr, stream_);     // (nothing to update)
  return SEGGER_OK;
}

// ------------------------------------------------------------------------------------------------ the gradient guard
extern "C" int64_t segger_grad_guard_workspace_bytes(int32_t n_tensors, int64_t total_blocks) {
  SEGGER_REQUIRE(n_tensors >= 0 && total_blocks >= 0, "segger_grad_guard_workspace_bytes: negative n_tensors or total_blocks");
  SEGGER_REQUIRE(total_blocks < (1LL << 40), "segger_grad_guard_workspace_bytes: too many blocks");
  return (int64_t)guard_workspace(n_tensors, total_blocks, nullptr);
}

extern "C" int segger_grad_guard(const segger_adam_tensor* tensors, int32_t n_tensors, const segger_guard_cfg* cfg,
                                 segger_guard_state* state, void* workspace, int64_t workspace_bytes, segger_stream_t stream_) {
  return grad_guard_launch(tensors, n_tensors, cfg, state, workspace, workspace_bytes, stream_);
}
