"""Float64 oracle of the gradient guard's state transition (include/segger_amd.h: segger_guard_state), and hand-worked
cases.  What it stands for: ``scaler.unscale_(opt); clip_grad_norm_(params, max_norm); scaler.step(opt); scaler.update()``
decided in one place -- the (loss-scaled) gradients, the state before and the configuration go in; what the update
multiplies every gradient by, whether the step is skipped, the reported norm and the state after come out.  Plain numpy /
math, no torch: tests/test_grad_guard_cases.py holds it to the hand-worked numbers and to torch's own clipping and scaler
recurrence, tests/test_gpu_grad_guard.py holds the kernels to it."""
import math

import numpy as np

F32 = np.float32


def fresh_state(scale=1.0, growth_tracker=0, n_skipped=0, n_clipped=0):
    return dict(scale=F32(scale), growth_tracker=int(growth_tracker), n_skipped=int(n_skipped), n_clipped=int(n_clipped))


def config(max_norm=0.0, growth=2.0, backoff=0.5, growth_interval=0):
    return dict(max_norm=float(max_norm), growth=float(growth), backoff=float(backoff), growth_interval=int(growth_interval))


def guard_step(grads, state, cfg):
    """-> dict(coef, skip, norm, scale, growth_tracker, n_skipped, n_clipped).  ``grads``: float32 arrays of any shape
    (the gradients as the backward left them: times ``state['scale']``).  The sum of squares is exact to the last bit
    (``math.fsum`` of exact float64 squares of float32 values); everything after it is float64 until the final casts."""
    flat = [np.asarray(g, dtype=F32).reshape(-1) for g in grads]
    skip = int(any(not np.isfinite(g).all() for g in flat))
    scale = float(state["scale"])
    out = dict(state)
    if skip:
        out.update(coef=F32(0.0), skip=1, norm=math.nan, n_skipped=state["n_skipped"] + 1)
        if cfg["growth_interval"] > 0:
            out.update(scale=F32(scale * cfg["backoff"]), growth_tracker=0)
        return out
    total = math.fsum(math.fsum((g.astype(np.float64) ** 2).tolist()) for g in flat)
    norm = math.sqrt(total) / scale
    clip = min(1.0, cfg["max_norm"] / (norm + 1e-6)) if cfg["max_norm"] > 0 else 1.0
    out.update(coef=F32(clip / scale), skip=0, norm=norm, n_clipped=state["n_clipped"] + int(clip < 1.0))
    if cfg["growth_interval"] > 0:
        out["growth_tracker"] = state["growth_tracker"] + 1
        if out["growth_tracker"] == cfg["growth_interval"]:
            out.update(scale=F32(scale * cfg["growth"]), growth_tracker=0)
    return out


def next_state(result):
    return {k: result[k] for k in ("scale", "growth_tracker", "n_skipped", "n_clipped")}


def _tail(n, value):
    g = np.full(n, 0.5, dtype=F32)
    g[-1] = value
    return g


NAN, INF = float("nan"), float("inf")

# (name, gradients, state before, configuration, expected) -- every expected number worked out by hand:
CASES = [
    # |(3, 4)| = 5 = max_norm exactly: torch's formula still divides by norm + 1e-6, so the clip factor is a hair below 1
    # (5 / 5.000001 = 0.99999980000004) and the step counts as clipped
    ("norm_exactly_at_max_norm", [[3.0, 4.0]], fresh_state(1.0), config(max_norm=5.0),
     dict(coef=F32(0.99999980000004), skip=0, norm=5.0, scale=F32(1.0), growth_tracker=0, n_skipped=0, n_clipped=1)),
    # clipping off, scale 2: the true norm is 5 / 2, the gradients are only unscaled
    ("max_norm_zero_is_clipping_off", [[3.0], [4.0]], fresh_state(2.0), config(max_norm=0.0),
     dict(coef=F32(0.5), skip=0, norm=2.5, scale=F32(2.0), growth_tracker=0, n_skipped=0, n_clipped=0)),
    # all zero: min(1, 1 / (0 + 1e-6)) = 1, no division by zero, coef = 1 / scale
    ("all_zero_gradients", [np.zeros((3, 5)), np.zeros(7), np.zeros(0)], fresh_state(8.0), config(max_norm=1.0),
     dict(coef=F32(0.125), skip=0, norm=0.0, scale=F32(8.0), growth_tracker=0, n_skipped=0, n_clipped=0)),
    # a clipped step under a scale: |(6, 8)| / 2 = 5, max_norm 1 -> clip = 1 / 5.000001, coef = clip / 2
    ("clipped_under_a_scale", [[6.0, 8.0]], fresh_state(2.0, n_clipped=4), config(max_norm=1.0),
     dict(coef=F32(0.09999998000000400), skip=0, norm=5.0, scale=F32(2.0), growth_tracker=0, n_skipped=0, n_clipped=5)),
    # one inf, dynamic scale: skipped, the scale backs off and the tracker goes back to 0
    ("one_inf_backs_off_and_resets_the_tracker", [[1.0, 2.0], [INF, 0.0]], fresh_state(1024.0, growth_tracker=3),
     config(max_norm=1.0, growth_interval=5),
     dict(coef=F32(0.0), skip=1, norm=NAN, scale=F32(512.0), growth_tracker=0, n_skipped=1, n_clipped=0)),
    ("one_negative_inf", [[-INF]], fresh_state(4.0), config(growth_interval=2),
     dict(coef=F32(0.0), skip=1, norm=NAN, scale=F32(2.0), growth_tracker=0, n_skipped=1, n_clipped=0)),
    # one NaN, STATIC scale (growth_interval 0 = never change): skipped, the scale stays
    ("one_nan_static_scale", [[1.0], [NAN, 3.0]], fresh_state(1024.0, n_skipped=2), config(max_norm=1.0),
     dict(coef=F32(0.0), skip=1, norm=NAN, scale=F32(1024.0), growth_tracker=0, n_skipped=3, n_clipped=0)),
    # a NaN in the last element of odd-sized tensors: the scalar tail of a block (7 elements; 2049 = one past a block)
    ("nan_in_the_last_element_of_an_odd_tensor", [np.ones(4), _tail(7, NAN)], fresh_state(1.0), config(),
     dict(coef=F32(0.0), skip=1, norm=NAN, scale=F32(1.0), growth_tracker=0, n_skipped=1, n_clipped=0)),
    ("nan_one_past_a_block", [_tail(2049, NAN)], fresh_state(1.0), config(),
     dict(coef=F32(0.0), skip=1, norm=NAN, scale=F32(1.0), growth_tracker=0, n_skipped=1, n_clipped=0)),
    # growth on exactly the growth_interval-th clean step, not before: interval 3, tracker 1 -> 2 (no growth) ...
    ("no_growth_before_the_interval", [[0.0, 2.0]], fresh_state(16.0, growth_tracker=1), config(growth_interval=3),
     dict(coef=F32(0.0625), skip=0, norm=0.125, scale=F32(16.0), growth_tracker=2, n_skipped=0, n_clipped=0)),
    # ... tracker 2 -> 3 = the interval: the scale doubles, the tracker restarts; coef still uses the scale of THIS step
    ("growth_on_the_interval", [[0.0, 2.0]], fresh_state(16.0, growth_tracker=2), config(growth_interval=3),
     dict(coef=F32(0.0625), skip=0, norm=0.125, scale=F32(32.0), growth_tracker=0, n_skipped=0, n_clipped=0)),
    ("growth_interval_one_grows_every_clean_step", [[1.0]], fresh_state(1.0), config(growth=4.0, growth_interval=1),
     dict(coef=F32(1.0), skip=0, norm=1.0, scale=F32(4.0), growth_tracker=0, n_skipped=0, n_clipped=0)),
]
