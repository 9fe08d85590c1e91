from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from .. import _lib


_FILLS = {"const": _lib.FILL_CONST, "tile": _lib.FILL_TILE, "div": _lib.FILL_DIV, "mod": _lib.FILL_MOD,
          "ramp": _lib.FILL_RAMP}


def _adam_jobs(opt):
    """[(param group, [(param, grad, exp_avg, exp_avg_sq, step)])] when ``segger_adam_step`` covers ``opt``, else None."""
    from ..optim import Adam as _Adam
    if type(opt) not in (torch.optim.Adam, _Adam):   # (not subclasses in general: torch's AdamW is one)
        return None
    # torch's AMP contract for fused optimizers (``_step_supports_amp_scaling``): ``GradScaler.step`` skips its own unscale /
    # inf check and hands both to the optimizer as ``grad_scale`` / ``found_inf``.  The kernel reads neither: torch's fused
    # step does the scaled, skippable update.
    if getattr(opt, "grad_scale", None) is not None or getattr(opt, "found_inf", None) is not None:
        return None
    jobs = []
    for g in opt.param_groups:
        if (g.get("amsgrad") or g.get("weight_decay") or g.get("maximize") or g.get("differentiable")
                or not g.get("capturable") or isinstance(g["lr"], Tensor)):
            return None
        rows = []
        for p in g["params"]:
            if p.grad is None:
                continue
            st = opt.state.get(p)
            if not st or "exp_avg" not in st:
                return None
            ts = (p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"])
            if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts) or p.grad.is_sparse:
                return None
            rows.append(ts)
        jobs.append((g, rows))
    return jobs


def adam_step_counters(opt, params=None) -> Optional[list]:
    """The step counters ``segger_adam_step`` would advance (one fp32 scalar per parameter ``params`` -- default: those with
    a gradient -- of a covered optimizer whose state exists), at most 64 in ONE parameter group; None otherwise.  A captured
    step hands them to :func:`step_draws` and then calls ``adam_step(opt, steps_advanced=True)``."""
    from ..optim import Adam as _Adam
    if type(opt) not in (torch.optim.Adam, _Adam) or len(opt.param_groups) != 1:
        return None
    g = opt.param_groups[0]
    if (g.get("amsgrad") or g.get("weight_decay") or g.get("maximize") or g.get("differentiable")
            or not g.get("capturable") or isinstance(g["lr"], Tensor)):
        return None
    out = []
    for p in (g["params"] if params is None else params):
        st = opt.state.get(p)
        if not st or "step" not in st or not st["step"].is_cuda or st["step"].dtype != torch.float32:
            return None
        out.append(st["step"])
    return out if 0 < len(out) <= 64 else None


def double_bits(x: float) -> int:
    """The int64 whose bits are the fp64 pattern of ``x`` (a ``const`` fill of a float64 buffer by :func:`stage`)."""
    import struct
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def adam_hyper(opt) -> Optional[tuple]:
    """(lr, beta1, beta2, eps) of a one-group optimizer of the kind :func:`adam_step` covers (plain capturable Adam, Python
    float learning rate; the state need not exist yet), else None."""
    from ..optim import Adam as _Adam
    if type(opt) not in (torch.optim.Adam, _Adam) or len(opt.param_groups) != 1:
        return None
    g = opt.param_groups[0]
    if (g.get("amsgrad") or g.get("weight_decay") or g.get("maximize") or g.get("differentiable")
            or not g.get("capturable") or isinstance(g["lr"], Tensor)):
        return None
    return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))


class GuardState:
    """The device side of a gradient guard (``segger_guard_state`` + the workspace of ``segger_grad_guard``), allocated
    once.  ``norm`` (float64: the unscaled global L2 norm of the last step, NaN when it was skipped), ``scale`` (float32:
    the loss scale the next backward is seeded with), ``n_skipped`` / ``n_clipped`` (int64 totals), ``skipped`` (int32,
    0 / 1: the last step), ``coef`` and ``growth_tracker`` are 0-dim VIEWS of the device struct: nothing waits for the
    device until one of them is read (``float(state.norm)``)."""

    def __init__(self, device, scale: float = 1.0):
        scale = float(scale)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"GuardState: the loss scale must be positive and finite, not {scale}")
        S = _lib.GuardState
        self.device = torch.device(device)
        self.buf = torch.zeros(C.sizeof(S), dtype=torch.uint8, device=self.device)

        def view(name, dtype):
            f = getattr(S, name)
            return self.buf[f.offset:f.offset + f.size].view(dtype).reshape(())
        self.coef, self.skipped = view("coef", torch.float32), view("skip", torch.int32)
        self.norm, self.scale = view("norm", torch.float64), view("scale", torch.float32)
        self.growth_tracker = view("growth_tracker", torch.int32)
        self.n_skipped, self.n_clipped = view("n_skipped", torch.int64), view("n_clipped", torch.int64)
        self.scale.fill_(scale)
        self.coef.fill_(1.0 / scale)
        self._workspaces: list = []          # every one ever handed out stays alive: captured graphs hold their addresses
        self._hyper: dict = {}

    def workspace(self, n_tensors: int, total_blocks: int) -> Tensor:
        need = int(_lib.load().segger_grad_guard_workspace_bytes(int(n_tensors), int(total_blocks)))
        if need < 0:
            _lib.check(need, "segger_grad_guard_workspace_bytes")
        if not self._workspaces or self._workspaces[-1].numel() < need:
            self._workspaces.append(torch.empty(max(need, 256), dtype=torch.uint8, device=self.device))
        return self._workspaces[-1]

    def hyper(self, values: tuple) -> Tensor:
        """float64[4] on the device holding ``values`` (an eager guarded step without a staged array)."""
        if values not in self._hyper:
            self._hyper[values] = torch.tensor(values, dtype=torch.float64, device=self.device)
        return self._hyper[values]


def accumulate_batches(n) -> int:
    """``accumulate_grad_batches`` as given -> the window length: an int >= 1 (1: no accumulation), else ``ValueError``."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"accumulate_grad_batches must be an int >= 1, not {n!r}")
    return n


class GradWindow:
    """The device side of gradient accumulation over ``n`` micro-steps (``segger_accum_window`` + one fp32 accumulator per
    parameter), allocated once and owned by whoever owns the optimizer's steps -- a :class:`GraphedTrainer` hands all its
    buckets one, so a window may span buckets.  ``pos`` (micro-steps summed into the open window) and ``close`` (the last
    accumulate closed it) are 0-dim int32 VIEWS of the device struct: nothing waits for the device until one is read."""

    def __init__(self, params, n: int):
        self.n = accumulate_batches(n)
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("GradWindow: no parameter requires a gradient")
        self.device = params[0].device
        self.buf = torch.zeros(C.sizeof(_lib.AccumWindow), dtype=torch.uint8, device=self.device)
        S = _lib.AccumWindow
        view = lambda name: self.buf[getattr(S, name).offset:getattr(S, name).offset + 4].view(torch.int32).reshape(())
        self.pos, self.close = view("pos"), view("close")
        self._acc: dict = {}
        self._keep: list = []                                 # (the ids stay those of live tensors)
        self.ensure(params)

    def ensure(self, params) -> None:
        """An accumulator for every parameter of ``params`` that requires a gradient and has none yet (never call this
        inside a capture: the tensor would live in the graph's pool)."""
        for p in params:
            if p.requires_grad and id(p) not in self._acc:
                self._acc[id(p)] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                self._keep.append(p)

    def acc(self, p) -> Tensor:
        """The accumulator of parameter ``p``: one tensor for the trainer's lifetime."""
        return self._acc[id(p)]

    def accumulators(self) -> list:
        return [self._acc[id(p)] for p in self._keep]


def grad_accumulate(params, window: GradWindow) -> None:
    """``segger_grad_accumulate``: ``acc = g / n`` on the first micro-step of a window, ``acc += g / n`` on the others, for the
    gradients of ``params`` (those with ``.grad`` set) in one launch per 64 tensors; the DEVICE knows the position and moves
    the window on.  Afterwards ``p.grad`` IS the accumulator: ``grad_guard`` / ``adam_step`` with ``window=`` read it."""
    rows = []
    for p in params:
        g = p.grad
        if g is None:
            continue
        a = window.acc(p)
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and not g.is_sparse and g.shape == a.shape):
            raise NotImplementedError("accumulate_grad_batches > 1: segger_grad_accumulate takes dense contiguous fp32 "
                                      f"gradients on the device, not {g.dtype} {tuple(g.shape)}")
        rows.append((a, g))
    arr = (_lib.AdamTensor * max(len(rows), 1))()
    for t, (a, g) in zip(arr, rows):
        t.param, t.grad, t.numel = a.data_ptr(), g.data_ptr(), a.numel()
    dev = window.device
    with _lib.on_device(dev):
        rc = _lib.load().segger_grad_accumulate(arr, len(rows), window.n, window.buf.data_ptr(), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_grad_accumulate")
    for p in params:
        if p.grad is not None:
            p.grad = window.acc(p)


def window_flush(window: GradWindow, phase: int) -> None:
    """``segger_accum_window_flush``: phase 0 before the close-only sequence (guard, Adam), phase 1 after it."""
    dev = window.device
    with _lib.on_device(dev):
        rc = _lib.load().segger_accum_window_flush(window.buf.data_ptr(), int(phase), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_accum_window_flush")


def adam_init_state(opt) -> None:
    """Adam's initial state (``step`` = 0 as an fp32 device scalar, zero moments -- what a capturable
    ``torch.optim.Adam._init_group`` creates on its first step) for every parameter with a gradient that has none yet: the
    kernels run on existing state only, and a guarded step cannot leave its first update to ``optimizer.step()``."""
    for g in opt.param_groups:
        for p in g["params"]:
            if p.grad is None or opt.state.get(p):
                continue
            st = opt.state[p]
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def _adam_table(rows):
    arr = (_lib.AdamTensor * len(rows))()
    for a, (p, gr, m, v, st) in zip(arr, rows):
        a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.step, a.numel = (p.data_ptr(), gr.data_ptr(), m.data_ptr(),
                                                                     v.data_ptr(), st.data_ptr(), p.numel())
    return arr


def _guarded_rows(opt, who: str):
    jobs = _adam_jobs(opt)
    jobs = None if jobs is None else [(g, rows) for g, rows in jobs if rows]
    if jobs is None or len(jobs) != 1:
        raise RuntimeError(f"{who}: the gradient guard needs an optimizer segger_adam_step covers -- a plain capturable "
                           "torch.optim.Adam (no amsgrad / weight decay / maximize, a Python float learning rate), fp32 "
                           "contiguous parameters and gradients on the device, existing state (ops.adam_init_state), no "
                           "GradScaler attached -- with exactly one parameter group that has gradients")
    return jobs[0]


def grad_guard(opt, state: GuardState, *, max_norm: Optional[float] = None, growth: float = 2.0, backoff: float = 0.5,
               growth_interval: int = 0, steps_advanced: bool = False, window: Optional["GradWindow"] = None) -> None:
    """``segger_grad_guard`` over the gradients of ``opt``'s parameters: global-norm clipping (``max_norm``; None / 0 =
    off), the loss scale ``state.scale`` the backward was seeded with (``growth_interval`` = 0: static; > 0: grown by
    ``growth`` after that many clean steps in a row, cut by ``backoff`` on a skipped one, as ``torch.amp.GradScaler``) and
    the skip on a non-finite gradient, decided on the device and left in ``state`` for ``adam_step(..., guard=state)``.
    ``steps_advanced``: Adam's step counters were advanced at the head of the step; a skipped step takes that back.
    Enqueue-only, two launches per 64 tensors.  An optimizer the Adam kernel does not cover is an error.
    ``window`` (a :class:`GradWindow` behind :func:`grad_accumulate`: ``.grad`` is the accumulator):
    ``segger_grad_guard_windowed`` -- the decision is taken, and ``state`` touched, only when the window closes."""
    if window is not None and steps_advanced:
        raise ValueError("grad_guard: inside an accumulation window Adam's counters are never advanced ahead of the update")
    g, rows = _guarded_rows(opt, "grad_guard")
    cfg = _lib.GuardCfg(float(max_norm or 0.0), float(growth), float(backoff), int(growth_interval),
                        _lib.ADAM_STEPS_ADVANCED if steps_advanced else 0)
    arr = _adam_table(rows)
    blocks = sum((r[0].numel() + _lib.ADAM_ELEMS_PER_BLOCK - 1) // _lib.ADAM_ELEMS_PER_BLOCK for r in rows)
    dev = rows[0][0].device
    ws = state.workspace(len(rows), blocks)
    with _lib.on_device(dev):
        if window is not None:
            rc = _lib.load().segger_grad_guard_windowed(arr, len(rows), C.byref(cfg), state.buf.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), window.buf.data_ptr(), _lib.stream_ptr(dev))
        else:
            rc = _lib.load().segger_grad_guard(arr, len(rows), C.byref(cfg), state.buf.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(dev))
    _lib.check(rc, "segger_grad_guard")


def adam_step(opt, steps_advanced: bool = False, counter: Optional[Tensor] = None, counter_inc: int = 0,
              hyper_dev: Optional[Tensor] = None, guard: Optional[GuardState] = None,
              window: Optional["GradWindow"] = None) -> bool:
    """``optimizer.step()`` of a plain capturable ``torch.optim.Adam`` through ``segger_adam_step``: every parameter tensor
    in two launches, on the optimizer's own state tensors (checkpoints and eager ``optimizer.step()`` calls stay
    interchangeable).  -> False, nothing done, when the optimizer is anything else (amsgrad, weight decay, maximize, a
    tensor learning rate, non-fp32 or non-contiguous parameters, state not created yet): the caller then runs
    ``optimizer.step()`` itself.  ``steps_advanced``: the step counters were advanced already (:func:`adam_step_counters`);
    ``counter`` (int64[1] on the device): ``counter += counter_inc`` rides in the update launch.  ``hyper_dev`` (float64[4]
    on the device = lr, beta1, beta2, eps; one parameter group): the kernel reads them from there when it RUNS
    (``segger_adam_step_dev``) -- a captured step follows a learning-rate schedule without a new capture.
    ``guard`` (a :class:`GuardState` that :func:`grad_guard` has just filled): ``segger_adam_step_guarded`` -- every gradient
    times ``guard.coef``, nothing written on a skipped step (``counter`` still advances); an optimizer the kernel does not
    cover is then an ERROR, not ``False``: the caller's own ``optimizer.step()`` would drop the guard.
    (Host cost ~135 us per call for 60 tensors, nearly all of it the per-tensor attribute reads; a cached launch table
    that re-checked pointers and state identity per step measured the same -- tools/host_phases.py.)
    ``window`` (a :class:`GradWindow` behind :func:`grad_accumulate`; needs ``hyper_dev``, excludes ``steps_advanced``):
    ``segger_adam_step_windowed`` -- counters, moments and parameters change only when the window closes (``counter`` still
    advances); with or without ``guard``."""
    if window is not None and (steps_advanced or hyper_dev is None):
        raise ValueError("adam_step: window= needs hyper_dev and excludes steps_advanced")
    if guard is not None:
        g, rows = _guarded_rows(opt, "adam_step")
        if hyper_dev is None:
            hyper_dev = guard.hyper((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])))
    # torch's AMP contract for fused optimizers (``_step_supports_amp_scaling``): ``GradScaler.step`` skips its own unscale /
    # inf check and hands both to the optimizer as ``grad_scale`` / ``found_inf``.  The kernel reads neither: torch's fused
    # step does the scaled, skippable update.
    jobs = _adam_jobs(opt)
    if jobs is None:
        return False
    jobs = [(g, rows) for g, rows in jobs if rows]
    if (steps_advanced or counter is not None or hyper_dev is not None) and len(jobs) != 1:
        raise RuntimeError("adam_step: advanced counters / device hyper-parameters need exactly one parameter group with gradients")
    if hyper_dev is not None and (hyper_dev.dtype != torch.float64 or hyper_dev.numel() != 4 or not hyper_dev.is_contiguous()
                                  or not hyper_dev.is_cuda):
        raise ValueError("adam_step: hyper_dev must be a contiguous float64[4] tensor on the device")
    lib = _lib.load()
    for g, rows in jobs:
        arr = _adam_table(rows)
        dev = rows[0][0].device
        b1, b2 = g["betas"]
        with _lib.on_device(dev):
            if window is not None:
                rc = lib.segger_adam_step_windowed(arr, len(rows), hyper_dev.data_ptr(), 0, _lib.ptr(counter), int(counter_inc),
                                                   guard.buf.data_ptr() if guard is not None else None,
                                                   window.buf.data_ptr(), _lib.stream_ptr(dev))
            elif guard is not None:
                rc = lib.segger_adam_step_guarded(arr, len(rows), hyper_dev.data_ptr(), 1 if steps_advanced else 0,
                                                  _lib.ptr(counter), int(counter_inc), guard.buf.data_ptr(),
                                                  _lib.stream_ptr(dev))
            elif hyper_dev is not None:
                rc = lib.segger_adam_step_dev(arr, len(rows), hyper_dev.data_ptr(), 1 if steps_advanced else 0,
                                              _lib.ptr(counter), int(counter_inc), _lib.stream_ptr(dev))
            else:
                rc = lib.segger_adam_step_ex(arr, len(rows), float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                             1 if steps_advanced else 0, _lib.ptr(counter), int(counter_inc), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_adam_step")
    return True


def float_bits(x: float) -> int:
    """The int whose low 32 bits are the fp32 pattern of ``x`` (a ``const`` fill of a float buffer)."""
    import struct
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


@torch.no_grad()
def stage(segments, device) -> None:
    """``segger_stage``: all of ``segments`` in one launch.  A segment is ``(dst, src, fill, a, b, c[, add])``: ``dst`` a
    contiguous tensor written in full; ``src`` a contiguous tensor (or None) copied to its front; the rest filled by
    ``fill`` in ("const", "tile", "div", "mod", "ramp") with integer parameters a, b, c (see include/segger_amd.h);
    ``add`` (integer segments only) is added to every copied / tile-replicated element."""
    lib = _lib.load()
    n = len(segments)
    arr = (_lib.StageSeg * n)()
    for i, seg in enumerate(segments):
        dst, src, fill, a, b, c = seg[:6]
        add = int(seg[6]) if len(seg) > 6 else 0
        if add and dst.is_floating_point():
            raise TypeError(f"stage: segment {i}: `add` is for integer segments")
        if not dst.is_contiguous() or (src is not None and not src.is_contiguous()):
            raise ValueError("stage: tensors must be contiguous")
        n_copy = 0 if src is None else int(src.numel())
        g = arr[i]
        g.dst, g.src = dst.data_ptr(), (src.data_ptr() if src is not None and src.numel() else None)
        g.n_copy, g.n_total = n_copy, int(dst.numel())
        g.a, g.b, g.c = int(a), int(b), int(c)
        g.dst_bytes, g.src_bytes = dst.element_size(), (src.element_size() if src is not None else dst.element_size())
        g.fill = _FILLS[fill]
        g.copy_add = add
        if n_copy > g.n_total:
            raise ValueError(f"stage: segment {i}: source longer than destination")
        if src is not None and src.is_floating_point() != dst.is_floating_point():
            raise TypeError(f"stage: segment {i}: no conversion between float and integer")
        if dst.is_floating_point() and src is not None and src.dtype != dst.dtype:
            raise TypeError(f"stage: segment {i}: float segments copy bit patterns, dtypes must agree")
    with _lib.on_device(device):
        rc = lib.segger_stage(arr, n, _lib.stream_ptr(device))
    _lib.check(rc, "segger_stage")
