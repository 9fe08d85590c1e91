from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE
from ..graph import EdgeCSR
from .. import ops                # route switches: read as ops.NAME when called, never bound here
from ._common import _defer_keep, _f32_vec, _rows, _vendor_gemm, _wgrad_ws_bytes
from .packs import _pack_for, f32_split_planes


# --------------------------------------------------------------------------
# Tall-skinny projection GEMM (MFMA) with autograd
# --------------------------------------------------------------------------
def linear_supported(k_in: int, m_out: int, dtype: torch.dtype) -> bool:
    return dtype in DTYPE_CODE and bool(_lib.load().segger_linear_supported(int(k_in), int(m_out), DTYPE_CODE[dtype]))


def linear_fwd_launch(x: Tensor, w: Tensor, bias: Optional[Tensor], out: Optional[Tensor] = None) -> Tensor:
    """y = x @ w.T + bias for a [n, K] activation (row stride allowed) and contiguous [M, K] weight."""
    _lib.require_cuda(x, w)
    lib = _lib.load()
    n, k = x.shape
    m = w.shape[0]
    if w.dtype != x.dtype or not w.is_contiguous() or w.shape[1] != k:
        raise ValueError("linear: weight must be contiguous [M, K] in the activation dtype")
    xp, ldx = _rows(x, k, "x")
    y = out if out is not None else torch.empty((n, m), dtype=x.dtype, device=x.device)
    yp, ldy = _rows(y, m, "y")
    b = _f32_vec(bias, m, "bias")
    with _lib.on_device(x.device):
        rc = lib.segger_linear_fwd(xp, ldx, w.data_ptr(), _lib.ptr(b), yp, ldy, n, k, m, DTYPE_CODE[x.dtype],
                                   _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_fwd")
    return y


def linear_f32_gate_launch(x: Tensor, w: Tensor, gate: Tensor, kind: str) -> Tensor:
    """``(x @ w.T) * act'(gate)`` at fp32 storage, ``kind`` in ("gelu", "silu") (``segger_linear_fwd_f32_gate``): the data
    gradient through an activation in one kernel; on the bf16x3 split when :data:`F32_SPLIT` covers the shape."""
    _lib.require_cuda(x, w, gate)
    n, k = x.shape
    m = int(w.shape[0])
    if x.dtype != torch.float32 or gate.dtype != torch.float32 or tuple(gate.shape) != (n, m) or w.shape[1] != k:
        raise ValueError("linear_f32_gate: x fp32 [n, K], w [M, K], gate fp32 [n, M]")
    xp, ldx = _rows(x, k, "x")
    gp, ldg = _rows(gate, m, "gate")
    y = torch.empty((n, m), dtype=torch.float32, device=x.device)
    split = ops.F32_SPLIT and ldx % 4 == 0 and linear_f32_split_supported(k, m)
    wq = f32_split_planes(w) if split else w.detach().float().contiguous()
    with _lib.on_device(x.device):
        rc = _lib.load().segger_linear_fwd_f32_gate(xp, ldx, wq.data_ptr(), int(split), gp, ldg, {"gelu": 1, "silu": 2}[kind],
                                                    y.data_ptr(), m, n, k, m, _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_fwd_f32_gate")
    return y


def linear_f32_act_launch(x: Tensor, w: Tensor, bias: Optional[Tensor], kind: str) -> Tuple[Tensor, Tensor]:
    """``(y, act(y))`` with ``y = x @ w.T + bias`` at fp32 storage from ONE kernel (``segger_linear_fwd_f32_act``; exact-fp32
    MFMA, K in 64 / 128 / 256), ``kind`` in ("gelu", "silu")."""
    _lib.require_cuda(x, w)
    n, k = x.shape
    m = int(w.shape[0])
    if x.dtype != torch.float32 or w.dtype != torch.float32 or w.shape[1] != k or not w.is_contiguous():
        raise ValueError("linear_f32_act: x fp32 [n, K], w contiguous fp32 [M, K]")
    xp, ldx = _rows(x, k, "x")
    y = torch.empty((n, m), dtype=torch.float32, device=x.device)
    ya = torch.empty((n, m), dtype=torch.float32, device=x.device)
    b = None if bias is None else bias.detach().float().contiguous()
    with _lib.on_device(x.device):
        rc = _lib.load().segger_linear_fwd_f32_act(xp, ldx, w.data_ptr(), _lib.ptr(b), y.data_ptr(), m, ya.data_ptr(), m,
                                                   {"gelu": 1, "silu": 2}[kind], n, k, m, _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_fwd_f32_act")
    return y, ya


def linear_f32_gate_supported(k_in: int, m_out: int) -> bool:
    return (m_out % 64 == 0 and k_in in (64, 128, 256)) or (ops.F32_SPLIT and linear_f32_split_supported(k_in, m_out))


def linear_f32_split_supported(k_in: int, m_out: int) -> bool:
    return bool(_lib.load().segger_linear_fwd_f32_split_supported(int(k_in), int(m_out)))


def linear_f32_split_launch(x: Tensor, w3: Tensor, bias: Optional[Tensor]) -> Tensor:
    """y = x @ w.T + bias for fp32 ``x`` [n, K] on the bf16 matrix pipe (``segger_linear_fwd_f32_split``: three-way bf16
    split of both operands, six partial products, fp32 accumulation); ``w3`` = :func:`f32_split_planes` of w."""
    _lib.require_cuda(x, w3)
    n, k = x.shape
    m = int(w3.shape[1])
    if x.dtype != torch.float32 or w3.dtype != torch.bfloat16 or tuple(w3.shape) != (3, m, k) or not w3.is_contiguous():
        raise ValueError("linear_f32_split: x fp32 [n, K], w3 contiguous bf16 [3, M, K]")
    xp, ldx = _rows(x, k, "x")
    y = torch.empty((n, m), dtype=torch.float32, device=x.device)
    b = _f32_vec(bias, m, "bias")
    with _lib.on_device(x.device):
        rc = _lib.load().segger_linear_fwd_f32_split(xp, ldx, w3.data_ptr(), _lib.ptr(b), y.data_ptr(), m, n, k, m,
                                                     _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_fwd_f32_split")
    return y


def colsum(x: Tensor) -> Tensor:
    """fp32 column sums of a [n, cols] matrix (row stride allowed): the bias gradient ``grad_out.sum(0)``."""
    _lib.require_cuda(x)
    lib = _lib.load()
    n, cols = x.shape
    if x.dtype not in DTYPE_CODE or cols % 8 != 0 or cols > 2048:
        return x.sum(0, dtype=torch.float32)
    xp, ld = _rows(x, cols, "x")
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws_bytes = lib.segger_colsum_workspace_bytes(n, cols)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.segger_colsum(xp, ld, n, cols, DTYPE_CODE[x.dtype], out.data_ptr(), ws.data_ptr(), ws_bytes,
                               _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_colsum")
    return out


def segment_rowsum(x: Tensor, by_id: EdgeCSR) -> Tensor:
    """fp32 [n_ids, D]: sum of the rows of ``x`` grouped by id (``by_id`` = :func:`rows_by_id` of the row ids)."""
    _lib.require_cuda(x)
    lib = _lib.load()
    n, d = x.shape
    n_seg = by_id.n_rows
    xp, ld = _rows(x, d, "x")
    out = torch.empty((n_seg, d), dtype=torch.float32, device=x.device)
    ws_bytes = lib.segger_segment_rowsum_workspace_bytes(n, n_seg, d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.segger_segment_rowsum(xp, ld, n, d, DTYPE_CODE[x.dtype], by_id.indptr.data_ptr(),
                                       by_id.col.data_ptr() if n else None, n_seg, out.data_ptr(), ws.data_ptr(),
                                       ws_bytes, _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_segment_rowsum")
    return out


def linear_wgrad_supported(m_out: int, k_in: int, dtype: torch.dtype) -> bool:
    return dtype in DTYPE_CODE and bool(_lib.load().segger_linear_wgrad_supported(int(m_out), int(k_in), DTYPE_CODE[dtype]))


def linear_wgrad_launch(gy: Tensor, x: Tensor, want_bias: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """(dW[M, K], db[M]) fp32 of ``y = x @ W.T + b`` from ``gy`` [n, M] and ``x`` [n, K] (row strides allowed):
    one pass over both matrices on the MFMA weight-gradient kernel (``segger_linear_wgrad``)."""
    _lib.require_cuda(gy, x)
    lib = _lib.load()
    n, m = gy.shape
    k = x.shape[1]
    if x.shape[0] != n or gy.dtype != x.dtype:
        raise ValueError("linear_wgrad: gy / x must share the row count and the dtype")
    gp, ldg = _rows(gy, m, "gy")
    xp, ldx = _rows(x, k, "x")
    gw = torch.empty((m, k), dtype=torch.float32, device=x.device)
    gb = torch.empty(m, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = _wgrad_ws_bytes(n, m, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    split = (ops.F32_SPLIT and ops.F32_SPLIT_WGRAD and x.dtype == torch.float32 and ldg % 4 == 0 and ldx % 4 == 0
             and bool(lib.segger_linear_wgrad_f32_split_supported(m, k)))
    with _lib.on_device(x.device):
        if split:        # fp32 storage: six bf16 partial products instead of the exact-fp32 MFMA (see F32_SPLIT)
            rc = lib.segger_linear_wgrad_f32_split(gp, ldg, xp, ldx, n, m, k, gw.data_ptr(), _lib.ptr(gb), ws.data_ptr(),
                                                   ws_bytes, _lib.stream_ptr(x.device))
        else:
            rc = lib.segger_linear_wgrad(gp, ldg, xp, ldx, n, m, k, DTYPE_CODE[x.dtype], gw.data_ptr(), _lib.ptr(gb),
                                         ws.data_ptr(), ws_bytes, _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_wgrad")
    _defer_keep(ws, gw, gb)
    return gw, gb


def linear_wgrad_dx_supported(m_out: int, k_in: int, dtype: torch.dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and bool(
        _lib.load().segger_linear_wgrad_dx_supported(int(m_out), int(k_in), DTYPE_CODE[dtype]))


def linear_wgrad_dx_gate_supported(m_out: int, k_in: int, dtype: torch.dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and bool(
        _lib.load().segger_linear_wgrad_dx_gate_supported(int(m_out), int(k_in), DTYPE_CODE[dtype]))


def linear_wgrad_dx_launch(gy: Tensor, x: Tensor, wt: Tensor, want_bias: bool = True, gate: Optional[Tensor] = None
                           ) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """(dX[n, K], dW[M, K], db[M]) of ``y = x @ W.T + b`` in ONE pass over ``gy`` [n, M] (``segger_linear_wgrad_dx``):
    ``wt`` = W^T [K, M] contiguous in the activation dtype; dX in the activation dtype, dW / db fp32.  ``gate`` [n, K]:
    dX comes multiplied by gelu'(gate) (x was gelu(gate); ``linear_wgrad_dx_gate_supported``)."""
    _lib.require_cuda(gy, x, wt)
    lib = _lib.load()
    n, m = gy.shape
    k = x.shape[1]
    if x.shape[0] != n or gy.dtype != x.dtype or wt.dtype != x.dtype or tuple(wt.shape) != (k, m) or not wt.is_contiguous():
        raise ValueError("linear_wgrad_dx: gy [n, M], x [n, K] and a contiguous W^T [K, M] of one dtype")
    gp, ldg = _rows(gy, m, "gy")
    xp, ldx = _rows(x, k, "x")
    qp, ldq = None, 0
    if gate is not None:
        if tuple(gate.shape) != (n, k) or gate.dtype != x.dtype:
            raise ValueError("linear_wgrad_dx: gate must be [n, K] in the activation dtype")
        _lib.require_cuda(gate)
        qp, ldq = _rows(gate, k, "gate")
    gx = torch.empty((n, k), dtype=x.dtype, device=x.device)
    gw = torch.empty((m, k), dtype=torch.float32, device=x.device)
    gb = torch.empty(m, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = _wgrad_ws_bytes(n, m, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = lib.segger_linear_wgrad_dx(gp, ldg, xp, ldx, wt.data_ptr(), n, m, k, DTYPE_CODE[x.dtype], gw.data_ptr(),
                                        _lib.ptr(gb), gx.data_ptr(), k, qp, ldq, ws.data_ptr(), ws_bytes,
                                        _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_wgrad_dx")
    _defer_keep(ws, gw, gb)
    return gx, gw, gb


def linear_fwd_pair_launch(xa: Tensor, wa: Tensor, xb: Tensor, wb: Tensor) -> Tuple[Tensor, Tensor]:
    """``(xa @ wa.T, xb @ wb.T)`` for 16-bit activations whose widths may differ (``segger_linear_fwd_pair_k``: one launch
    for widths (384, 128) or equal widths -- a first layer's two data gradients -- two otherwise)."""
    _lib.require_cuda(xa, wa, xb, wb)
    args, outs = [], []
    for x, w in ((xa, wa), (xb, wb)):
        n, k = x.shape
        m = int(w.shape[0])
        if w.dtype != x.dtype or not w.is_contiguous() or w.shape[1] != k:
            raise ValueError("linear_fwd_pair: weights must be contiguous [M, K] in the activation dtype")
        y = torch.empty((n, m), dtype=x.dtype, device=x.device)
        a = _lib.LinearArgs()
        a.x, a.ldx = _rows(x, k, "x")
        a.w, a.y, a.ldy, a.n_rows, a.m_out = w.data_ptr(), y.data_ptr(), m, n, m
        args.append(a)
        outs.append(y)
    with _lib.on_device(xa.device):
        rc = _lib.load().segger_linear_fwd_pair_k(C.byref(args[0]), int(xa.shape[1]), C.byref(args[1]), int(xb.shape[1]),
                                                  DTYPE_CODE[xa.dtype], _lib.stream_ptr(xa.device))
    _lib.check(rc, "segger_linear_fwd_pair_k")
    return outs[0], outs[1]


def linear_wgrad_pair_launch(sides, dx: bool):
    """``sides`` = two (gy [n, M], x [n, K], wt [K, M] | None, want_bias) of one K and dtype -> [(gx | None, gw, gb | None)] * 2 from
    ONE launch (``segger_linear_wgrad_pair``; ``dx``: the one-pass form with the data gradients, else dW / db only)."""
    lib = _lib.load()
    dev, dt = sides[0][0].device, sides[0][1].dtype
    args, outs, keep = [], [], []
    for gy, x, wt, want_bias in sides:
        _lib.require_cuda(gy, x)
        n, m = gy.shape
        k = x.shape[1]
        if x.shape[0] != n or gy.dtype != dt or x.dtype != dt:
            raise ValueError("linear_wgrad_pair: gy / x must share the row count and the dtype")
        a = _lib.WgradArgs()
        a.dy, a.ld_dy = _rows(gy, m, "gy")
        a.x, a.ld_x = _rows(x, k, "x")
        a.n_rows, a.m_out = n, m
        gx = None
        if dx:
            if wt.dtype != dt or tuple(wt.shape) != (k, m) or not wt.is_contiguous():
                raise ValueError("linear_wgrad_pair: W^T must be contiguous [K, M] in the activation dtype")
            gx = torch.empty((n, k), dtype=dt, device=dev)
            a.w_t, a.dx, a.ld_dx = wt.data_ptr(), gx.data_ptr(), k
        gw = torch.empty((m, k), dtype=torch.float32, device=dev)
        gb = torch.empty(m, dtype=torch.float32, device=dev) if want_bias else None
        ws_bytes = _wgrad_ws_bytes(n, m, k)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        a.grad_w, a.grad_b, a.workspace, a.workspace_bytes = gw.data_ptr(), _lib.ptr(gb), ws.data_ptr(), ws_bytes
        args.append(a)
        outs.append((gx, gw, gb))
        keep.append((ws, gw, gb))
    with _lib.on_device(dev):
        rc = lib.segger_linear_wgrad_pair(C.byref(args[0]), C.byref(args[1]), int(sides[0][1].shape[1]), DTYPE_CODE[dt],
                                          _lib.stream_ptr(dev))
    _lib.check(rc, "segger_linear_wgrad_pair")
    for kk in keep:
        _defer_keep(*kk)
    return outs


def _weight_grad_gemm(gy: Tensor, x: Tensor) -> Tensor:
    """dW[M, K] = gy^T x as a plain library GEMM: shapes the MFMA weight-gradient kernel does not cover
    (``linear_wgrad_supported``).  fp32 result."""
    _vendor_gemm("weight gradient dW = dY^T X", x.shape[1], gy.shape[1], x.dtype)
    return (gy.t() @ x).float()


class _Linear(torch.autograd.Function):
    """x [n, K] (bf16/f16); ``n_w`` fp32 master weights [M_i, K] stacked by rows, ``n_w`` fp32 biases (or None)
    -> [n, sum M_i].  Forward, the data gradient and the weight / bias gradients run on the hand-written MFMA kernels
    (csrc/linear.hip, csrc/linear_wgrad.hip); each parameter's gradient is a row window of the one fused result."""

    @staticmethod
    def forward(ctx, x, n_w, *params):
        weights, biases = params[:n_w], params[n_w:]
        pk = _pack_for(weights, biases).get(x.dtype, x.device)
        if ops.F32_SPLIT and x.dtype == torch.float32 and linear_f32_split_supported(x.shape[1], pk.w.shape[0]):
            y = linear_f32_split_launch(x, pk.planes(), pk.b)
        else:
            y = linear_fwd_launch(x, pk.w, pk.b)
        ctx.save_for_backward(x)
        ctx.n_w = n_w
        _linear_save(ctx, pk, weights, biases)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return _linear_backward(ctx, x, gy, ctx.needs_input_grad[0], ctx.needs_input_grad[2:])


def _linear_save(ctx, pk, weights, biases) -> None:
    ctx.pack = pk
    ctx.rows = [int(w.shape[0]) for w in weights]
    ctx.has_bias = [b is not None for b in biases]
    # the pack is refreshed IN PLACE after an optimizer step; a backward that runs later than that (not the case in
    # forward -> backward -> step training) would see the new weights: remember which generation this forward used
    ctx.w, ctx.wt_of, ctx.w_key = pk.w, pk, pk.key


def _grad_rows(gy: Tensor, dt) -> Tensor:
    if gy.dtype != dt:
        gy = gy.to(dt)
    if gy.dim() != 2 or (gy.shape[0] > 1 and gy.stride(1) != 1):
        gy = gy.contiguous()
    return gy


def _linear_backward(st, x, gy, need_x: bool, need_params, pre=None) -> tuple:
    """-> (gx, None, *grads_w, *grads_b) of one projection; ``st`` holds what :func:`_linear_save` left, ``need_params`` =
    needs_input_grad of its weights then biases; ``pre`` = (gx | None, gw, gb) already computed by a paired launch."""
    dt = x.dtype
    n_w = len(st.rows)
    gy = _grad_rows(gy, dt)
    w = st.w
    m, k = w.shape
    gx = None
    want_w = any(need_params[:n_w])
    want_b = any(h and g for h, g in zip(st.has_bias, need_params[n_w:]))
    gw = gb = None
    if pre is not None:
        gx, gw, gb = pre
    if need_x and gx is None:
        if st.wt_of.key != st.w_key:
            raise RuntimeError("the projection weights changed between this forward and its backward "
                               "(optimizer step in between?): run backward before stepping")
        # (st.wt_of.wt = W^T [K, M], dX = dY @ W -- asked for only where it is read: at fp32 storage the split kernels take
        #  the transposed PLANES instead, and the property's transposing copy was one stray launch per projection and step)
        if (ops.FUSED_WGRAD_DX and (want_w or want_b) and x.shape[0] > 0 and linear_wgrad_dx_supported(m, k, dt)):
            gx, gw, gb = linear_wgrad_dx_launch(gy, x, st.wt_of.wt, want_bias=want_b)    # dY read ONCE for dX, dW and db
        elif ops.F32_SPLIT and dt == torch.float32 and linear_f32_split_supported(m, k):
            gx = linear_f32_split_launch(gy, st.wt_of.planes(transposed=True), None)
        elif linear_supported(m, k, dt):
            gx = linear_fwd_launch(gy, st.wt_of.wt, None)
        else:
            _vendor_gemm("data gradient dX = dY W", m, k, dt)
            gx = gy @ w
    if gw is not None:
        pass
    elif (want_w or want_b) and x.shape[0] > 0 and linear_wgrad_supported(m, k, dt):
        gw, gb = linear_wgrad_launch(gy, x, want_bias=want_b)       # dY and X read once for both
    else:
        if want_w:
            gw = _weight_grad_gemm(gy, x)
        if want_b:
            gb = colsum(gy)
    grads_w, grads_b, r0 = [], [], 0
    for i, r in enumerate(st.rows):
        grads_w.append(gw[r0:r0 + r] if (gw is not None and need_params[i]) else None)
        grads_b.append(gb[r0:r0 + r] if (gb is not None and st.has_bias[i] and need_params[n_w + i]) else None)
        r0 += r
    return (gx, None) + tuple(grads_w) + tuple(grads_b)


class _State:
    pass


class _LinearPair(torch.autograd.Function):
    """Two projections with the same K as one launch (``segger_linear_fwd_pair``): (xa, xb, n_wa, n_wb, *weights_a,
    *biases_a, *weights_b, *biases_b) -> (ya, yb).  Backward: each side's own :func:`_linear_backward`."""

    @staticmethod
    def forward(ctx, xa, xb, n_wa, n_wb, *params):
        pa, pb = params[:2 * n_wa], params[2 * n_wa:]
        lib = _lib.load()
        sides, args, outs = [], [], []
        for x, n_w, pp in ((xa, n_wa, pa), (xb, n_wb, pb)):
            weights, biases = pp[:n_w], pp[n_w:]
            pk = _pack_for(weights, biases).get(x.dtype, x.device)
            st = _State()
            _linear_save(st, pk, weights, biases)
            sides.append(st)
            n, k = x.shape
            m = int(pk.w.shape[0])
            y = torch.empty((n, m), dtype=x.dtype, device=x.device)
            a = _lib.LinearArgs()
            a.x, a.ldx = _rows(x, k, "x")
            a.w, a.bias = pk.w.data_ptr(), _lib.ptr(_f32_vec(pk.b, m, "bias"))
            a.y, a.ldy = _rows(y, m, "y")
            a.n_rows, a.m_out = n, m
            args.append(a)
            outs.append(y)
        with _lib.on_device(xa.device):
            rc = lib.segger_linear_fwd_pair(C.byref(args[0]), C.byref(args[1]), int(xa.shape[1]), DTYPE_CODE[xa.dtype],
                                            _lib.stream_ptr(xa.device))
        _lib.check(rc, "segger_linear_fwd_pair")
        ctx.save_for_backward(xa, xb)
        ctx.sides, ctx.n_w = sides, (n_wa, n_wb)
        return outs[0], outs[1]

    @staticmethod
    def backward(ctx, gya, gyb):
        xa, xb = ctx.saved_tensors
        n_wa, n_wb = ctx.n_w
        need = ctx.needs_input_grad
        na, nb = need[4:4 + 2 * n_wa], need[4 + 2 * n_wa:]
        pre = (None, None)
        sts = ctx.sides
        dt = xa.dtype
        wants = [any(nn[:len(st.rows)]) or any(h and g for h, g in zip(st.has_bias, nn[len(st.rows):]))
                 for st, nn in zip(sts, (na, nb))]
        if (ops.WGRAD_PAIR and all(wants) and gya is not None and gyb is not None and dt in (torch.bfloat16, torch.float16)
                and xa.shape[0] > 0 and xb.shape[0] > 0):
            # both sides' backward passes in one launch: with the data gradients when both want them and the one-pass
            # kernel covers both shapes, else the weight / bias gradients only
            k = int(xa.shape[1])
            ms = [int(st.w.shape[0]) for st in sts]
            dx = (ops.FUSED_WGRAD_DX and need[0] and need[1] and all(linear_wgrad_dx_supported(m, k, dt) for m in ms))
            if dx or all(linear_wgrad_supported(m, k, dt) for m in ms):
                for st in sts:
                    if dx and st.wt_of.key != st.w_key:
                        raise RuntimeError("the projection weights changed between this forward and its backward "
                                           "(optimizer step in between?): run backward before stepping")
                gya, gyb = _grad_rows(gya, dt), _grad_rows(gyb, dt)
                bias = [any(h and g for h, g in zip(st.has_bias, nn[len(st.rows):])) for st, nn in zip(sts, (na, nb))]
                pre = linear_wgrad_pair_launch([(gya, xa, sts[0].wt_of.wt if dx else None, bias[0]),
                                                (gyb, xb, sts[1].wt_of.wt if dx else None, bias[1])], dx)
                if not dx and need[0] and need[1] and all(linear_supported(m, k, dt) for m in ms):
                    # the two data gradients the one-pass kernel does not cover (a first layer reads K = 256): one launch
                    for st in sts:
                        if st.wt_of.key != st.w_key:
                            raise RuntimeError("the projection weights changed between this forward and its backward "
                                               "(optimizer step in between?): run backward before stepping")
                    gxa, gxb = linear_fwd_pair_launch(gya, sts[0].wt_of.wt, gyb, sts[1].wt_of.wt)
                    pre = [(gxa,) + tuple(pre[0][1:]), (gxb,) + tuple(pre[1][1:])]
        ra = _linear_backward(sts[0], xa, gya, need[0], na, pre[0])
        rb = _linear_backward(sts[1], xb, gyb, need[1], nb, pre[1])
        return (ra[0], rb[0], None, None) + ra[2:] + rb[2:]


def linear_pair(xa: Tensor, wa, ba, xb: Tensor, wb, bb) -> Tuple[Tensor, Tensor]:
    """``(linear(xa, wa, ba), linear(xb, wb, bb))`` -- as ONE launch when both are 2-D activations of the same dtype and
    width on the MFMA kernels (a hetero layer's transcript and boundary projections, ``lin_last`` of both node types)."""
    tup = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v,)
    wa, ba, wb, bb = tup(wa), tup(ba), tup(wb), tup(bb)
    ma, mb = sum(int(w.shape[0]) for w in wa), sum(int(w.shape[0]) for w in wb)
    ok = (ops.LINEAR_PAIR and xa.dim() == 2 and xb.dim() == 2 and xa.is_cuda and xb.is_cuda and xa.dtype == xb.dtype
          and xa.dtype in (torch.bfloat16, torch.float16)
          and xa.shape[1] == xb.shape[1] and xa.shape[0] > 0 and xb.shape[0] > 0
          and len(ba) == len(wa) and len(bb) == len(wb)
          and linear_supported(xa.shape[1], ma, xa.dtype) and linear_supported(xb.shape[1], mb, xb.dtype))
    if not ok:
        return linear(xa, wa, ba), linear(xb, wb, bb)
    if xa.shape[0] > 1 and xa.stride(1) != 1:
        xa = xa.contiguous()
    if xb.shape[0] > 1 and xb.stride(1) != 1:
        xb = xb.contiguous()
    return _LinearPair.apply(xa, xb, len(wa), len(wb), *wa, *ba, *wb, *bb)


def linear(x: Tensor, weight, bias) -> Tensor:
    """``F.linear`` for node-feature matrices.  ``weight`` / ``bias`` may be sequences of tensors: the maps are
    stacked by rows into one GEMM (``[lin_l | lin_r | ...](x)``).  Activations with a covered (K, M) use the MFMA
    kernels -- bf16 / f16 on v_mfma_f32_32x32x16, fp32 (the reference's arithmetic width) on the exact-fp32
    v_mfma_f32_32x32x2_f32 -- and only uncovered shapes fall to the vendor GEMM."""
    weights = tuple(weight) if isinstance(weight, (list, tuple)) else (weight,)
    biases = tuple(bias) if isinstance(bias, (list, tuple)) else (bias,)
    if len(biases) != len(weights):
        raise ValueError("linear: one bias (or None) per weight")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    m_out = sum(int(w.shape[0]) for w in weights)
    if x2.is_cuda and linear_supported(x2.shape[1], m_out, x2.dtype) and x2.shape[0] > 0:
        if x2.shape[0] > 1 and x2.stride(1) != 1:
            x2 = x2.contiguous()
        y = _Linear.apply(x2, len(weights), *weights, *biases)
    else:
        _lib.require_cuda(x2)
        if x2.shape[0] > 0:
            _vendor_gemm("projection y = x W^T", x2.shape[1], m_out, x2.dtype)
        w = weights[0] if len(weights) == 1 else torch.cat(weights, 0)
        b = None
        if any(bb is not None for bb in biases):
            b = torch.cat([bb if bb is not None else ww.new_zeros(ww.shape[0]) for ww, bb in zip(weights, biases)], 0)
        y = torch.nn.functional.linear(x2, w.to(x2.dtype), None if b is None else b.to(x2.dtype))
    return y.reshape(*lead, m_out)
