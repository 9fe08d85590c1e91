from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE
from ..graph import EdgeCSR
from .. import ops                # route switches: read as ops.NAME when called, never bound here
from ._common import _defer_keep, _f32_vec, _grad_rows, _rows, _seq, _vendor_gemm, _wgrad_ws_bytes
from .packs import _pack_for, f32_split_planes


# --------------------------------------------------------------------------
# Tall-skinny projection GEMM (MFMA) with autograd
# --------------------------------------------------------------------------
_ACT_KIND = {"gelu": 1, "silu": 2}        # the activation codes of the fp32 gate / act kernels


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
        rc = _lib.load().segger_linear_fwd_f32_gate(xp, ldx, wq.data_ptr(), int(split), gp, ldg, _ACT_KIND[kind],
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
                                                   _ACT_KIND[kind], n, k, m, _lib.stream_ptr(x.device))
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


def _wgrad_outputs(n: int, m: int, k: int, want_bias: bool, device):
    """-> (dW [M, K], db [M] | None, workspace, its bytes): what a weight-gradient launch writes, fp32; kept alive for a
    deferred final sum (``ops.deferred_reductions``)."""
    gw = torch.empty((m, k), dtype=torch.float32, device=device)
    gb = torch.empty(m, dtype=torch.float32, device=device) if want_bias else None
    ws_bytes = _wgrad_ws_bytes(n, m, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    _defer_keep(ws, gw, gb)
    return gw, gb, ws, ws_bytes


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
    gw, gb, ws, ws_bytes = _wgrad_outputs(n, m, k, want_bias, x.device)
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
    gw, gb, ws, ws_bytes = _wgrad_outputs(n, m, k, want_bias, x.device)
    with _lib.on_device(x.device):
        rc = lib.segger_linear_wgrad_dx(gp, ldg, xp, ldx, wt.data_ptr(), n, m, k, DTYPE_CODE[x.dtype], gw.data_ptr(),
                                        _lib.ptr(gb), gx.data_ptr(), k, qp, ldq, ws.data_ptr(), ws_bytes,
                                        _lib.stream_ptr(x.device))
    _lib.check(rc, "segger_linear_wgrad_dx")
    return gx, gw, gb


def _linear_args(x: Tensor, w: Tensor, bias: Optional[Tensor]):
    """-> (``segger_linear_args`` of ``y = x @ w.T + bias``, the new y): one side of a paired forward launch."""
    n, k = x.shape
    m = int(w.shape[0])
    if w.dtype != x.dtype or not w.is_contiguous() or w.shape[1] != k:
        raise ValueError("linear pair: weights must be contiguous [M, K] in the activation dtype")
    y = torch.empty((n, m), dtype=x.dtype, device=x.device)
    a = _lib.LinearArgs()
    a.x, a.ldx = _rows(x, k, "x")
    a.w, a.bias = w.data_ptr(), _lib.ptr(_f32_vec(bias, m, "bias"))
    a.y, a.ldy, a.n_rows, a.m_out = y.data_ptr(), m, n, m
    return a, y


def linear_fwd_pair_launch(xa: Tensor, wa: Tensor, xb: Tensor, wb: Tensor) -> Tuple[Tensor, Tensor]:
    """``(xa @ wa.T, xb @ wb.T)`` for 16-bit activations whose widths may differ (``segger_linear_fwd_pair_k``: one launch
    for widths (384, 128) or equal widths -- a first layer's two data gradients -- two otherwise)."""
    _lib.require_cuda(xa, wa, xb, wb)
    (aa, ya), (ab, yb) = _linear_args(xa, wa, None), _linear_args(xb, wb, None)
    with _lib.on_device(xa.device):
        rc = _lib.load().segger_linear_fwd_pair_k(C.byref(aa), int(xa.shape[1]), C.byref(ab), int(xb.shape[1]),
                                                  DTYPE_CODE[xa.dtype], _lib.stream_ptr(xa.device))
    _lib.check(rc, "segger_linear_fwd_pair_k")
    return ya, yb


def linear_wgrad_pair_launch(sides, dx: bool):
    """``sides`` = two (gy [n, M], x [n, K], wt [K, M] | None, want_bias) of one K and dtype -> [(gx | None, gw, gb | None)] * 2 from
    ONE launch (``segger_linear_wgrad_pair``; ``dx``: the one-pass form with the data gradients, else dW / db only)."""
    lib = _lib.load()
    dev, dt = sides[0][0].device, sides[0][1].dtype
    args, outs = [], []
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
        gw, gb, ws, ws_bytes = _wgrad_outputs(n, m, k, want_bias, dev)
        a.grad_w, a.grad_b, a.workspace, a.workspace_bytes = gw.data_ptr(), _lib.ptr(gb), ws.data_ptr(), ws_bytes
        args.append(a)
        outs.append((gx, gw, gb, ws))
    with _lib.on_device(dev):
        rc = lib.segger_linear_wgrad_pair(C.byref(args[0]), C.byref(args[1]), int(sides[0][1].shape[1]), DTYPE_CODE[dt],
                                          _lib.stream_ptr(dev))
    _lib.check(rc, "segger_linear_wgrad_pair")
    return [o[:3] for o in outs]


def _weight_grad_gemm(gy: Tensor, x: Tensor) -> Tensor:
    """dW[M, K] = gy^T x as a plain library GEMM: shapes the MFMA weight-gradient kernel does not cover
    (``linear_wgrad_supported``).  fp32 result."""
    _vendor_gemm("weight gradient dW = dY^T X", x.shape[1], gy.shape[1], x.dtype)
    return (gy.t() @ x).float()


class BackwardPlan(NamedTuple):
    """The route of each output of one projection backward (:func:`backward_plan`)."""
    dx: Optional[str] = None    # None | "one_pass" (segger_linear_wgrad_dx) | "f32_gate" | "f32_split" | "mfma" | "vendor"
    dw: Optional[str] = None    # dW / db: None | "one_pass" (they come with dX) | "mfma" | "vendor" (GEMM + colsum)
    gate: bool = False          # gelu'(pre) is applied inside the data-gradient kernel; else aten.gelu_backward, by the caller
    want_w: bool = False
    want_b: bool = False


def backward_plan(m: int, k: int, n: int, dt, need_x: bool, want_w: bool, want_b: bool, pre: bool = False,
                  pre_grad: bool = False, aligned: bool = True, site: str = "generic", have_dw: bool = False) -> BackwardPlan:
    """The kernels that serve dX [n, K], dW [M, K] and db of ``y = x W^T + b`` at dtype ``dt``, from shapes, needs and the
    ``ops`` switches alone (no tensor, no launch).  ``pre``: x = gelu(pre) and the data gradient goes to ``pre``
    (``pre_grad``: it requires one); ``aligned``: dY's rows start on 16 bytes (the fp32 split reads them as such).
    ``site``: "generic" (:class:`_Linear`, a side of :class:`_LinearPair`) has a vendor route for uncovered shapes; the
    first layer's nodes are entered with covered ones only -- "first" (``_EmbedLinear``) has the fp32 routes, "row_bias"
    (``_RowBiasLinear``) does not.  ``have_dw``: a paired launch already left dW / db (a one-pass dX still returns them)."""
    generic = site == "generic"
    f32 = dt == torch.float32 and site != "row_bias"
    dx = dw = None
    gate = False
    if ops.FUSED_WGRAD_DX and need_x and (want_w or want_b) and n > 0 and linear_wgrad_dx_supported(m, k, dt):
        dx = dw = "one_pass"                                 # dY read ONCE for dX, dW and db
        gate = bool(pre and ops.FUSED_GELU_GATE and linear_wgrad_dx_gate_supported(m, k, dt))
    else:
        if not need_x:
            pass
        elif f32 and pre and pre_grad and aligned and ops.F32_GATE_EPILOGUE and linear_f32_gate_supported(m, k):
            dx, gate = "f32_gate", True                      # dX * gelu'(pre) in one kernel
        elif ops.F32_SPLIT and f32 and aligned and linear_f32_split_supported(m, k):
            dx = "f32_split"
        else:
            dx = "mfma" if not generic or linear_supported(m, k, dt) else "vendor"
        if have_dw:
            pass
        elif not generic:
            dw = "mfma" if want_w else None
        elif want_w or want_b:
            dw = "mfma" if n > 0 and linear_wgrad_supported(m, k, dt) else "vendor"
    return BackwardPlan(dx, dw, gate, want_w, want_b)


def backward_pair_plan(k: int, ms, ns, dt, need_xs, wants, have_grads: bool = True) -> Optional[str]:
    """Two projection backwards of one K in shared launches: None (each side by its own :func:`backward_plan`) |
    "one_pass" (one ``segger_linear_wgrad_pair`` launch with both data gradients) | "wgrad" (one without them) |
    "wgrad+dx" (one without, and one ``segger_linear_fwd_pair_k`` launch for the two data gradients the one-pass kernel
    does not cover: a first layer reads K = 256).  ``ms`` / ``ns`` / ``need_xs`` / ``wants``: per side M, row count, "the
    input needs a gradient", "a parameter does"."""
    if not (ops.WGRAD_PAIR and all(wants) and have_grads and dt in (torch.bfloat16, torch.float16) and all(n > 0 for n in ns)):
        return None
    if ops.FUSED_WGRAD_DX and all(need_xs) and all(linear_wgrad_dx_supported(m, k, dt) for m in ms):
        return "one_pass"
    if not all(linear_wgrad_supported(m, k, dt) for m in ms):
        return None
    return "wgrad+dx" if all(need_xs) and all(linear_supported(m, k, dt) for m in ms) else "wgrad"


def _run_backward(plan: BackwardPlan, gy: Tensor, x: Tensor, weights, pre: Optional[Tensor] = None) -> tuple:
    """-> (gx, gw, gb) of ``plan``.  ``weights(form)``: "wt" = W^T [K, M] (dX = dY @ W), "planes_t" = its bf16x3 planes,
    "w" = W -- each asked for only on the route that reads it: at fp32 storage the split kernels take the transposed PLANES,
    and building W^T as well was one stray transposing launch per projection and step."""
    gx = gw = gb = None
    if plan.dx == "one_pass":
        gx, gw, gb = linear_wgrad_dx_launch(gy, x, weights("wt"), want_bias=plan.want_b, gate=pre if plan.gate else None)
    elif plan.dx == "f32_gate":
        gx = linear_f32_gate_launch(gy, weights("wt"), pre, "gelu")
    elif plan.dx == "f32_split":
        gx = linear_f32_split_launch(gy, weights("planes_t"), None)
    elif plan.dx == "mfma":
        gx = linear_fwd_launch(gy, weights("wt"), None)
    elif plan.dx == "vendor":
        _vendor_gemm("data gradient dX = dY W", gy.shape[1], x.shape[1], x.dtype)
        gx = gy @ weights("w")
    if plan.dw == "mfma":
        gw, gb = linear_wgrad_launch(gy, x, want_bias=plan.want_b)       # dY and X read once for both
    elif plan.dw == "vendor":
        gw = _weight_grad_gemm(gy, x) if plan.want_w else None
        gb = colsum(gy) if plan.want_b else None
    return gx, gw, gb


class _Saved:
    """What a projection's forward leaves for its backward beside the input: the pack, the generation of the weights it
    read (the pack is refreshed IN PLACE after an optimizer step; a backward that runs later than that -- not the case in
    forward -> backward -> step training -- would see the new weights), the stacked row counts and the bias flags."""
    __slots__ = ("pack", "key", "rows", "has_bias")

    def __init__(self, pk):
        self.pack, self.key, self.rows, self.has_bias = pk, pk.key, pk.rows, pk.has_bias

    def weights(self, form: str) -> Tensor:
        pk = self.pack
        if pk.key != self.key:
            raise RuntimeError("the projection weights changed between this forward and its backward "
                               "(optimizer step in between?): run backward before stepping")
        return pk.wt if form == "wt" else pk.planes(transposed=True) if form == "planes_t" else pk.w

    def wants(self, need_params) -> Tuple[bool, bool]:
        """(a weight, a bias) wants a gradient; ``need_params`` = needs_input_grad of the weights, then of the biases."""
        n_w = len(self.rows)
        return any(need_params[:n_w]), any(h and g for h, g in zip(self.has_bias, need_params[n_w:]))


def _projection_backward(st: _Saved, x, gy, need_x: bool, need_params, done=(None, None, None)) -> tuple:
    """-> (gx, (*grads_w, *grads_b)) of one projection: plans and runs what ``done`` = (gx, gw, gb) of a paired launch left
    open; each parameter's gradient is a row window of the stacked result."""
    gx, gw, gb = done
    gy = _grad_rows(gy, x.dtype)
    m, k = st.pack.w.shape
    plan = backward_plan(m, k, x.shape[0], x.dtype, need_x and gx is None, *st.wants(need_params),
                         aligned=gy.stride(0) % 4 == 0, have_dw=gw is not None)
    out = _run_backward(plan, gy, x, st.weights)
    if plan.dx:
        gx = out[0]
    if plan.dw:
        gw, gb = out[1:]
    n_w, grads_w, grads_b, r0 = len(st.rows), [], [], 0
    for i, r in enumerate(st.rows):
        grads_w.append(gw[r0:r0 + r] if (gw is not None and need_params[i]) else None)
        grads_b.append(gb[r0:r0 + r] if (gb is not None and st.has_bias[i] and need_params[n_w + i]) else None)
        r0 += r
    return gx, tuple(grads_w) + tuple(grads_b)


class _Linear(torch.autograd.Function):
    """x [n, K] (bf16/f16); ``n_w`` fp32 master weights [M_i, K] stacked by rows, ``n_w`` fp32 biases (or None)
    -> [n, sum M_i].  Forward, the data gradient and the weight / bias gradients run on the hand-written MFMA kernels
    (csrc/linear.hip, csrc/linear_wgrad.hip); each parameter's gradient is a row window of the one fused result."""

    @staticmethod
    def forward(ctx, x, n_w, *params):
        pk = _pack_for(params[:n_w], params[n_w:]).get(x.dtype, x.device)
        if ops.F32_SPLIT and x.dtype == torch.float32 and linear_f32_split_supported(x.shape[1], pk.w.shape[0]):
            y = linear_f32_split_launch(x, pk.planes(), pk.b)
        else:
            y = linear_fwd_launch(x, pk.w, pk.b)
        ctx.save_for_backward(x)
        ctx.st = _Saved(pk)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gx, grads = _projection_backward(ctx.st, x, gy, ctx.needs_input_grad[0], ctx.needs_input_grad[2:])
        return (gx, None) + grads


class _LinearPair(torch.autograd.Function):
    """Two projections with the same K as one launch (``segger_linear_fwd_pair``): (xa, xb, n_wa, n_wb, *weights_a,
    *biases_a, *weights_b, *biases_b) -> (ya, yb).  Backward: what :func:`backward_pair_plan` shares, then each side's own."""

    @staticmethod
    def forward(ctx, xa, xb, n_wa, n_wb, *params):
        sides, args, outs = [], [], []
        for x, n_w, pp in ((xa, n_wa, params[:2 * n_wa]), (xb, n_wb, params[2 * n_wa:])):
            pk = _pack_for(pp[:n_w], pp[n_w:]).get(x.dtype, x.device)
            sides.append(_Saved(pk))
            a, y = _linear_args(x, pk.w, pk.b)
            args.append(a)
            outs.append(y)
        with _lib.on_device(xa.device):
            rc = _lib.load().segger_linear_fwd_pair(C.byref(args[0]), C.byref(args[1]), int(xa.shape[1]), DTYPE_CODE[xa.dtype],
                                                    _lib.stream_ptr(xa.device))
        _lib.check(rc, "segger_linear_fwd_pair")
        ctx.save_for_backward(xa, xb)
        ctx.sides = sides
        return outs[0], outs[1]

    @staticmethod
    def backward(ctx, *gys):
        xs, sts, need = ctx.saved_tensors, ctx.sides, ctx.needs_input_grad
        split = 4 + 2 * len(sts[0].rows)
        needs = (need[4:split], need[split:])
        wants = [st.wants(nn) for st, nn in zip(sts, needs)]
        dt = xs[0].dtype
        pair = backward_pair_plan(int(xs[0].shape[1]), [int(st.pack.w.shape[0]) for st in sts], [x.shape[0] for x in xs], dt,
                                  need[:2], [w or b for w, b in wants], all(g is not None for g in gys))
        done = [(None, None, None)] * 2
        if pair:
            gys = [_grad_rows(g, dt) for g in gys]
            dx = pair == "one_pass"
            done = linear_wgrad_pair_launch([(g, x, st.weights("wt") if dx else None, wb[1])
                                             for g, x, st, wb in zip(gys, xs, sts, wants)], dx)
            if pair == "wgrad+dx":
                gxs = linear_fwd_pair_launch(gys[0], sts[0].weights("wt"), gys[1], sts[1].weights("wt"))
                done = [(gx,) + d[1:] for gx, d in zip(gxs, done)]
        (gxa, ga), (gxb, gb) = [_projection_backward(st, x, g, nx, nn, d)
                                for st, x, g, nx, nn, d in zip(sts, xs, gys, need, needs, done)]
        return (gxa, gxb, None, None) + ga + gb


def linear_pair(xa: Tensor, wa, ba, xb: Tensor, wb, bb) -> Tuple[Tensor, Tensor]:
    """``(linear(xa, wa, ba), linear(xb, wb, bb))`` -- as ONE launch when both are 2-D activations of the same dtype and
    width on the MFMA kernels (a hetero layer's transcript and boundary projections, ``lin_last`` of both node types)."""
    wa, ba, wb, bb = _seq(wa), _seq(ba), _seq(wb), _seq(bb)
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
    weights, biases = _seq(weight), _seq(bias)
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
