from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE
from .. import ops                # route switches: read as ops.NAME when called, never bound here
from ._common import _defer_keep, _grad_rows, _rows
from .packs import _pack_for
from .linear import (linear_f32_act_launch, linear_f32_gate_launch, linear_f32_gate_supported, linear_fwd_launch,
                     linear_supported, linear_wgrad_launch, linear_wgrad_supported)


# --------------------------------------------------------------------------
# Positional embedder: per-graph min / max
# --------------------------------------------------------------------------
@torch.no_grad()
def segment_minmax(pos: Tensor, batch: Optional[Tensor], num_graphs: int, keep_empty: bool = False,
                   out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
    """-> (mins[num_graphs, 2], maxs[num_graphs, 2]) fp32 of ``pos`` grouped by ``batch``.  ``keep_empty``: graphs
    without nodes keep (+inf, -inf) instead of the reference's (0, 0) -- for consumers that only look up the graphs of
    existing nodes (one launch less).  ``out``: buffers the caller has ALREADY filled with +inf / -inf (a captured step
    does that in its staging launch): no initialising launch either."""
    _lib.require_cuda(pos)
    lib = _lib.load()
    dev = pos.device
    pos = pos.to(torch.float32).contiguous()
    if pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError("segment_minmax: pos must be [n, 2]")
    if batch is not None:
        batch = batch.to(device=dev, dtype=torch.int64).contiguous()
        if batch.numel() != pos.shape[0]:
            raise ValueError("segment_minmax: batch / pos length mismatch")
    flags = 2 if keep_empty else 0
    if out is not None:
        mins, maxs = out
        for t in (mins, maxs):
            if t.dtype != torch.float32 or t.numel() < 2 * num_graphs or not t.is_contiguous() or t.device != dev:
                raise ValueError("segment_minmax: out must be two contiguous float32 [num_graphs, 2] tensors on pos's device")
        flags |= 1
    else:
        mins = torch.empty((num_graphs, 2), dtype=torch.float32, device=dev)
        maxs = torch.empty((num_graphs, 2), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = lib.segger_segment_minmax_ex(pos.data_ptr(), _lib.ptr(batch), int(pos.shape[0]), int(num_graphs),
                                          mins.data_ptr(), maxs.data_ptr(), flags, _lib.stream_ptr(dev))
    _lib.check(rc, "segger_segment_minmax_ex")
    return mins, maxs


class _MlpSiluF32(torch.autograd.Function):
    """``linear(silu(linear(x, w0, b0)), w2, b2)`` at fp32 storage as ONE autograd node (the positional embedder's shared MLP,
    ist_encoder.py:43-49, on its un-fused route): the backward's SiLU derivative rides in the epilogue of the data-gradient
    GEMM (``segger_linear_fwd_f32_gate``) instead of torch's silu_backward pass.  ``x`` receives no gradient (the sinusoid
    features are constants)."""

    @staticmethod
    def forward(ctx, x, w0, b0, w2, b2, gelu_out=False):
        w0d, w2d = w0.detach().contiguous(), w2.detach().contiguous()
        z1, h1 = linear_f32_act_launch(x, w0d, b0, "silu")           # pre-activation and SiLU from one kernel
        ctx.save_for_backward(x, z1, h1, w2)
        if gelu_out:                                                  # (y, gelu(y)): the second a constant for autograd
            y, gy_ = linear_f32_act_launch(h1, w2d, b2, "gelu")
            ctx.mark_non_differentiable(gy_)
            return y, gy_
        return linear_fwd_launch(h1, w2d, b2.detach())

    @staticmethod
    def backward(ctx, gy, _unused=None):
        x, z1, h1, w2 = ctx.saved_tensors
        gy = gy.contiguous()
        gw2, gb2 = linear_wgrad_launch(gy, h1)
        dz1 = linear_f32_gate_launch(gy, w2.detach().t().contiguous(), z1, "silu")
        gw0, gb0 = linear_wgrad_launch(dz1, x)
        return None, gw0, gb0, gw2, gb2, None


def mlp_silu_f32_supported(x: Tensor, w0: Tensor, w2: Tensor) -> bool:
    d_in, d_h, d_out = int(w0.shape[1]), int(w0.shape[0]), int(w2.shape[0])
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] > 0 and not x.requires_grad
            and linear_supported(d_in, d_h, torch.float32) and linear_supported(d_h, d_out, torch.float32)
            and linear_wgrad_supported(d_h, d_in, torch.float32) and linear_wgrad_supported(d_out, d_h, torch.float32)
            and linear_f32_gate_supported(d_out, d_h) and d_in in (64, 128, 256) and d_h in (64, 128, 256)
            and d_h % 64 == 0 and d_out % 64 == 0)


def mlp_silu_f32(x: Tensor, w0, b0, w2, b2, gelu_out: bool = False):
    """``linear(silu(linear(x)))``; ``gelu_out``: ``(y, gelu(y))`` with the GELU a constant for autograd (the gradient is
    expected for ``y``: the consumer applies gelu')."""
    return _MlpSiluF32.apply(x, w0, b0, w2, b2, gelu_out)


def pos_poly_mlp_f32_supported(pos: Tensor, w0: Tensor, w2: Tensor) -> bool:
    dim, fd = int(w0.shape[0]), int(w0.shape[1])
    return (ops.POS_POLY_F32 and pos.is_cuda and pos.dim() == 2 and pos.shape[1] == 2 and pos.shape[0] > 0 and not pos.requires_grad
            and w0.dtype == torch.float32 and w2.dtype == torch.float32 and tuple(w2.shape) == (dim, dim)
            and bool(_lib.load().segger_posenc_poly_supported(fd, dim))
            and linear_supported(dim, dim, torch.float32) and linear_wgrad_supported(dim, dim, torch.float32)
            and linear_f32_gate_supported(dim, dim) and dim % 64 == 0)


class _PosPolyMlpF32(torch.autograd.Function):
    """``Linear -> SiLU -> Linear`` of ``Positional2dEmbedder`` on the sinusoid of the normalised coordinates at fp32 storage,
    from the POSITIONS (ist_encoder.py:57-79 in one autograd node): the first layer by ``segger_posenc_poly_fwd`` (13
    coefficients per channel, refreshed from W0 / b0 by ``segger_posenc_poly_coef``), its weight gradient by
    ``segger_posenc_poly_wgrad`` (13 moments per channel); the 64-wide second layer on the exact-fp32 kernels as before."""

    @staticmethod
    def forward(ctx, pos, batch, mins, maxs, eps, max_period, w0, b0, w2, b2, gelu_out=False):
        lib = _lib.load()
        dev = pos.device
        pos = pos.detach().to(torch.float32).contiguous()
        if batch is not None:
            batch = batch.to(device=dev, dtype=torch.int64).contiguous()
        n, dim, fd = int(pos.shape[0]), int(w0.shape[0]), int(w0.shape[1])
        w0d, w2d, b0d = w0.detach().contiguous(), w2.detach().contiguous(), b0.detach().float().contiguous()
        coef = torch.empty((dim, 16), dtype=torch.float32, device=dev)
        z1 = torch.empty((2 * n, dim), dtype=torch.float32, device=dev)
        h1 = torch.empty_like(z1)
        pn = torch.empty(2 * n, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            st = _lib.stream_ptr(dev)
            rc = lib.segger_posenc_poly_coef(w0d.data_ptr(), b0d.data_ptr(), fd, dim, float(max_period), coef.data_ptr(), st)
            _lib.check(rc, "segger_posenc_poly_coef")
            rc = lib.segger_posenc_poly_fwd(pos.data_ptr(), _lib.ptr(batch), mins.data_ptr(), maxs.data_ptr(), n, float(eps),
                                            coef.data_ptr(), dim, z1.data_ptr(), h1.data_ptr(), pn.data_ptr(), st)
            _lib.check(rc, "segger_posenc_poly_fwd")
        ctx.save_for_backward(pn, z1, h1, w2)
        ctx.cfg = (fd, dim, float(max_period))
        if gelu_out:                                                  # (y, gelu(y)): the second a constant for autograd
            y, gy_ = linear_f32_act_launch(h1, w2d, b2, "gelu")
            ctx.mark_non_differentiable(gy_)
            return y, gy_
        return linear_fwd_launch(h1, w2d, b2.detach())

    @staticmethod
    def backward(ctx, gy, _unused=None):
        pn, z1, h1, w2 = ctx.saved_tensors
        fd, dim, max_period = ctx.cfg
        lib = _lib.load()
        dev = gy.device
        gy = gy.contiguous()
        gw2, gb2 = linear_wgrad_launch(gy, h1)
        dz1 = linear_f32_gate_launch(gy, w2.detach().t().contiguous(), z1, "silu")
        gw0 = torch.empty((dim, fd), dtype=torch.float32, device=dev)
        gb0 = torch.empty(dim, dtype=torch.float32, device=dev)
        rows = int(dz1.shape[0])
        ws_bytes = int(lib.segger_posenc_poly_wgrad_workspace_bytes(rows, dim))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.segger_posenc_poly_wgrad(dz1.data_ptr(), dim, pn.data_ptr(), rows, fd, dim, max_period, gw0.data_ptr(),
                                              gb0.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
        _lib.check(rc, "segger_posenc_poly_wgrad")
        _defer_keep(ws)
        return None, None, None, None, None, None, gw0, gb0, gw2, gb2, None


def pos_poly_mlp_f32(pos: Tensor, batch: Optional[Tensor], mins: Tensor, maxs: Tensor, w0, b0, w2, b2, *, eps: float = 1e-8,
                     max_period: float = 10000.0, gelu_out: bool = False):
    """[n, 2] positions -> the embedder's MLP output as coordinate rows [2n, dim] (``gelu_out``: ``(y, gelu(y))``, the GELU a
    constant for autograd as in :func:`mlp_silu_f32`)."""
    return _PosPolyMlpF32.apply(pos, batch, mins, maxs, eps, max_period, w0, b0, w2, b2, gelu_out)


@torch.no_grad()
def posfreq(pos: Tensor, batch: Optional[Tensor], mins: Tensor, maxs: Tensor, freq_dim: int, dtype: torch.dtype,
            eps: float = 1e-8, max_period: float = 10000.0) -> Tensor:
    """[n, 2] positions -> [n, 2, freq_dim] sinusoid of the per-graph normalised coordinates."""
    _lib.require_cuda(pos)
    lib = _lib.load()
    dev = pos.device
    pos = pos.to(torch.float32).contiguous()
    n = int(pos.shape[0])
    if batch is not None:
        batch = batch.to(device=dev, dtype=torch.int64).contiguous()
    out = torch.empty((n, 2, freq_dim), dtype=dtype, device=dev)
    with _lib.on_device(dev):
        rc = lib.segger_posfreq(pos.data_ptr(), _lib.ptr(batch), mins.data_ptr(), maxs.data_ptr(), n, freq_dim,
                                eps, max_period, out.data_ptr(), DTYPE_CODE[dtype], _lib.stream_ptr(dev))
    _lib.check(rc, "segger_posfreq")
    return out


def posmlp_supported(freq_dim: int, dim: int, dtype: torch.dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and bool(
        _lib.load().segger_posmlp_supported(int(freq_dim), int(dim), DTYPE_CODE[dtype]))


class _PosMlp(torch.autograd.Function):
    """Positional2dEmbedder in one kernel (``segger_posmlp_fwd``): [n, 2] positions -> [n, 128].  With gradients the
    kernel also stores the first layer's pre-activation and the normalised coordinates (4 bytes per row), and the
    backward is assembled from the projection kernels: dW2 / db2 by ``segger_linear_wgrad``, dh1 by
    ``segger_linear_fwd``, dW0 / db0 by ``segger_posmlp_wgrad`` (the sinusoid features regenerated in the kernel)."""

    @staticmethod
    def forward(ctx, pos, batch, mins, maxs, eps, max_period, dtype, train, gelu, w0, b0, w2, b2):
        _lib.require_cuda(pos, w0)
        lib = _lib.load()
        dev = pos.device
        pos = pos.to(torch.float32).contiguous()
        n = int(pos.shape[0])
        if batch is not None:
            batch = batch.to(device=dev, dtype=torch.int64).contiguous()
        pk0 = _pack_for((w0,), (b0,)).get(dtype, dev)
        pk2 = _pack_for((w2,), (b2,)).get(dtype, dev)
        pe = torch.empty((n, 2 * w2.shape[0]), dtype=dtype, device=dev)
        z1 = torch.empty((2 * n, w0.shape[0]), dtype=dtype, device=dev) if train else None
        pn = torch.empty(2 * n, dtype=torch.float32, device=dev) if train else None
        pre = torch.empty_like(pe) if (train and gelu) else None
        h1 = torch.empty_like(z1) if (train and not ops.FUSED_POSMLP_BWD) else None    # (the one-pass backward recomputes it)
        ctx.set_materialize_grads(False)
        with _lib.on_device(dev):
            rc = lib.segger_posmlp_fwd(pos.data_ptr(), _lib.ptr(batch), mins.data_ptr(), maxs.data_ptr(), n, float(eps),
                                       float(max_period), pk0.w.data_ptr(), pk0.b.data_ptr(), pk2.w.data_ptr(),
                                       pk2.b.data_ptr(), pe.data_ptr(), _lib.ptr(z1), _lib.ptr(pn), _lib.ptr(h1), _lib.ptr(pre),
                                       int(bool(gelu)),
                                       DTYPE_CODE[dtype],
                                       _lib.stream_ptr(dev))
        _lib.check(rc, "segger_posmlp_fwd")
        ctx.by_pre = bool(train and int(gelu) == 2)
        if train:
            ctx.save_for_backward(z1, pn, pre, h1)
            ctx.pk2, ctx.key2, ctx.max_period = pk2, pk2.key, float(max_period)
        if ctx.by_pre:
            # the consumer applies gelu' itself (in the epilogue of its data-gradient kernel) and returns d loss / d pre:
            # `pe` = gelu(pre) leaves as a constant, `pre` as the differentiable output
            ctx.mark_non_differentiable(pe)
            return pe, pre
        return pe

    @staticmethod
    def backward(ctx, gpe, gpre=None):
        z1, pn, pre, h1 = ctx.saved_tensors
        dt = z1.dtype
        d = z1.shape[1]
        if ctx.by_pre:
            gpe = gpre
        if gpe is None:                                      # (nothing downstream used the output)
            return (None,) * 13
        if pre is not None and not ctx.by_pre:               # the output was gelu(embedder output)
            gpe = torch.ops.aten.gelu_backward(gpe.to(dt), pre)
        g = _grad_rows(gpe.reshape(-1, d), dt)
        if ctx.pk2.key != ctx.key2:
            raise RuntimeError("the positional MLP's weights changed between this forward and its backward")
        need = ctx.needs_input_grad
        if h1 is None:                                       # one pass over g: all four parameter gradients
            lib = _lib.load()
            dev = z1.device
            gw0 = torch.empty((d, 4 * d), dtype=torch.float32, device=dev)
            gb0 = torch.empty(d, dtype=torch.float32, device=dev)
            gw2 = torch.empty((d, d), dtype=torch.float32, device=dev)
            gb2 = torch.empty(d, dtype=torch.float32, device=dev)
            n_rows = int(g.shape[0])
            ws_bytes = lib.segger_posmlp_bwd_workspace_bytes(n_rows)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            gp, ldg = _rows(g, d, "g")
            with _lib.on_device(dev):
                rc = lib.segger_posmlp_bwd(gp, ldg, z1.data_ptr(), pn.data_ptr(), ctx.pk2.wt.data_ptr(), n_rows,
                                           ctx.max_period, DTYPE_CODE[dt], gw0.data_ptr(), gb0.data_ptr(), gw2.data_ptr(),
                                           gb2.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
            _lib.check(rc, "segger_posmlp_bwd")
            _defer_keep(ws, gw0, gb0, gw2, gb2)
            return (None, None, None, None, None, None, None, None, None, gw0 if need[9] else None,
                    gb0 if need[10] else None, gw2 if need[11] else None, gb2 if need[12] else None)
        gw2, gb2 = linear_wgrad_launch(g, h1)
        # dz1 = (g @ W2) * silu'(z1): the SiLU derivative is applied in the GEMM's epilogue
        lib0 = _lib.load()
        dz1 = torch.empty_like(z1)
        wt = ctx.pk2.wt
        gp, ldg = _rows(g, d, "g")
        with _lib.on_device(z1.device):
            rc = lib0.segger_linear_fwd_silu_grad(gp, ldg, wt.data_ptr(), z1.data_ptr(), d, dz1.data_ptr(), d,
                                                  int(g.shape[0]), d, d, DTYPE_CODE[dt], _lib.stream_ptr(z1.device))
        _lib.check(rc, "segger_linear_fwd_silu_grad")
        # dW0 = dz1^T F with the sinusoid features F regenerated from one float per row inside the kernel
        lib = _lib.load()
        dev = z1.device
        gw0 = torch.empty((d, 4 * d), dtype=torch.float32, device=dev)
        gb0 = torch.empty(d, dtype=torch.float32, device=dev)
        ws_bytes = lib.segger_linear_wgrad_workspace_bytes(int(dz1.shape[0]), d, 4 * d)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        dp, ldd = _rows(dz1, d, "dz1")
        with _lib.on_device(dev):
            rc = lib.segger_posmlp_wgrad(dp, ldd, pn.data_ptr(), int(dz1.shape[0]), ctx.max_period, DTYPE_CODE[dt],
                                         gw0.data_ptr(), gb0.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
        _lib.check(rc, "segger_posmlp_wgrad")
        _defer_keep(ws, gw0, gb0)
        return (None, None, None, None, None, None, None, None, None, gw0 if need[9] else None,
                gb0 if need[10] else None, gw2 if need[11] else None, gb2 if need[12] else None)


def _posmlp_fwd_launch(pos, batch, mins, maxs, eps, max_period, dtype, train, gelu, pk0, pk2, d):
    """One ``segger_posmlp_fwd`` launch -> (pe, z1, pn, pre): what ``_PosMlp`` / ``_PosMlpPair`` keep of a row set (the
    one-pass backward recomputes h1)."""
    dev = pos.device
    pos = pos.to(torch.float32).contiguous()
    n = int(pos.shape[0])
    if batch is not None:
        batch = batch.to(device=dev, dtype=torch.int64).contiguous()
    pe = torch.empty((n, 2 * d), dtype=dtype, device=dev)
    z1 = torch.empty((2 * n, d), dtype=dtype, device=dev) if train else None
    pn = torch.empty(2 * n, dtype=torch.float32, device=dev) if train else None
    pre = torch.empty_like(pe) if (train and gelu) else None
    with _lib.on_device(dev):
        rc = _lib.load().segger_posmlp_fwd(pos.data_ptr(), _lib.ptr(batch), mins.data_ptr(), maxs.data_ptr(), n, float(eps),
                                           float(max_period), pk0.w.data_ptr(), pk0.b.data_ptr(), pk2.w.data_ptr(),
                                           pk2.b.data_ptr(), pe.data_ptr(), _lib.ptr(z1), _lib.ptr(pn), None, _lib.ptr(pre),
                                           int(gelu), DTYPE_CODE[dtype], _lib.stream_ptr(dev))
    _lib.check(rc, "segger_posmlp_fwd")
    return pe, z1, pn, pre


class _PosMlpPair(torch.autograd.Function):
    """``Positional2dEmbedder`` of TWO row sets as one autograd node: a = the transcripts (GELU applied in the kernel,
    ``(gelu(pre), pre)`` out as ``posmlp(return_pre=True)``), b = the boundaries (plain).  Two forward launches; the
    backward is ONE ``segger_posmlp_bwd_pair`` launch whose partial sums cover both sets, so the embedder's parameters get a
    single gradient each -- two ``_PosMlp`` nodes cost four accumulation launches behind autograd."""

    @staticmethod
    def forward(ctx, pos_a, batch_a, mins_a, maxs_a, pos_b, batch_b, mins_b, maxs_b, eps, max_period, dtype, w0, b0, w2, b2):
        _lib.require_cuda(pos_a, pos_b, w0)
        dev = pos_a.device
        d = int(w0.shape[0])
        pk0 = _pack_for((w0,), (b0,)).get(dtype, dev)
        pk2 = _pack_for((w2,), (b2,)).get(dtype, dev)
        ctx.set_materialize_grads(False)
        pe_a, z1_a, pn_a, pre_a = _posmlp_fwd_launch(pos_a, batch_a, mins_a, maxs_a, eps, max_period, dtype, True, 2, pk0, pk2, d)
        pe_b, z1_b, pn_b, _ = _posmlp_fwd_launch(pos_b, batch_b, mins_b, maxs_b, eps, max_period, dtype, True, 0, pk0, pk2, d)
        ctx.save_for_backward(z1_a, pn_a, z1_b, pn_b)
        ctx.pk2, ctx.key2, ctx.max_period = pk2, pk2.key, float(max_period)
        ctx.mark_non_differentiable(pe_a)                    # gelu(pre) leaves as a constant; `pre` carries the gradient
        return pe_a, pre_a, pe_b

    @staticmethod
    def backward(ctx, _gpe_a, gpre_a, gpe_b):
        z1_a, pn_a, z1_b, pn_b = ctx.saved_tensors
        if gpre_a is None and gpe_b is None:
            return (None,) * 15
        if ctx.pk2.key != ctx.key2:
            raise RuntimeError("the positional MLP's weights changed between this forward and its backward")
        dt, d, dev = z1_a.dtype, int(z1_a.shape[1]), z1_a.device
        lib = _lib.load()

        def rows(g):
            if g is None:
                return None, d, 0
            g = _grad_rows(g.reshape(-1, d), dt)
            gp, ldg = _rows(g, d, "g")
            return (g, gp), ldg, int(g.shape[0])
        ga, lda, na = rows(gpre_a)
        gb, ldb, nb = rows(gpe_b)
        gw0 = torch.empty((d, 4 * d), dtype=torch.float32, device=dev)
        gb0 = torch.empty(d, dtype=torch.float32, device=dev)
        gw2 = torch.empty((d, d), dtype=torch.float32, device=dev)
        gb2 = torch.empty(d, dtype=torch.float32, device=dev)
        ws_bytes = lib.segger_posmlp_bwd_pair_workspace_bytes(na, nb)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.segger_posmlp_bwd_pair(ga[1] if ga else None, lda, z1_a.data_ptr(), pn_a.data_ptr(), na,
                                            gb[1] if gb else None, ldb, z1_b.data_ptr(), pn_b.data_ptr(), nb,
                                            ctx.pk2.wt.data_ptr(), ctx.max_period, DTYPE_CODE[dt], gw0.data_ptr(), gb0.data_ptr(),
                                            gw2.data_ptr(), gb2.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
        _lib.check(rc, "segger_posmlp_bwd_pair")
        _defer_keep(ws, gw0, gb0, gw2, gb2, ga, gb)
        need = ctx.needs_input_grad
        return (None,) * 11 + (gw0 if need[11] else None, gb0 if need[12] else None, gw2 if need[13] else None,
                               gb2 if need[14] else None)


def posmlp_pair_supported(w0: Tensor, b0, w2: Tensor, b2, dtype: torch.dtype) -> bool:
    """The one-node route of :func:`posmlp_pair`: the fused 16-bit embedder with its one-pass backward, training."""
    return (ops.FUSED_POSMLP_BWD and b0 is not None and b2 is not None and posmlp_supported(w0.shape[1], w0.shape[0], dtype)
            and tuple(w2.shape) == (w0.shape[0], w0.shape[0]) and torch.is_grad_enabled()
            and any(t.requires_grad for t in (w0, b0, w2, b2)))


def posmlp_pair(pos_a: Tensor, batch_a, mins_a: Tensor, maxs_a: Tensor, pos_b: Tensor, batch_b, mins_b: Tensor, maxs_b: Tensor,
                w0: Tensor, b0: Tensor, w2: Tensor, b2: Tensor, dtype: torch.dtype, eps: float = 1e-8, max_period: float = 10000.0):
    """``((gelu(pe_a), pe_a), pe_b)``: :func:`posmlp` of two row sets (``a`` as ``gelu=True, return_pre=True``, ``b`` plain)
    behind ONE autograd node (:class:`_PosMlpPair`); see :func:`posmlp_pair_supported`."""
    if not posmlp_pair_supported(w0, b0, w2, b2, dtype):
        raise ValueError("posmlp_pair: unsupported (see posmlp_pair_supported)")
    act_a, pre_a, pe_b = _PosMlpPair.apply(pos_a, batch_a, mins_a, maxs_a, pos_b, batch_b, mins_b, maxs_b, eps, max_period, dtype,
                                           w0, b0, w2, b2)
    return (act_a, pre_a), pe_b


def posmlp(pos: Tensor, batch: Optional[Tensor], mins: Tensor, maxs: Tensor, w0: Tensor, b0: Tensor, w2: Tensor,
           b2: Tensor, dtype: torch.dtype, eps: float = 1e-8, max_period: float = 10000.0, gelu: bool = False,
           return_pre: bool = False):
    """``Positional2dEmbedder.forward`` (reference ist_encoder.py:33-79) for bf16 / f16 activations; ``gelu``: the GELU
    that ISTEncoder applies to the concatenated input (ist_encoder.py:324-325) on top, in the same kernel.
    ``return_pre`` (with ``gelu``): ``(gelu(pre), pre)`` where the first is a constant for autograd and ``pre`` (the
    embedder's output, None when nothing needs a gradient) carries the gradient -- for a consumer that multiplies by
    gelu'(pre) itself (``embed_linear``)."""
    if not posmlp_supported(w0.shape[1], w0.shape[0], dtype) or tuple(w2.shape) != (w0.shape[0], w0.shape[0]):
        raise ValueError("posmlp: unsupported shapes (see segger_posmlp_supported)")
    if b0 is None or b2 is None:
        raise ValueError("posmlp: the embedder's Linear layers carry biases")
    train = torch.is_grad_enabled() and any(t.requires_grad for t in (w0, b0, w2, b2))   # else nothing is stored
    if return_pre and gelu:
        if train:
            return _PosMlp.apply(pos, batch, mins, maxs, eps, max_period, dtype, train, 2, w0, b0, w2, b2)
        return _PosMlp.apply(pos, batch, mins, maxs, eps, max_period, dtype, train, 1, w0, b0, w2, b2), None
    return _PosMlp.apply(pos, batch, mins, maxs, eps, max_period, dtype, train, int(bool(gelu)), w0, b0, w2, b2)
