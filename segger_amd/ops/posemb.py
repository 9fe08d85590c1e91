from __future__ import annotations

import functools
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
# Positional embedder: what every launcher and autograd node below shares
# --------------------------------------------------------------------------
def _pos_batch(pos: Tensor, batch: Optional[Tensor]):
    """-> (positions as contiguous fp32, batch vector as contiguous int64 on their device | None): what the kernels read."""
    pos = pos.to(torch.float32).contiguous()
    if batch is not None:
        batch = batch.to(device=pos.device, dtype=torch.int64).contiguous()
    return pos, batch


def _check_minmax(what: str, mins: Tensor, maxs: Tensor, pos: Tensor, num_graphs: Optional[int] = None) -> None:
    """The kernels read ``float[num_graphs][2]`` through raw pointers: anything else is refused here, before a launch."""
    for t in (mins, maxs):
        if (t.dtype != torch.float32 or not t.is_contiguous() or t.device != pos.device
                or (num_graphs is not None and t.numel() < 2 * num_graphs)):
            raise ValueError(f"{what}: mins / maxs must be contiguous float32 [num_graphs, 2] tensors on pos's device")


def _check_pack(ctx) -> None:
    """``ctx.pk2`` (the 16-bit copy of W2 a forward ran on, ``ctx.key2`` its key then) still is that copy."""
    if ctx.pk2.key != ctx.key2:
        raise RuntimeError("the positional MLP's weights changed between this forward and its backward")


def _param_grads(ctx, *grads):
    """A backward's return value where the node's LAST inputs are the parameters: None for whatever needs no gradient."""
    need = ctx.needs_input_grad
    lead = len(need) - len(grads)
    return (None,) * lead + tuple(g if wanted else None for g, wanted in zip(grads, need[lead:]))


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
    pos, batch = _pos_batch(pos, batch)
    dev = pos.device
    if pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError("segment_minmax: pos must be [n, 2]")
    if batch is not None and batch.numel() != pos.shape[0]:
        raise ValueError("segment_minmax: batch / pos length mismatch")
    flags = 2 if keep_empty else 0
    if out is not None:
        mins, maxs = out
        _check_minmax("segment_minmax: out", mins, maxs, pos, num_graphs)
        flags |= 1
    else:
        mins = torch.empty((num_graphs, 2), dtype=torch.float32, device=dev)
        maxs = torch.empty((num_graphs, 2), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = lib.segger_segment_minmax_ex(pos.data_ptr(), _lib.ptr(batch), int(pos.shape[0]), int(num_graphs),
                                          mins.data_ptr(), maxs.data_ptr(), flags, _lib.stream_ptr(dev))
    _lib.check(rc, "segger_segment_minmax_ex")
    return mins, maxs


# --------------------------------------------------------------------------
# fp32 storage: the embedder's MLP as one autograd node, two forms of its first layer
# --------------------------------------------------------------------------
def _f32_second_layer(ctx, h1, w2, b2, gelu_out):
    """The forward tail of both fp32 nodes: ``linear(h1, w2, b2)``, or with ``gelu_out`` ``(y, gelu(y))`` from one kernel, the
    second a constant for autograd."""
    w2d = w2.detach().contiguous()
    if gelu_out:
        y, gy_ = linear_f32_act_launch(h1, w2d, b2, "gelu")
        ctx.mark_non_differentiable(gy_)
        return y, gy_
    return linear_fwd_launch(h1, w2d, b2.detach())


def _f32_backward_head(gy, z1, h1, w2):
    """The backward head of both fp32 nodes -> (dz1, dW2, db2): the SiLU derivative rides in the epilogue of the data-gradient
    GEMM (``segger_linear_fwd_f32_gate``) instead of torch's silu_backward pass."""
    gy = gy.contiguous()
    gw2, gb2 = linear_wgrad_launch(gy, h1)
    return linear_f32_gate_launch(gy, w2.detach().t().contiguous(), z1, "silu"), gw2, gb2


class _MlpSiluF32(torch.autograd.Function):
    """``linear(silu(linear(x, w0, b0)), w2, b2)`` at fp32 storage as ONE autograd node (the positional embedder's shared MLP,
    ist_encoder.py:43-49, on its un-fused route).  ``x`` receives no gradient (the sinusoid features are constants)."""

    @staticmethod
    def forward(ctx, x, w0, b0, w2, b2, gelu_out=False):
        z1, h1 = linear_f32_act_launch(x, w0.detach().contiguous(), b0, "silu")    # pre-activation and SiLU from one kernel
        ctx.save_for_backward(x, z1, h1, w2)
        return _f32_second_layer(ctx, h1, w2, b2, gelu_out)

    @staticmethod
    def backward(ctx, gy, _unused=None):
        x, z1, h1, w2 = ctx.saved_tensors
        dz1, gw2, gb2 = _f32_backward_head(gy, z1, h1, w2)
        gw0, gb0 = linear_wgrad_launch(dz1, x)
        return None, gw0, gb0, gw2, gb2, None


def mlp_silu_f32_covers(d_in: int, d_h: int, d_out: int) -> bool:
    """The widths :func:`mlp_silu_f32` has kernels for (forward, gate and weight gradient of both layers)."""
    return (linear_supported(d_in, d_h, torch.float32) and linear_supported(d_h, d_out, torch.float32)
            and linear_wgrad_supported(d_h, d_in, torch.float32) and linear_wgrad_supported(d_out, d_h, torch.float32)
            and linear_f32_gate_supported(d_out, d_h) and d_in in (64, 128, 256) and d_h in (64, 128, 256)
            and d_h % 64 == 0 and d_out % 64 == 0)


def mlp_silu_f32_supported(x: Tensor, w0: Tensor, w2: Tensor) -> bool:
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] > 0 and not x.requires_grad
            and mlp_silu_f32_covers(int(w0.shape[1]), int(w0.shape[0]), int(w2.shape[0])))


def mlp_silu_f32(x: Tensor, w0, b0, w2, b2, gelu_out: bool = False):
    """``linear(silu(linear(x)))``; ``gelu_out``: ``(y, gelu(y))`` with the GELU a constant for autograd (the gradient is
    expected for ``y``: the consumer applies gelu')."""
    return _MlpSiluF32.apply(x, w0, b0, w2, b2, gelu_out)


def pos_poly_f32_covers(fd: int, dim: int) -> bool:
    """The widths :func:`pos_poly_mlp_f32` has kernels for, with its switch (``ops.POS_POLY_F32``)."""
    return bool(ops.POS_POLY_F32 and _lib.load().segger_posenc_poly_supported(int(fd), int(dim))
                and linear_supported(dim, dim, torch.float32) and linear_wgrad_supported(dim, dim, torch.float32)
                and linear_f32_gate_supported(dim, dim) and dim % 64 == 0)


def pos_poly_mlp_f32_supported(pos: Tensor, w0: Tensor, w2: Tensor) -> bool:
    dim, fd = int(w0.shape[0]), int(w0.shape[1])
    return (pos.is_cuda and pos.dim() == 2 and pos.shape[1] == 2 and pos.shape[0] > 0 and not pos.requires_grad
            and w0.dtype == torch.float32 and w2.dtype == torch.float32 and tuple(w2.shape) == (dim, dim)
            and pos_poly_f32_covers(fd, dim))


class _PosPolyMlpF32(torch.autograd.Function):
    """``Linear -> SiLU -> Linear`` of ``Positional2dEmbedder`` on the sinusoid of the normalised coordinates at fp32 storage,
    from the POSITIONS (ist_encoder.py:57-79 in one autograd node): the first layer by ``segger_posenc_poly_fwd`` (13
    coefficients per channel, refreshed from W0 / b0 by ``segger_posenc_poly_coef``), its weight gradient by
    ``segger_posenc_poly_wgrad`` (13 moments per channel); the 64-wide second layer on the exact-fp32 kernels as before."""

    @staticmethod
    def forward(ctx, pos, batch, mins, maxs, num_graphs, eps, max_period, w0, b0, w2, b2, gelu_out=False):
        lib = _lib.load()
        pos, batch = _pos_batch(pos, batch)
        _check_minmax("pos_poly_mlp_f32", mins, maxs, pos, num_graphs)
        dev, n, dim, fd = pos.device, int(pos.shape[0]), int(w0.shape[0]), int(w0.shape[1])
        w0d, b0d = w0.detach().contiguous(), b0.detach().float().contiguous()
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
        return _f32_second_layer(ctx, h1, w2, b2, gelu_out)

    @staticmethod
    def backward(ctx, gy, _unused=None):
        pn, z1, h1, w2 = ctx.saved_tensors
        fd, dim, max_period = ctx.cfg
        lib = _lib.load()
        dev = gy.device
        dz1, gw2, gb2 = _f32_backward_head(gy, z1, h1, w2)
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
        return None, None, None, None, None, None, None, gw0, gb0, gw2, gb2, None


def pos_poly_mlp_f32(pos: Tensor, batch: Optional[Tensor], mins: Tensor, maxs: Tensor, w0, b0, w2, b2, *, eps: float = 1e-8,
                     max_period: float = 10000.0, gelu_out: bool = False, num_graphs: Optional[int] = None):
    """[n, 2] positions -> the embedder's MLP output as coordinate rows [2n, dim] (``gelu_out``: ``(y, gelu(y))``, the GELU a
    constant for autograd as in :func:`mlp_silu_f32`).  ``num_graphs``: rows of ``mins`` / ``maxs`` to insist on."""
    return _PosPolyMlpF32.apply(pos, batch, mins, maxs, num_graphs, eps, max_period, w0, b0, w2, b2, gelu_out)


@torch.no_grad()
def posfreq(pos: Tensor, batch: Optional[Tensor], mins: Tensor, maxs: Tensor, freq_dim: int, dtype: torch.dtype,
            eps: float = 1e-8, max_period: float = 10000.0, num_graphs: Optional[int] = None) -> Tensor:
    """[n, 2] positions -> [n, 2, freq_dim] sinusoid of the per-graph normalised coordinates."""
    _lib.require_cuda(pos)
    lib = _lib.load()
    pos, batch = _pos_batch(pos, batch)
    _check_minmax("posfreq", mins, maxs, pos, num_graphs)
    dev, n = pos.device, int(pos.shape[0])
    out = torch.empty((n, 2, freq_dim), dtype=dtype, device=dev)
    with _lib.on_device(dev):
        rc = lib.segger_posfreq(pos.data_ptr(), _lib.ptr(batch), mins.data_ptr(), maxs.data_ptr(), n, freq_dim,
                                eps, max_period, out.data_ptr(), DTYPE_CODE[dtype], _lib.stream_ptr(dev))
    _lib.check(rc, "segger_posfreq")
    return out


# --------------------------------------------------------------------------
# 16-bit storage: the whole embedder in one kernel; one launcher per kernel, shared by the two autograd nodes
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _posmlp_covers(freq_dim: int, dim: int, code: int) -> bool:
    return bool(_lib.load().segger_posmlp_supported(freq_dim, dim, code))    # (asked several times per embedder call)


def posmlp_supported(freq_dim: int, dim: int, dtype: torch.dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and _posmlp_covers(int(freq_dim), int(dim), DTYPE_CODE[dtype])


def _posmlp_fwd_launch(pos, batch, mins, maxs, eps, max_period, dtype, pk0, pk2, d, *, train, gelu, keep_h1=False):
    """One ``segger_posmlp_fwd`` launch -> (pe, z1, pn, pre, h1): what ``_PosMlp`` / ``_PosMlpPair`` keep of a row set.  With
    gradients the kernel also stores the first layer's pre-activation and the normalised coordinates (4 bytes per row), with
    ``gelu`` the output before it, with ``keep_h1`` the SiLU.  The caller checked ``mins`` / ``maxs`` before it cast weights."""
    pos, batch = _pos_batch(pos, batch)
    dev, n = pos.device, int(pos.shape[0])
    pe = torch.empty((n, 2 * d), dtype=dtype, device=dev)
    z1 = torch.empty((2 * n, d), dtype=dtype, device=dev) if train else None
    pn = torch.empty(2 * n, dtype=torch.float32, device=dev) if train else None
    pre = torch.empty_like(pe) if (train and gelu) else None
    h1 = torch.empty_like(z1) if (train and keep_h1) else None
    with _lib.on_device(dev):
        rc = _lib.load().segger_posmlp_fwd(pos.data_ptr(), _lib.ptr(batch), mins.data_ptr(), maxs.data_ptr(), n, float(eps),
                                           float(max_period), pk0.w.data_ptr(), pk0.b.data_ptr(), pk2.w.data_ptr(),
                                           pk2.b.data_ptr(), pe.data_ptr(), _lib.ptr(z1), _lib.ptr(pn), _lib.ptr(h1),
                                           _lib.ptr(pre), int(bool(gelu)), DTYPE_CODE[dtype], _lib.stream_ptr(dev))
    _lib.check(rc, "segger_posmlp_fwd")
    return pe, z1, pn, pre, h1


def _posmlp_bwd_launch(set_a, set_b, wt, max_period, dt, d):
    """One ``segger_posmlp_bwd_pair`` launch over two row sets ``(grad rows as _grad_rows leaves them | None, z1, pn)`` ->
    (dW0, db0, dW2, db2) fp32, the partial sums of both sets summed together.  A set without a gradient is an empty side, and
    an all-None ``set_b`` makes this the single-set backward (``segger_posmlp_bwd`` is that call in C; it has no caller here)."""
    lib, dev = _lib.load(), wt.device
    sides = [(None, d, None, None, 0) if g is None else _rows(g, d, "g") + (z1.data_ptr(), pn.data_ptr(), int(g.shape[0]))
             for g, z1, pn in (set_a, set_b)]
    gw0, gb0, gw2, gb2 = (torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((d, 4 * d), d, (d, d), d))
    ws_bytes = lib.segger_posmlp_bwd_pair_workspace_bytes(sides[0][4], sides[1][4])
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        rc = lib.segger_posmlp_bwd_pair(*sides[0], *sides[1], wt.data_ptr(), max_period, DTYPE_CODE[dt], gw0.data_ptr(),
                                        gb0.data_ptr(), gw2.data_ptr(), gb2.data_ptr(), ws.data_ptr(), ws_bytes,
                                        _lib.stream_ptr(dev))
    _lib.check(rc, "segger_posmlp_bwd_pair")
    _defer_keep(ws, gw0, gb0, gw2, gb2, set_a[0], set_b[0])
    return gw0, gb0, gw2, gb2


def _silu_grad_launch(g, wt, z1):
    """One ``segger_linear_fwd_silu_grad`` launch -> dz1 = (g @ W2) * silu'(z1): the SiLU derivative in the GEMM's epilogue."""
    d, dev = int(z1.shape[1]), z1.device
    dz1 = torch.empty_like(z1)
    gp, ldg = _rows(g, d, "g")
    with _lib.on_device(dev):
        rc = _lib.load().segger_linear_fwd_silu_grad(gp, ldg, wt.data_ptr(), z1.data_ptr(), d, dz1.data_ptr(), d,
                                                     int(g.shape[0]), d, d, DTYPE_CODE[z1.dtype], _lib.stream_ptr(dev))
    _lib.check(rc, "segger_linear_fwd_silu_grad")
    return dz1


def _posmlp_wgrad_launch(dz1, pn, max_period):
    """One ``segger_posmlp_wgrad`` launch -> (dW0, db0) fp32: dW0 = dz1^T F with the sinusoid features F regenerated from one
    float per row inside the kernel."""
    lib = _lib.load()
    d, dev, rows = int(dz1.shape[1]), dz1.device, int(dz1.shape[0])
    gw0 = torch.empty((d, 4 * d), dtype=torch.float32, device=dev)
    gb0 = torch.empty(d, dtype=torch.float32, device=dev)
    ws_bytes = lib.segger_linear_wgrad_workspace_bytes(rows, d, 4 * d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dp, ldd = _rows(dz1, d, "dz1")
    with _lib.on_device(dev):
        rc = lib.segger_posmlp_wgrad(dp, ldd, pn.data_ptr(), rows, max_period, DTYPE_CODE[dz1.dtype], gw0.data_ptr(),
                                     gb0.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
    _lib.check(rc, "segger_posmlp_wgrad")
    _defer_keep(ws, gw0, gb0)
    return gw0, gb0


class _PosMlp(torch.autograd.Function):
    """Positional2dEmbedder in one kernel (``segger_posmlp_fwd``): [n, 2] positions -> [n, 128].  The backward is one pass
    (``segger_posmlp_bwd_pair`` with an empty second side) or, with ``ops.FUSED_POSMLP_BWD`` off, assembled from the
    projection kernels: dW2 / db2 by ``segger_linear_wgrad``, dz1 by ``segger_linear_fwd_silu_grad``, dW0 / db0 by
    ``segger_posmlp_wgrad``."""

    @staticmethod
    def forward(ctx, pos, batch, mins, maxs, num_graphs, eps, max_period, dtype, train, gelu, w0, b0, w2, b2):
        _lib.require_cuda(pos, w0)
        dev = pos.device
        _check_minmax("posmlp", mins, maxs, pos, num_graphs)
        pk0 = _pack_for((w0,), (b0,)).get(dtype, dev)
        pk2 = _pack_for((w2,), (b2,)).get(dtype, dev)
        ctx.set_materialize_grads(False)
        pe, z1, pn, pre, h1 = _posmlp_fwd_launch(pos, batch, mins, maxs, eps, max_period, dtype, pk0, pk2, int(w0.shape[0]),
                                                 train=train, gelu=gelu, keep_h1=not ops.FUSED_POSMLP_BWD)
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
        dt, d = z1.dtype, int(z1.shape[1])
        if ctx.by_pre:
            gpe = gpre
        if gpe is None:                                      # (nothing downstream used the output)
            return (None,) * 14
        if pre is not None and not ctx.by_pre:               # the output was gelu(embedder output)
            gpe = torch.ops.aten.gelu_backward(gpe.to(dt), pre)
        g = _grad_rows(gpe.reshape(-1, d), dt)
        _check_pack(ctx)
        if h1 is None:                                       # one pass over g: all four parameter gradients
            return _param_grads(ctx, *_posmlp_bwd_launch((g, z1, pn), (None, None, None), ctx.pk2.wt, ctx.max_period, dt, d))
        gw2, gb2 = linear_wgrad_launch(g, h1)
        gw0, gb0 = _posmlp_wgrad_launch(_silu_grad_launch(g, ctx.pk2.wt, z1), pn, ctx.max_period)
        return _param_grads(ctx, gw0, gb0, gw2, gb2)


class _PosMlpPair(torch.autograd.Function):
    """``Positional2dEmbedder`` of TWO row sets as one autograd node: a = the transcripts (GELU applied in the kernel,
    ``(gelu(pre), pre)`` out as ``posmlp(return_pre=True)``), b = the boundaries (plain).  Two forward launches; the
    backward is ONE ``segger_posmlp_bwd_pair`` launch whose partial sums cover both sets, so the embedder's parameters get a
    single gradient each -- two ``_PosMlp`` nodes cost four accumulation launches behind autograd."""

    @staticmethod
    def forward(ctx, pos_a, batch_a, mins_a, maxs_a, pos_b, batch_b, mins_b, maxs_b, num_graphs, eps, max_period, dtype,
                w0, b0, w2, b2):
        _lib.require_cuda(pos_a, pos_b, w0)
        dev, d = pos_a.device, int(w0.shape[0])
        _check_minmax("posmlp_pair", mins_a, maxs_a, pos_a, num_graphs)
        _check_minmax("posmlp_pair", mins_b, maxs_b, pos_b, num_graphs)
        pk0 = _pack_for((w0,), (b0,)).get(dtype, dev)
        pk2 = _pack_for((w2,), (b2,)).get(dtype, dev)
        ctx.set_materialize_grads(False)
        pe_a, z1_a, pn_a, pre_a, _ = _posmlp_fwd_launch(pos_a, batch_a, mins_a, maxs_a, eps, max_period, dtype, pk0, pk2, d,
                                                        train=True, gelu=True)
        pe_b, z1_b, pn_b, _, _ = _posmlp_fwd_launch(pos_b, batch_b, mins_b, maxs_b, eps, max_period, dtype, pk0, pk2, d,
                                                    train=True, gelu=False)
        ctx.save_for_backward(z1_a, pn_a, z1_b, pn_b)
        ctx.pk2, ctx.key2, ctx.max_period = pk2, pk2.key, float(max_period)
        ctx.mark_non_differentiable(pe_a)                    # gelu(pre) leaves as a constant; `pre` carries the gradient
        return pe_a, pre_a, pe_b

    @staticmethod
    def backward(ctx, _gpe_a, gpre_a, gpe_b):
        z1_a, pn_a, z1_b, pn_b = ctx.saved_tensors
        if gpre_a is None and gpe_b is None:
            return (None,) * 16
        _check_pack(ctx)
        dt, d = z1_a.dtype, int(z1_a.shape[1])
        ga, gb = (None if g is None else _grad_rows(g.reshape(-1, d), dt) for g in (gpre_a, gpe_b))
        return _param_grads(ctx, *_posmlp_bwd_launch((ga, z1_a, pn_a), (gb, z1_b, pn_b), ctx.pk2.wt, ctx.max_period, dt, d))


def posmlp_pair_supported(w0: Tensor, b0, w2: Tensor, b2, dtype: torch.dtype) -> bool:
    """The one-node route of :func:`posmlp_pair`: the fused 16-bit embedder with its one-pass backward, training."""
    return (ops.FUSED_POSMLP_BWD and b0 is not None and b2 is not None and posmlp_supported(w0.shape[1], w0.shape[0], dtype)
            and tuple(w2.shape) == (w0.shape[0], w0.shape[0]) and torch.is_grad_enabled()
            and any(t.requires_grad for t in (w0, b0, w2, b2)))


def posmlp_pair(pos_a: Tensor, batch_a, mins_a: Tensor, maxs_a: Tensor, pos_b: Tensor, batch_b, mins_b: Tensor, maxs_b: Tensor,
                w0: Tensor, b0: Tensor, w2: Tensor, b2: Tensor, dtype: torch.dtype, eps: float = 1e-8, max_period: float = 10000.0,
                num_graphs: Optional[int] = None):
    """``((gelu(pe_a), pe_a), pe_b)``: :func:`posmlp` of two row sets (``a`` as ``gelu=True, return_pre=True``, ``b`` plain)
    behind ONE autograd node (:class:`_PosMlpPair`); see :func:`posmlp_pair_supported`."""
    if not posmlp_pair_supported(w0, b0, w2, b2, dtype):
        raise ValueError("posmlp_pair: unsupported (see posmlp_pair_supported)")
    act_a, pre_a, pe_b = _PosMlpPair.apply(pos_a, batch_a, mins_a, maxs_a, pos_b, batch_b, mins_b, maxs_b, num_graphs, eps,
                                           max_period, dtype, w0, b0, w2, b2)
    return (act_a, pre_a), pe_b


def posmlp(pos: Tensor, batch: Optional[Tensor], mins: Tensor, maxs: Tensor, w0: Tensor, b0: Tensor, w2: Tensor,
           b2: Tensor, dtype: torch.dtype, eps: float = 1e-8, max_period: float = 10000.0, gelu: bool = False,
           return_pre: bool = False, num_graphs: Optional[int] = None):
    """``Positional2dEmbedder.forward`` (reference ist_encoder.py:33-79) for bf16 / f16 activations; ``gelu``: the GELU
    that ISTEncoder applies to the concatenated input (ist_encoder.py:324-325) on top, in the same kernel.
    ``return_pre`` (with ``gelu``): ``(gelu(pre), pre)`` where the first is a constant for autograd and ``pre`` (the
    embedder's output, None when nothing needs a gradient) carries the gradient -- for a consumer that multiplies by
    gelu'(pre) itself (``embed_linear``).  ``num_graphs``: rows of ``mins`` / ``maxs`` to insist on."""
    if not posmlp_supported(w0.shape[1], w0.shape[0], dtype) or tuple(w2.shape) != (w0.shape[0], w0.shape[0]):
        raise ValueError("posmlp: unsupported shapes (see segger_posmlp_supported)")
    if b0 is None or b2 is None:
        raise ValueError("posmlp: the embedder's Linear layers carry biases")
    train = torch.is_grad_enabled() and any(t.requires_grad for t in (w0, b0, w2, b2))   # else nothing is stored
    by_pre = bool(return_pre and gelu)
    mode = 2 if (by_pre and train) else int(bool(gelu))
    r = _PosMlp.apply(pos, batch, mins, maxs, num_graphs, eps, max_period, dtype, train, mode, w0, b0, w2, b2)
    return (r, None) if (by_pre and not train) else r
