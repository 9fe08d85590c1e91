from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE
from .. import graph as _graph
from ..graph import EdgeCSR, EdgeGraph
from .. import ops                # route switches: read as ops.NAME when called, never bound here
from ._common import _bits_ptr, _defer_keep, _f32_vec, _gat_bwd_ws_bytes, _grad_rows, _has_specialised, _rows, _seed_parts


# --------------------------------------------------------------------------
# GATv2 aggregation: raw launches
# --------------------------------------------------------------------------
def gatv2_fwd_launch(by_dst: EdgeCSR, xl: Tensor, xr: Tensor, att: Tensor, bias: Optional[Tensor],
                     heads: int, channels: int, out: Tensor, *, pre: Optional[Tensor] = None,
                     lse: Optional[Tensor] = None, alpha: Optional[Tensor] = None,
                     apply_gelu: bool = False, negative_slope: float = 0.2,
                     dropout_p: float = 0.0, seed: int = 0, keep_bits: Optional[Tensor] = None) -> None:
    a, keep = _gat_fwd_args(by_dst, xl, xr, att, bias, heads, channels, out, pre=pre, lse=lse, alpha=alpha,
                            apply_gelu=apply_gelu, negative_slope=negative_slope, dropout_p=dropout_p, seed=seed,
                            keep_bits=keep_bits)
    with _lib.on_device(xl.device):
        rc = _lib.load().segger_gatv2_fwd(C.byref(a), _lib.stream_ptr(xl.device))
    _lib.check(rc, "segger_gatv2_fwd")


def gatv2_fwd_pair_launch(first: dict, second: dict) -> None:
    """Two forwards of one hetero layer in ONE launch (``segger_gatv2_fwd_pair``): ``first`` the low-degree edge type
    (tx-neighbors-tx), ``second`` the high-degree one (tx-belongs-bd); each a dict of :func:`gatv2_fwd_launch`'s
    arguments.  Falls back to two launches inside the library when the pair does not qualify."""
    a, keep_a = _gat_fwd_args(**first)
    b, keep_b = _gat_fwd_args(**second)
    dev = first["xl"].device
    lib = _lib.load()
    with _lib.on_device(dev):
        if ops._FWD_PAIR:
            rc = lib.segger_gatv2_fwd_pair(C.byref(a), C.byref(b), _lib.stream_ptr(dev))
        else:
            rc = lib.segger_gatv2_fwd(C.byref(a), _lib.stream_ptr(dev)) or lib.segger_gatv2_fwd(C.byref(b), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_gatv2_fwd_pair")


def _gat_fwd_args(by_dst: EdgeCSR, xl: Tensor, xr: Tensor, att: Tensor, bias: Optional[Tensor],
                  heads: int, channels: int, out: Tensor, *, pre: Optional[Tensor] = None,
                  lse: Optional[Tensor] = None, alpha: Optional[Tensor] = None,
                  apply_gelu: bool = False, negative_slope: float = 0.2,
                  dropout_p: float = 0.0, seed: int = 0, keep_bits: Optional[Tensor] = None):
    _lib.require_cuda(xl, xr, att, out)
    hc = heads * channels
    if not (xl.dtype == xr.dtype == out.dtype) or xl.dtype not in DTYPE_CODE:
        raise TypeError(f"gatv2: x_l/x_r/out must share a dtype in {list(DTYPE_CODE)}")
    a = _lib.GatFwdArgs()
    a.by_dst = by_dst.c_struct(ordered=_graph.ROW_ORDER_FORWARD)
    a.x_l, a.ld_xl = _rows(xl, hc, "x_l")
    a.x_r, a.ld_xr = _rows(xr, hc, "x_r")
    if xl.shape[0] != by_dst.n_cols or xr.shape[0] != by_dst.n_rows or out.shape[0] != by_dst.n_rows:
        raise ValueError("gatv2: feature row counts do not match the graph")
    vecs = (_f32_vec(att, hc, "att"), _f32_vec(bias, hc, "bias"))
    a.att, a.bias = vecs[0].data_ptr(), _lib.ptr(vecs[1])
    a.heads, a.channels, a.dtype, a.apply_gelu = heads, channels, DTYPE_CODE[xl.dtype], int(apply_gelu)
    a.negative_slope, a.dropout_p = negative_slope, dropout_p
    a.seed, a.seed_dev = _seed_parts(seed)
    a.out, a.ld_out = _rows(out, hc, "out")
    if pre is not None:
        a.pre, a.ld_pre = _rows(pre, hc, "pre")
    a.lse, a.alpha = _lib.ptr(lse), _lib.ptr(alpha)
    if keep_bits is not None and dropout_p > 0.0:
        a.keep_bits = _bits_ptr(keep_bits, by_dst.n_edges)
    return a, vecs                                       # (vecs: the fp32 copies the struct points at)


def gatv2_bwd_launch(g: EdgeGraph, xl: Tensor, xr: Tensor, att: Tensor, bias: Optional[Tensor],
                     heads: int, channels: int, grad_out: Tensor, pre: Tensor, lse: Tensor,
                     grad_xl: Tensor, grad_xr: Tensor, **kw) -> Tuple[Tensor, Tensor]:
    """Writes grad_xl / grad_xr (views allowed); returns (grad_att[HC], grad_bias[HC]) fp32.  ``zero_rows_out``: a
    second [n_src, HC] matrix the source pass zero-fills on its way (ignored when this edge type runs the one-pass form
    or the generic kernels); ``grad_xl_zeroed``: the one-pass form may skip its own zero fill."""
    a, gparams, keep, _ = _gat_bwd_args(g, xl, xr, att, bias, heads, channels, grad_out, pre, lse, grad_xl, grad_xr, **kw)
    with _lib.on_device(xl.device):
        rc = _lib.load().segger_gatv2_bwd(C.byref(a), _lib.stream_ptr(xl.device))
    _lib.check(rc, "segger_gatv2_bwd")
    return gparams[0], gparams[1]


def gatv2_bwd_pair_launch(first: tuple, first_kw: dict, second: tuple, second_kw: dict):
    """The backward of both edge types of one hetero layer through ``segger_gatv2_bwd_pair``: ``first`` the two-pass
    edge type (tx-neighbors-tx), ``second`` the one-pass one (tx-belongs-bd), each the positional / keyword arguments
    of :func:`gatv2_bwd_launch`.  ``second``'s ``grad_xl`` is the matrix ``first`` zero-fills (``zero_rows_out``); the
    library merges the source pass of ``first`` with the destination pass of ``second`` (and the two slab sums) where
    the pair qualifies and runs the two backward passes one after the other otherwise.  -> ((grad_att, grad_bias) of first, of second)."""
    a, gp_a, keep_a, zeroed = _gat_bwd_args(*first, **first_kw)
    b, gp_b, keep_b, _ = _gat_bwd_args(*second, grad_xl_zeroed=zeroed, **second_kw)
    dev = first[1].device
    lib = _lib.load()
    with _lib.on_device(dev):
        if ops._BWD_PAIR:
            rc = lib.segger_gatv2_bwd_pair(C.byref(a), C.byref(b), _lib.stream_ptr(dev))
        else:
            rc = lib.segger_gatv2_bwd(C.byref(a), _lib.stream_ptr(dev)) or lib.segger_gatv2_bwd(C.byref(b), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_gatv2_bwd_pair")
    return (gp_a[0], gp_a[1]), (gp_b[0], gp_b[1])


def _gat_bwd_args(g: EdgeGraph, xl: Tensor, xr: Tensor, att: Tensor, bias: Optional[Tensor],
                  heads: int, channels: int, grad_out: Tensor, pre: Tensor, lse: Tensor,
                  grad_xl: Tensor, grad_xr: Tensor, *, apply_gelu: bool, negative_slope: float = 0.2,
                  dropout_p: float = 0.0, seed: int = 0, keep_bits: Optional[Tuple] = None,
                  zero_rows_out: Optional[Tensor] = None, grad_xl_zeroed: bool = False, passes: int = 0,
                  scratch: Optional[Tuple[Tensor, Tensor]] = None):
    """-> (segger_gatv2_bwd_args, gparams [2, HC] fp32, the tensors the struct points at, whether the source pass
    zero-fills ``zero_rows_out``).  ``passes`` (1: destination pass alone, 2: source pass alone over the ``scratch`` =
    (grad_pre, dsum) a passes = 1 call returned in ``gatv2_bwd_launch.scratch``): timing hooks of bench.py, see
    include/segger_amd.h."""
    _lib.require_cuda(xl, xr, grad_out)
    lib = _lib.load()
    hc = heads * channels
    dev, dt = xl.device, xl.dtype
    n_dst = g.n_dst
    a = _lib.GatBwdArgs()
    a.by_dst = g.by_dst.c_struct()
    zero_filled = False
    if g.by_src is None and g.src_unique() and _has_specialised(heads, channels):
        a.src_unique = 1          # every source has at most one out-edge: the destination pass stores grad_xl itself
        a.grad_xl_zeroed = int(bool(grad_xl_zeroed))
    else:
        a.by_src = g.require_by_src().c_struct()
        if zero_rows_out is not None and _has_specialised(heads, channels) and g.n_src > 0:
            a.zero_rows_out, a.ld_zero = _rows(zero_rows_out, hc, "zero_rows_out")
            zero_filled = True
    a.x_l, a.ld_xl = _rows(xl, hc, "x_l")
    a.x_r, a.ld_xr = _rows(xr, hc, "x_r")
    vecs = (_f32_vec(att, hc, "att"), _f32_vec(bias, hc, "bias"))
    a.att, a.bias = vecs[0].data_ptr(), _lib.ptr(vecs[1])
    a.heads, a.channels, a.dtype, a.apply_gelu = heads, channels, DTYPE_CODE[dt], int(apply_gelu)
    a.negative_slope, a.dropout_p = negative_slope, dropout_p
    a.seed, a.seed_dev = _seed_parts(seed)
    if keep_bits is not None and dropout_p > 0.0:
        if keep_bits[0] is not None:
            a.keep_bits_dst = _bits_ptr(keep_bits[0], g.n_edges)
        if keep_bits[1] is not None:
            a.keep_bits_src = _bits_ptr(keep_bits[1], g.n_edges)
    grad_out = _grad_rows(grad_out, dt)
    a.grad_out, a.ld_go = _rows(grad_out, hc, "grad_out")
    a.pre, a.ld_pre = _rows(pre, hc, "pre")
    a.lse = lse.data_ptr()
    if scratch is not None:
        grad_pre, dsum = scratch
    else:
        grad_pre = torch.empty((n_dst, hc), dtype=dt, device=dev)
        dsum = torch.empty((n_dst, heads, 2), dtype=torch.float32, device=dev)     # (lse, D) pairs for the source pass
    a.passes = int(passes)
    gatv2_bwd_launch.scratch = (grad_pre, dsum)
    a.grad_pre, a.ld_gp = _rows(grad_pre, hc, "grad_pre")
    a.dsum = dsum.data_ptr()
    a.grad_xl, a.ld_gxl = _rows(grad_xl, hc, "grad_xl")
    a.grad_xr, a.ld_gxr = _rows(grad_xr, hc, "grad_xr")
    gparams = torch.empty((2, hc), dtype=torch.float32, device=dev)
    a.grad_att, a.grad_bias = gparams[0].data_ptr(), gparams[1].data_ptr()
    two_pass = not a.src_unique
    ws_bytes = _gat_bwd_ws_bytes(n_dst, g.n_src if two_pass else 0, g.n_edges if two_pass else 0, heads, channels)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    _defer_keep(ws, gparams)
    return a, gparams, (vecs, grad_out, grad_pre, dsum, ws), zero_filled


class _GatV2Aggregate(torch.autograd.Function):
    """One edge type: (x_l, x_r, att, bias) -> out [n_dst, H*C] (GELU optionally fused)."""

    @staticmethod
    def forward(ctx, xl, xr, att, bias, graph: EdgeGraph, heads, channels, apply_gelu,
                negative_slope, dropout_p, seed, want_alpha, keep_bits=None):
        hc = heads * channels
        dev, dt = xl.device, xl.dtype
        n_dst = graph.n_dst
        need_grad = any(ctx.needs_input_grad[:4])
        out = torch.empty((n_dst, hc), dtype=dt, device=dev)
        pre = torch.empty((n_dst, hc), dtype=dt, device=dev) if (need_grad and apply_gelu) else None
        lse = torch.empty((n_dst, heads), dtype=torch.float32, device=dev) if need_grad else None
        alpha = torch.empty((graph.n_edges, heads), dtype=torch.float32, device=dev) if want_alpha else None
        gatv2_fwd_launch(graph.by_dst, xl, xr, att, bias, heads, channels, out, pre=pre, lse=lse, alpha=alpha,
                         apply_gelu=apply_gelu, negative_slope=negative_slope, dropout_p=dropout_p, seed=seed,
                         keep_bits=None if keep_bits is None else keep_bits[0])
        if need_grad:
            ctx.save_for_backward(xl, xr, att, bias, pre if apply_gelu else out, lse)
            ctx.graph, ctx.cfg = graph, (heads, channels, apply_gelu, negative_slope, dropout_p, seed)
            ctx.keep_bits = keep_bits
        if want_alpha:
            ctx.mark_non_differentiable(alpha)
            return out, alpha
        return out, None

    @staticmethod
    def backward(ctx, grad_out, _grad_alpha):
        xl, xr, att, bias, pre, lse = ctx.saved_tensors
        heads, channels, apply_gelu, slope, p, seed = ctx.cfg
        g = ctx.graph
        hc = heads * channels
        gxl = torch.empty((g.n_src, hc), dtype=xl.dtype, device=xl.device)
        gxr = torch.empty((g.n_dst, hc), dtype=xl.dtype, device=xl.device)
        gatt, gbias = gatv2_bwd_launch(g, xl, xr, att, bias, heads, channels, grad_out, pre, lse, gxl, gxr,
                                       apply_gelu=apply_gelu, negative_slope=slope, dropout_p=p, seed=seed,
                                       keep_bits=ctx.keep_bits)
        gatt = gatt.reshape(att.shape).to(att.dtype)
        gbias = gbias.reshape(bias.shape).to(bias.dtype) if bias is not None else None
        return gxl, gxr, gatt, gbias, None, None, None, None, None, None, None, None, None


def gatv2_aggregate(xl: Tensor, xr: Tensor, att: Tensor, bias: Optional[Tensor], graph: EdgeGraph,
                    heads: int, channels: int, *, apply_gelu: bool = False, negative_slope: float = 0.2,
                    dropout_p: float = 0.0, seed: int = 0, return_alpha: bool = False, keep_bits=None):
    """``keep_bits`` = (by_dst bits, by_src bits or None): one layer's planes of :func:`dropout_bits` for ``seed``."""
    out, alpha = _GatV2Aggregate.apply(xl, xr, att, bias, graph, heads, channels, apply_gelu,
                                       negative_slope, dropout_p, seed, return_alpha, keep_bits)
    return (out, alpha) if return_alpha else out


class _HeteroGatLayer(torch.autograd.Function):
    """segger's HeteroConv layer as one autograd node.

    ``xp_tx`` = [lin_l(tx-tx) | lin_r(tx-tx) | lin_l(tx-bd)] (x_tx), one fused
    projection [Nt, 3*HC]; ``xp_bd`` = lin_r(tx-bd)(x_bd) [Nb, HC].  The three
    backward passes write their slices of one [Nt, 3*HC] gradient, so the
    projection's backward is a single GEMM (no slice-zero-add chains).
    """

    @staticmethod
    def forward(ctx, xp_tx, xp_bd, att_tt, bias_tt, att_tb, bias_tb, g_tt: EdgeGraph, g_tb: EdgeGraph,
                heads, channels, apply_gelu, slope, dropout_p, seed_tt, seed_tb, want_alpha, bits_tt=None, bits_tb=None):
        hc = heads * channels
        dev, dt = xp_tx.device, xp_tx.dtype
        need_grad = any(ctx.needs_input_grad[:6])
        xl_tt, xr_tt, xl_tb = xp_tx[:, :hc], xp_tx[:, hc:2 * hc], xp_tx[:, 2 * hc:]
        nt, nb = xp_tx.shape[0], xp_bd.shape[0]
        y_tx = torch.empty((nt, hc), dtype=dt, device=dev)
        y_bd = torch.empty((nb, hc), dtype=dt, device=dev)
        mk = lambda n: torch.empty((n, hc), dtype=dt, device=dev) if (need_grad and apply_gelu) else None
        pre_tx, pre_bd = mk(nt), mk(nb)
        lse_tx = torch.empty((nt, heads), dtype=torch.float32, device=dev) if need_grad else None
        lse_bd = torch.empty((nb, heads), dtype=torch.float32, device=dev) if need_grad else None
        alpha = torch.empty((g_tt.n_edges, heads), dtype=torch.float32, device=dev) if want_alpha else None
        # both edge types in ONE launch (segger_gatv2_fwd_pair): at segger's default batch size the tx-belongs-bd blocks
        # disappear inside the tx-neighbors-tx launch (46 -> 40 us per layer); at C2 it measures neutral
        gatv2_fwd_pair_launch(
            dict(by_dst=g_tt.by_dst, xl=xl_tt, xr=xr_tt, att=att_tt, bias=bias_tt, heads=heads, channels=channels, out=y_tx,
                 pre=pre_tx, lse=lse_tx, alpha=alpha, apply_gelu=apply_gelu, negative_slope=slope, dropout_p=dropout_p,
                 seed=seed_tt, keep_bits=None if bits_tt is None else bits_tt[0]),
            dict(by_dst=g_tb.by_dst, xl=xl_tb, xr=xp_bd, att=att_tb, bias=bias_tb, heads=heads, channels=channels, out=y_bd,
                 pre=pre_bd, lse=lse_bd, apply_gelu=apply_gelu, negative_slope=slope, dropout_p=dropout_p, seed=seed_tb,
                 keep_bits=None if bits_tb is None else bits_tb[0]))
        if need_grad:
            ctx.save_for_backward(xp_tx, xp_bd, att_tt, bias_tt, att_tb, bias_tb,
                                  pre_tx if apply_gelu else y_tx, pre_bd if apply_gelu else y_bd, lse_tx, lse_bd)
            ctx.graphs = (g_tt, g_tb)
            ctx.cfg = (heads, channels, apply_gelu, slope, dropout_p, seed_tt, seed_tb)
            ctx.bits = (bits_tt, bits_tb)
        if want_alpha:
            ctx.mark_non_differentiable(alpha)
        return y_tx, y_bd, alpha

    @staticmethod
    def backward(ctx, gy_tx, gy_bd, _ga):
        xp_tx, xp_bd, att_tt, bias_tt, att_tb, bias_tb, pre_tx, pre_bd, lse_tx, lse_bd = ctx.saved_tensors
        heads, channels, apply_gelu, slope, p, seed_tt, seed_tb = ctx.cfg
        g_tt, g_tb = ctx.graphs
        hc = heads * channels
        gxp_tx = torch.empty_like(xp_tx)
        gxp_bd = torch.empty_like(xp_bd)
        if gy_tx is None:
            gy_tx = torch.zeros_like(pre_tx)
        if gy_bd is None:
            gy_bd = torch.zeros_like(pre_bd)
        # tx-neighbors-tx first: its source pass visits every transcript row and zero-fills the tx-belongs-bd window of
        # the stacked projection gradient on the way, so the one-pass tx-belongs-bd backward needs no fill of its own.
        # (Running tx-belongs-bd on a second stream beside it was measured in round 3: the kernels do overlap, but the
        # small one then takes 10x longer and the big ones 3-7 % longer -- same total)
        # The library goes one step further (segger_gatv2_bwd_pair, every batch size): the tx-neighbors-tx DESTINATION
        # pass does the zero fill and its source pass shares a launch with the tx-belongs-bd pass.
        (gatt_tt, gbias_tt), (gatt_tb, gbias_tb) = gatv2_bwd_pair_launch(
            (g_tt, xp_tx[:, :hc], xp_tx[:, hc:2 * hc], att_tt, bias_tt, heads, channels, gy_tx, pre_tx, lse_tx,
             gxp_tx[:, :hc], gxp_tx[:, hc:2 * hc]),
            dict(apply_gelu=apply_gelu, negative_slope=slope, dropout_p=p, seed=seed_tt, keep_bits=ctx.bits[0],
                 zero_rows_out=gxp_tx[:, 2 * hc:]),
            (g_tb, xp_tx[:, 2 * hc:], xp_bd, att_tb, bias_tb, heads, channels, gy_bd, pre_bd, lse_bd,
             gxp_tx[:, 2 * hc:], gxp_bd),
            dict(apply_gelu=apply_gelu, negative_slope=slope, dropout_p=p, seed=seed_tb, keep_bits=ctx.bits[1]))
        r = lambda gt, ref: gt.reshape(ref.shape).to(ref.dtype) if ref is not None else None
        return (gxp_tx, gxp_bd, r(gatt_tt, att_tt), r(gbias_tt, bias_tt), r(gatt_tb, att_tb), r(gbias_tb, bias_tb),
                None, None, None, None, None, None, None, None, None, None, None, None)


def hetero_gat_layer(xp_tx, xp_bd, att_tt, bias_tt, att_tb, bias_tb, g_tt, g_tb, heads, channels, *,
                     apply_gelu=True, negative_slope=0.2, dropout_p=0.0, seed_tt=0, seed_tb=0, return_alpha=False,
                     bits_tt=None, bits_tb=None):
    """``bits_tt`` / ``bits_tb`` = (by_dst plane, by_src plane or None) of :func:`dropout_bits` for this layer."""
    return _HeteroGatLayer.apply(xp_tx, xp_bd, att_tt, bias_tt, att_tb, bias_tb, g_tt, g_tb, heads, channels,
                                 apply_gelu, negative_slope, dropout_p, seed_tt, seed_tb, return_alpha, bits_tt, bits_tb)
