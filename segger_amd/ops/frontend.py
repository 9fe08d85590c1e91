from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE
from ..graph import EdgeCSR
from .. import ops                # route switches: read as ops.NAME when called, never bound here
from ._common import _grad_rows, _rows, _seq, _tag_prenorm, _vendor_gemm
from .packs import f32_split_planes
from .linear import (_run_backward, backward_plan, linear_f32_split_supported, linear_supported, linear_wgrad_supported,
                     segment_rowsum)


# --------------------------------------------------------------------------
# Encoder front end / tail (fused row-wise kernels)
# --------------------------------------------------------------------------


class EmbedInput:
    """The transcripts' first-layer input ``gelu(cat(table[ids], pe))`` (ist_encoder.py:312-325) kept as its parts:
    ``table`` fp32 [G, D] (the gene embedding), ``ids`` int32 [n], ``act_pe`` = gelu(positional embedding) [n, D] in the
    compute dtype, ``by_gene`` = rows grouped by id.  :func:`embed_linear` projects it without materialising the
    concatenation.  ``pre_pe`` (optional): the positional embedding before its GELU when ``act_pe`` is a constant for
    autograd (``posmlp(return_pre=True)``): the projection's backward then returns d / d pre_pe."""

    def __init__(self, table: Tensor, ids: Tensor, act_pe: Tensor, by_gene: Optional[EdgeCSR],
                 pre_pe: Optional[Tensor] = None):
        self.table, self.ids, self.act_pe, self.by_gene, self.pre_pe = table, ids, act_pe, by_gene, pre_pe
        self.shape = (int(act_pe.shape[0]), int(table.shape[1]) + int(act_pe.shape[1]))
        self.dtype, self.device = act_pe.dtype, act_pe.device


class _RowBiasLinear(torch.autograd.Function):
    """y = c @ Wc^T + T[ids]  (``segger_linear_fwd_rowbias``).  Backward: dc = dY Wc, dWc = dY^T c (MFMA kernels),
    dT = rows of dY summed by id (``segger_segment_rowsum`` over the rows-by-gene grouping).  ``pre`` (optional):
    c = gelu(pre) is a constant and the data gradient is returned for ``pre``, gelu'(pre) applied in the kernel."""

    @staticmethod
    def forward(ctx, c, wc, tab, ids, by_gene, pre=None):
        lib = _lib.load()
        dev, dt = c.device, c.dtype
        n, k = c.shape
        m = wc.shape[0]
        w16 = wc.detach().to(dt).contiguous()
        tab16 = tab.detach().to(dt).contiguous()             # the table is added in fp32 but travels in the compute dtype
        y = torch.empty((n, m), dtype=dt, device=dev)
        cp, ldc = _rows(c, k, "c")
        with _lib.on_device(dev):
            rc = lib.segger_linear_fwd_rowbias(cp, ldc, w16.data_ptr(), None, tab16.data_ptr(), m, ids.data_ptr(),
                                               y.data_ptr(), m, n, k, m, DTYPE_CODE[dt], _lib.stream_ptr(dev))
        _lib.check(rc, "segger_linear_fwd_rowbias")
        ctx.save_for_backward(c, w16, pre)
        ctx.by_gene, ctx.ids, ctx.n_ids = by_gene, ids, int(tab.shape[0])
        return y

    @staticmethod
    def backward(ctx, gy):
        c, w16, pre = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy = _grad_rows(gy, c.dtype)
        m, k = w16.shape
        plan = backward_plan(m, k, c.shape[0], c.dtype, need[0] or (pre is not None and need[5]), need[1], False,
                             pre is not None, site="row_bias")
        gc, gw, _ = _run_backward(plan, gy, c, lambda form: w16.t().contiguous(), pre)      # (W^T: [n, M] @ Wc -> [n, K])
        gt = None
        if need[2]:
            by_gene = ctx.by_gene if ctx.by_gene is not None else rows_by_id(ctx.ids, ctx.n_ids)
            gt = segment_rowsum(gy, by_gene)
        if pre is not None:
            if gc is not None and not plan.gate:
                gc = torch.ops.aten.gelu_backward(gc, pre)
            return None, gw, gt, None, None, gc
        return gc, gw, gt, None, None, None


def embed_linear_supported(k: int, m_out: int, dtype: torch.dtype) -> bool:
    """The widths :func:`embed_linear` covers on the GPU: positional half ``k`` -> ``m_out`` (asked before any tensor exists)."""
    return (m_out % 4 == 0 and k in (64, 128) and linear_supported(k, m_out, dtype)
            and linear_supported(m_out, k, dtype) and linear_wgrad_supported(m_out, k, dtype))


def _gene_table_args(table, weights, biases, dt):
    a = _lib.GeneTableArgs()
    d = int(table.shape[1])
    a.table, a.n_genes, a.D, a.n_w, a.dtype = table.data_ptr(), int(table.shape[0]), d, len(weights), DTYPE_CODE[dt]
    for i, (w, b) in enumerate(zip(weights, biases)):
        if w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != 2 * d or w.stride(1) != 1:
            raise ValueError("embed_linear: weights must be fp32 [m, 2 D] with a dense last dimension")
        a.w[i], a.ld_w[i], a.m[i] = w.data_ptr(), int(w.stride(0)) if w.shape[0] > 1 else 2 * d, int(w.shape[0])
        if b is not None:
            if b.dtype != torch.float32 or not b.is_contiguous() or b.numel() != w.shape[0]:
                raise ValueError("embed_linear: biases must be contiguous fp32 [m]")
            a.b[i] = b.data_ptr()
    return a


class _EmbedLinear(torch.autograd.Function):
    """``linear(gelu(cat(table[ids], pe)), cat(weights), cat(biases))`` as ONE autograd node on hand-written kernels only:
    forward = ``segger_gene_table_fwd`` (the per-gene table T = gelu(E) Wa^T + b, and the positional half Wc / Wc^T of the
    weights in the compute dtype) + ``segger_linear_fwd_rowbias``; backward = the one-pass MFMA kernel (dc, dWc from one
    read of dY) + the by-gene row sum of dY + ``segger_gene_table_bwd`` (dE, both halves of every weight's gradient, the
    bias gradients).  Arguments: c = gelu(pre) [n, D] (compute dtype), pre (or None), table, ids, by_gene, n_w, then the n_w
    weights and the n_w biases (None allowed)."""

    @staticmethod
    def forward(ctx, c, pre, table, ids, by_gene, n_w, *wb):
        weights, biases = wb[:n_w], wb[n_w:]
        lib = _lib.load()
        dev, dt = c.device, c.dtype
        n, d = c.shape
        g = int(table.shape[0])
        m = sum(int(w.shape[0]) for w in weights)
        a = _gene_table_args(table, weights, biases, dt)
        tab = torch.empty((g, m), dtype=dt, device=dev)
        wc = torch.empty((m, d), dtype=dt, device=dev)
        wc_t = torch.empty((d, m), dtype=dt, device=dev)
        a.tab, a.ld_tab, a.wc, a.wc_t = tab.data_ptr(), m, wc.data_ptr(), wc_t.data_ptr()
        y = torch.empty((n, m), dtype=dt, device=dev)
        cp, ldc = _rows(c, d, "c")
        split = (ops.F32_SPLIT and dt == torch.float32 and ldc % 4 == 0 and linear_f32_split_supported(d, m))
        with _lib.on_device(dev):
            _lib.check(lib.segger_gene_table_fwd(C.byref(a), _lib.stream_ptr(dev)), "segger_gene_table_fwd")
            if split:      # fp32 storage: the positional GEMM on the bf16x3 split, the table row added in its epilogue
                w3 = f32_split_planes(wc)
                rc = lib.segger_linear_fwd_f32_split_rowbias(cp, ldc, w3.data_ptr(), tab.data_ptr(), m, ids.data_ptr(),
                                                             y.data_ptr(), m, n, d, m, _lib.stream_ptr(dev))
            else:
                rc = lib.segger_linear_fwd_rowbias(cp, ldc, wc.data_ptr(), None, tab.data_ptr(), m, ids.data_ptr(),
                                                   y.data_ptr(), m, n, d, m, DTYPE_CODE[dt], _lib.stream_ptr(dev))
        _lib.check(rc, "segger_linear_fwd_rowbias")
        ctx.save_for_backward(c, pre, table, ids, wc, wc_t, *weights)
        ctx.by_gene, ctx.n_w, ctx.has_bias = by_gene, n_w, tuple(b is not None for b in biases)
        return y

    @staticmethod
    def backward(ctx, gy):
        c, pre, table, ids, wc, wc_t = ctx.saved_tensors[:6]
        weights = ctx.saved_tensors[6:]
        n_w = ctx.n_w
        lib = _lib.load()
        dev, dt = c.device, c.dtype
        d = int(c.shape[1])
        m = int(wc.shape[0])
        gy = _grad_rows(gy, dt)
        need = ctx.needs_input_grad
        plan = backward_plan(m, d, c.shape[0], dt, need[0] or (pre is not None and need[1]), any(need[6:6 + n_w]), False,
                             pre is not None, need[1], gy.stride(0) % 4 == 0, site="first")
        gc, gw, _ = _run_backward(plan, gy, c, lambda form: wc_t if form == "wt" else f32_split_planes(wc, transposed=True),
                                  pre)
        by_gene = ctx.by_gene if ctx.by_gene is not None else rows_by_id(ids, int(table.shape[0]))
        gt = segment_rowsum(gy, by_gene)
        if gw is not None and lib.segger_reductions_pending() >= 0:
            # inside ops.deferred_reductions the weight gradient above is a placeholder until the flush: run what is queued
            # now (one launch) and go on deferring -- the launch below READS dWc
            with _lib.on_device(dev):
                _lib.check(lib.segger_reductions_flush(_lib.stream_ptr(dev)), "segger_reductions_flush")
                _lib.check(lib.segger_reductions_defer_begin(), "segger_reductions_defer_begin")
        biases = [None] * n_w
        a = _gene_table_args(table, weights, biases, dt)
        a.g_tab, a.g_wc = gt.data_ptr(), _lib.ptr(gw)
        g_table = torch.empty_like(table) if need[2] else None
        a.g_table = _lib.ptr(g_table)
        g_w, g_b = [], []
        for i, w in enumerate(weights):
            gwi = torch.empty((int(w.shape[0]), 2 * d), dtype=torch.float32, device=dev) if need[6 + i] else None
            gbi = (torch.empty(int(w.shape[0]), dtype=torch.float32, device=dev)
                   if ctx.has_bias[i] and need[6 + n_w + i] else None)
            a.g_w[i], a.g_b[i] = _lib.ptr(gwi), _lib.ptr(gbi)
            g_w.append(gwi); g_b.append(gbi)
        with _lib.on_device(dev):
            _lib.check(lib.segger_gene_table_bwd(C.byref(a), _lib.stream_ptr(dev)), "segger_gene_table_bwd")
        if pre is not None:
            if gc is not None and not plan.gate:
                gc = torch.ops.aten.gelu_backward(gc, pre)
            return (None, gc, g_table, None, None, None, *g_w, *g_b)
        return (gc, None, g_table, None, None, None, *g_w, *g_b)


def embed_linear(x: "EmbedInput", weight, bias) -> Tensor:
    """``linear(gelu(cat(table[ids], pe)), W, b)`` for the stacked first-layer projections without the concatenated
    [n, 2D] input: the embedding half depends on a row only through its gene, so it is a per-gene table
    ``T = gelu(table) Wa^T + b`` ([G, M], a tiny GEMM) added in the epilogue of the GEMM over the positional half
    (K: 2D -> D).  Autograd: T's gradient is the by-gene row sum of dY; table, Wa and b receive theirs through T."""
    weights, biases = _seq(weight), _seq(bias)
    d = int(x.table.shape[1])
    # (the table kernels are latency-sized: a few hundred genes.  A 5k-gene panel's dW reduction would take 0.6 ms on their
    #  24 workgroups -- the torch-composed route with its vendor GEMMs below serves those)
    if (ops.EMBED_LINEAR_ONE_NODE and len(weights) <= 4 and x.act_pe.shape[1] == d and x.table.shape[0] <= ops.EMBED_LINEAR_MAX_GENES
            and all(w.dtype == torch.float32 and w.dim() == 2 and w.shape[1] == 2 * d and w.stride(1) == 1 for w in weights)
            and all(b is None or (b.dtype == torch.float32 and b.is_contiguous()) for b in biases)):
        return _EmbedLinear.apply(x.act_pe, x.pre_pe, x.table, x.ids, x.by_gene, len(weights), *weights, *biases)
    w = weights[0] if len(weights) == 1 else torch.cat(weights, 0)                # [M, 2D] fp32 master weights
    _vendor_gemm("per-gene table T = gelu(E) Wa^T (torch-composed first layer)", d, w.shape[0], torch.float32)
    tab = torch.nn.functional.gelu(x.table) @ w[:, :d].t()                         # [G, M]
    if any(b is not None for b in biases):
        tab = tab + torch.cat([b if b is not None else ww.new_zeros(ww.shape[0]) for ww, b in zip(weights, biases)], 0)
    return _RowBiasLinear.apply(x.act_pe, w[:, d:], tab, x.ids, x.by_gene, x.pre_pe)


class _EmbedGelu(torch.autograd.Function):
    """gelu(cat(table[ids], pe)): table fp32 [G, D] (embedding weight), ids int32 [n], pe [n, D] -> [n, 2D]."""

    @staticmethod
    def forward(ctx, table, ids, pe, by_gene):
        _lib.require_cuda(table, ids, pe)
        lib = _lib.load()
        n, d = pe.shape
        g = table.shape[0]
        out = torch.empty((n, 2 * d), dtype=pe.dtype, device=pe.device)
        pp, ldp = _rows(pe, d, "pe")
        with _lib.on_device(pe.device):
            rc = lib.segger_embed_gelu_fwd(table.data_ptr(), ids.data_ptr(), pp, ldp, n, g, d, out.data_ptr(), 2 * d,
                                           DTYPE_CODE[pe.dtype], _lib.stream_ptr(pe.device))
        _lib.check(rc, "segger_embed_gelu_fwd")
        ctx.save_for_backward(table, ids, pe)
        ctx.by_gene = by_gene
        return out

    @staticmethod
    def backward(ctx, gx0):
        table, ids, pe = ctx.saved_tensors
        lib = _lib.load()
        dev = pe.device
        n, d = pe.shape
        g = table.shape[0]
        if gx0.dtype != pe.dtype:
            gx0 = gx0.to(pe.dtype)
        if gx0.stride(-1) != 1:
            gx0 = gx0.contiguous()
        gp, ldg = _rows(gx0, 2 * d, "gx0")
        pp, ldp = _rows(pe, d, "pe")
        gpe = torch.empty_like(pe)
        want_table = ctx.needs_input_grad[0]
        gtable = torch.empty_like(table) if want_table else None
        ws_bytes = lib.segger_embed_gelu_bwd_workspace_bytes(n, g, d) if want_table else 0
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        by_gene = ctx.by_gene
        if want_table and by_gene is None:
            by_gene = rows_by_id(ids, g)
        with _lib.on_device(dev):
            rc = lib.segger_embed_gelu_bwd(gp, ldg, table.data_ptr(), pp, ldp, n, g, d, gpe.data_ptr(), d, _lib.ptr(gtable),
                                           by_gene.indptr.data_ptr() if want_table else None,
                                           (by_gene.col.data_ptr() if n else None) if want_table else None,
                                           ws.data_ptr(), ws_bytes, DTYPE_CODE[pe.dtype], _lib.stream_ptr(dev))
        _lib.check(rc, "segger_embed_gelu_bwd")
        return gtable, None, gpe, None


class _FrontJoin(torch.autograd.Function):
    """(gelu(cat(table[ids], pe[:n_tx])), gelu(cat(xb, pe[n_tx:]))): the encoder's layer-0 input of both node types in one
    launch each way (``segger_front_join_fwd`` / ``_bwd``); ``pe`` = the positional embeddings of the two types back to
    back.  The backward returns the gradient of ``pe`` as one matrix."""

    @staticmethod
    def forward(ctx, table, ids, xb, pe, by_gene):
        _lib.require_cuda(table, ids, xb, pe)
        lib = _lib.load()
        n_tx, n_bd, d = int(ids.shape[0]), int(xb.shape[0]), int(pe.shape[1])
        dev, dt = pe.device, pe.dtype
        out_tx = torch.empty((n_tx, 2 * d), dtype=dt, device=dev)
        out_bd = torch.empty((n_bd, 2 * d), dtype=dt, device=dev)
        a = _lib.FrontJoinArgs()
        a.table, a.ids, a.n_rows_table, a.D, a.dtype = table.data_ptr(), _lib.ptr(ids) if n_tx else None, int(table.shape[0]), d, DTYPE_CODE[dt]
        a.pe, a.ld_pe = _rows(pe, d, "pe")
        a.n_tx, a.n_bd = n_tx, n_bd
        a.xb, a.ld_xb = _rows(xb, d, "xb")
        a.out_tx, a.ld_out_tx, a.out_bd, a.ld_out_bd = out_tx.data_ptr(), 2 * d, out_bd.data_ptr(), 2 * d
        with _lib.on_device(dev):
            rc = lib.segger_front_join_fwd(C.byref(a), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_front_join_fwd")
        ctx.save_for_backward(table, ids, xb, pe)
        ctx.by_gene = by_gene
        return out_tx, out_bd

    @staticmethod
    def backward(ctx, g_tx, g_bd):
        table, ids, xb, pe = ctx.saved_tensors
        lib = _lib.load()
        n_tx, n_bd, d = int(ids.shape[0]), int(xb.shape[0]), int(pe.shape[1])
        dev, dt = pe.device, pe.dtype

        def rows2(g, n):
            if g is None:
                g = torch.zeros((n, 2 * d), dtype=dt, device=dev)
            if g.dtype != dt:
                g = g.to(dt)
            if g.stride(-1) != 1:
                g = g.contiguous()
            return g
        g_tx, g_bd = rows2(g_tx, n_tx), rows2(g_bd, n_bd)
        g_pe = torch.empty((n_tx + n_bd, d), dtype=dt, device=dev)
        g_xb = torch.empty((n_bd, d), dtype=dt, device=dev)
        want_table = ctx.needs_input_grad[0]
        g_table = torch.empty_like(table) if want_table else None
        g = int(table.shape[0])
        ws_bytes = lib.segger_embed_gelu_bwd_workspace_bytes(n_tx, g, d) if want_table else 0
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        by_gene = ctx.by_gene
        if want_table and by_gene is None and n_tx:
            by_gene = rows_by_id(ids, g)
        a = _lib.FrontJoinArgs()
        a.table, a.ids, a.n_rows_table, a.D, a.dtype = table.data_ptr(), _lib.ptr(ids) if n_tx else None, g, d, DTYPE_CODE[dt]
        a.pe, a.ld_pe = _rows(pe, d, "pe")
        a.n_tx, a.n_bd = n_tx, n_bd
        a.xb, a.ld_xb = _rows(xb, d, "xb")
        a.g_tx, a.ld_g_tx = _rows(g_tx, 2 * d, "g_tx")
        a.g_bd, a.ld_g_bd = _rows(g_bd, 2 * d, "g_bd")
        a.g_pe, a.ld_g_pe, a.g_xb, a.ld_g_xb = g_pe.data_ptr(), d, g_xb.data_ptr(), d
        if want_table:
            a.g_table = g_table.data_ptr()
            if n_tx:
                a.gene_ptr, a.gene_rows = by_gene.indptr.data_ptr(), by_gene.col.data_ptr()
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        with _lib.on_device(dev):
            rc = lib.segger_front_join_bwd(C.byref(a), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_front_join_bwd")
        return g_table, None, g_xb, g_pe, None


def front_join(table: Tensor, ids: Tensor, xb: Tensor, pe: Tensor, by_gene: Optional[EdgeCSR] = None):
    """-> (x_tx [n_tx, 2D], x_bd [n_bd, 2D]) = (gelu(cat(table[ids], pe[:n_tx])), gelu(cat(xb, pe[n_tx:]))), reference
    ist_encoder.py:312-320 for both node types.  ``pe``: [n_tx + n_bd, D]; ``by_gene`` as :func:`embed_gelu`."""
    if table.dtype != torch.float32 or not table.is_contiguous():
        raise TypeError("front_join: the embedding table must be contiguous fp32")
    d = int(table.shape[1])
    if pe.shape[1] != d or xb.shape[1] != d or d % 8 or pe.shape[0] != ids.shape[0] + xb.shape[0] or xb.dtype != pe.dtype:
        raise ValueError("front_join: pe [n_tx + n_bd, D] and xb [n_bd, D] must match the table width and each other's dtype")
    return _FrontJoin.apply(table, ids.to(torch.int32).contiguous(), xb, pe, by_gene)


def rows_by_id(ids: Tensor, n_ids: int) -> EdgeCSR:
    """Rows grouped by id (``indptr`` over ids, ``col`` = row numbers, ascending inside an id): what the
    embedding-table gradient sums over.  One radix sort; cache it per batch (``ISTEncoder`` does)."""
    from ..graph import csr_from_coo
    n = int(ids.shape[0])
    return csr_from_coo(ids.long(), torch.arange(n, device=ids.device), int(n_ids), max(n, 1), validate=False)


def embed_gelu(table: Tensor, ids: Tensor, pe: Tensor, by_gene: Optional[EdgeCSR] = None) -> Tensor:
    """``by_gene`` = :func:`rows_by_id` of ``ids`` when the caller has it cached (built in backward otherwise)."""
    if table.dtype != torch.float32 or not table.is_contiguous():
        raise TypeError("embed_gelu: the embedding table must be contiguous fp32")
    if pe.shape[1] != table.shape[1] or pe.shape[1] % 32:
        raise ValueError("embed_gelu: pe width must equal the embedding width and be a multiple of 32")
    return _EmbedGelu.apply(table, ids.to(torch.int32).contiguous(), pe.contiguous(), by_gene)


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, eps):
        _lib.require_cuda(y)
        lib = _lib.load()
        n, c = y.shape
        z = torch.empty((n, c), dtype=y.dtype, device=y.device)
        yp, ldy = _rows(y, c, "y")
        with _lib.on_device(y.device):
            rc = lib.segger_l2norm_fwd(yp, ldy, n, c, eps, z.data_ptr(), c, DTYPE_CODE[y.dtype], _lib.stream_ptr(y.device))
        _lib.check(rc, "segger_l2norm_fwd")
        ctx.save_for_backward(y)
        ctx.eps = eps
        return z

    @staticmethod
    def backward(ctx, gz):
        (y,) = ctx.saved_tensors
        lib = _lib.load()
        n, c = y.shape
        if gz.dtype != y.dtype:
            gz = gz.to(y.dtype)
        if gz.stride(-1) != 1 or gz.dim() != 2:
            gz = gz.contiguous()
        gy = torch.empty((n, c), dtype=y.dtype, device=y.device)
        yp, ldy = _rows(y, c, "y")
        gp, ldg = _rows(gz, c, "gz")
        with _lib.on_device(y.device):
            rc = lib.segger_l2norm_bwd(yp, ldy, gp, ldg, n, c, ctx.eps, gy.data_ptr(), c, DTYPE_CODE[y.dtype],
                                       _lib.stream_ptr(y.device))
        _lib.check(rc, "segger_l2norm_bwd")
        return gy, None


class _L2NormMany(torch.autograd.Function):
    """Row normalisation of several matrices in ONE launch each way (``segger_l2norm_many``)."""

    @staticmethod
    def forward(ctx, eps, *ys):
        lib = _lib.load()
        c, dt, dev = int(ys[0].shape[1]), ys[0].dtype, ys[0].device
        zs = [torch.empty((int(y.shape[0]), c), dtype=dt, device=dev) for y in ys]
        segs = (_lib.L2NormSeg * len(ys))()
        for sg, y, z in zip(segs, ys, zs):
            sg.y, sg.ld_y = _rows(y, c, "y")
            sg.n, sg.out, sg.ld_out = int(y.shape[0]), z.data_ptr(), c
        with _lib.on_device(dev):
            rc = lib.segger_l2norm_many(segs, len(ys), c, eps, DTYPE_CODE[dt], _lib.stream_ptr(dev))
        _lib.check(rc, "segger_l2norm_many")
        ctx.save_for_backward(*ys)
        ctx.eps = eps
        return tuple(zs)

    @staticmethod
    def backward(ctx, *gzs):
        ys = ctx.saved_tensors
        lib = _lib.load()
        c, dt, dev = int(ys[0].shape[1]), ys[0].dtype, ys[0].device
        segs = (_lib.L2NormSeg * len(ys))()
        outs, keep, k = [], [], 0
        for y, gz in zip(ys, gzs):
            if gz is None:
                outs.append(None)
                continue
            if gz.dtype not in (dt, torch.float32):
                gz = gz.to(dt)
            if gz.dim() != 2 or (gz.shape[0] > 1 and gz.stride(1) != 1):
                gz = gz.contiguous()
            gy = torch.empty((int(y.shape[0]), c), dtype=dt, device=dev)
            sg = segs[k]; k += 1
            sg.y, sg.ld_y = _rows(y, c, "y")
            sg.n, sg.out, sg.ld_out = int(y.shape[0]), gy.data_ptr(), c
            sg.gz, sg.ld_gz = _rows(gz, c, "gz")
            sg.gz_f32 = int(gz.dtype == torch.float32 and dt != torch.float32)
            outs.append(gy); keep.append(gz)
        if k:
            with _lib.on_device(dev):
                rc = lib.segger_l2norm_many(segs, k, c, ctx.eps, DTYPE_CODE[dt], _lib.stream_ptr(dev))
            _lib.check(rc, "segger_l2norm_many")
        return (None,) + tuple(outs)


def l2_normalize_many(ys: dict, eps: float = 1e-12) -> dict:
    """``{k: F.normalize(v, dim=-1)}`` for up to four [n_k, C] matrices of one width and dtype in ONE launch (both node
    types of the encoder's tail, ist_encoder.py:331-332); anything else goes through :func:`l2_normalize` per entry."""
    vals = list(ys.values())
    if (1 < len(vals) <= 4 and all(v.dim() == 2 and v.is_cuda for v in vals) and vals[0].shape[1] in (8, 16, 32, 64, 128)
            and vals[0].dtype in DTYPE_CODE and all(v.shape[1] == vals[0].shape[1] and v.dtype == vals[0].dtype for v in vals)
            and all(v.shape[0] > 0 for v in vals)):
        zs = _L2NormMany.apply(float(eps), *vals)
        return {k: _tag_prenorm(z, y, eps) for k, y, z in zip(ys, vals, zs)}
    return {k: l2_normalize(v, eps) for k, v in ys.items()}


def l2_normalize(y: Tensor, eps: float = 1e-12) -> Tensor:
    """F.normalize(y, dim=-1) for [n, C] with C in {8,16,32,64,128}; other widths use torch."""
    if y.dim() == 2 and y.shape[1] in (8, 16, 32, 64, 128) and y.dtype in DTYPE_CODE:
        return _tag_prenorm(_L2Norm.apply(y, float(eps)), y, eps)
    _lib.require_cuda(y)
    return torch.nn.functional.normalize(y.float(), dim=-1, eps=eps).to(y.dtype)
