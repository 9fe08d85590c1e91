from __future__ import annotations

from collections import namedtuple
import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE
from ..graph import EdgeCSR
from .. import ops                # route switches: read as ops.NAME when called, never bound here
from ._common import _prenorm_of, _rows


# --------------------------------------------------------------------------
# Prediction head
# --------------------------------------------------------------------------
@torch.no_grad()
def edge_cos_argmax(by_src: EdgeCSR, z_src: Tensor, z_dst: Tensor, *, dst_index: Optional[Tensor] = None,
                    min_similarity: Optional[float] = None, eps: float = 1e-8, return_sim: bool = False):
    """-> (max_sim[f32 Ns], max_eid[i64 Ns], seg_idx[i64 Ns], sim[f32 E] | None)."""
    _lib.require_cuda(z_src, z_dst)
    lib = _lib.load()
    dev = z_src.device
    if z_src.dtype != z_dst.dtype or z_src.dtype not in DTYPE_CODE:
        raise TypeError("edge_cos_argmax: z_src / z_dst must share a supported dtype")
    c = int(z_src.shape[1])
    n = by_src.n_rows
    if z_src.shape[0] != n or z_dst.shape[0] != by_src.n_cols or z_dst.shape[1] != c:
        raise ValueError("edge_cos_argmax: embedding shapes do not match the graph")
    a = _lib.EdgeArgmaxArgs()
    a.by_src = by_src.c_struct()
    a.z_src, a.ld_zs = _rows(z_src, c, "z_src")
    a.z_dst, a.ld_zd = _rows(z_dst, c, "z_dst")
    a.channels, a.dtype, a.eps = c, DTYPE_CODE[z_src.dtype], eps
    a.use_min_similarity = int(min_similarity is not None)
    a.min_similarity = float(min_similarity) if min_similarity is not None else 0.0
    di = None
    if dst_index is not None:
        di = dst_index.to(device=dev, dtype=torch.int64).contiguous()
        if di.numel() != by_src.n_cols:
            raise ValueError("edge_cos_argmax: dst_index has the wrong length")
        a.dst_index = di.data_ptr()
    max_sim = torch.empty(n, dtype=torch.float32, device=dev)
    max_eid = torch.empty(n, dtype=torch.int64, device=dev)
    seg = torch.empty(n, dtype=torch.int64, device=dev)
    sim = torch.empty(by_src.n_edges, dtype=torch.float32, device=dev) if return_sim else None
    a.max_sim, a.max_eid, a.seg_idx, a.sim = max_sim.data_ptr(), max_eid.data_ptr(), seg.data_ptr(), _lib.ptr(sim)
    with _lib.on_device(dev):
        rc = lib.segger_edge_cos_argmax(C.byref(a), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_edge_cos_argmax")
    return max_sim, max_eid, seg, sim


# --------------------------------------------------------------------------
# Triplet margin loss over edges
# --------------------------------------------------------------------------
def _triplet_args(src, pos, neg, za, zb, margin, eps, kind: str = "triplet"):
    a = _lib.TripletArgs()
    a.loss_kind = _LOSS_KIND[kind]
    a.src, a.pos, a.neg, a.n_edges = src.data_ptr(), pos.data_ptr(), neg.data_ptr(), int(src.numel())
    c = int(za.shape[1])
    a.z_a, a.ld_za = _rows(za, c, "z_a")
    a.z_b, a.ld_zb = _rows(zb, c, "z_b")
    a.n_a, a.n_b = int(za.shape[0]), int(zb.shape[0])
    a.channels, a.dtype, a.margin, a.eps = c, DTYPE_CODE[za.dtype], margin, eps
    return a


def _triplet_grads(a, ga, gb, scale, a_packed=False, b_packed=False, pos_groups=None, anchor_unique=False) -> None:
    """The gradient side of a ``TripletArgs`` (``*_packed``: 16-bit atomics into a matrix of the embeddings' dtype)."""
    a.grad_a, a.grad_a_packed, a.grad_b, a.grad_b_packed = ga.data_ptr(), int(a_packed), gb.data_ptr(), int(b_packed)
    if pos_groups is not None:
        a.pos_indptr, a.pos_eid = pos_groups.indptr.data_ptr(), (pos_groups.eid.data_ptr() if pos_groups.n_edges else None)
        a.anchor_unique = int(anchor_unique)      # one walk over the groups: anchor rows stored, not added
    a.grad_scale, a.grad_scale_dev = 1.0, scale.data_ptr()


# ``anchors_unique`` is a bool, or a callable (``EdgeGraph.src_unique``) that may synchronise: asked in a backward only
_anchors_unique = lambda flag: bool(flag() if callable(flag) else flag)
# ... and the widths at which ``segger_triplet_bwd`` then takes the anchors in one walk over the groups
_one_walk_width = lambda c: c % 32 == 0 and c <= 128


class _TripletEdgeLoss(torch.autograd.Function):
    """``zb is None``: anchors, positives and negatives are rows of the same matrix ``za``
    (loss_tx); one gradient buffer receives all three contributions."""

    @staticmethod
    def forward(ctx, za, zb, src, pos, neg, margin, eps, pos_groups, anchors_unique=False, kind="triplet"):
        same = zb is None
        zb_ = za if same else zb
        _lib.require_cuda(za, zb_, src)
        lib = _lib.load()
        dev = za.device
        if za.dtype != zb_.dtype or za.dtype not in DTYPE_CODE:
            raise TypeError("triplet_edge_loss: z_a / z_b must share a supported dtype")
        src, pos, neg = (t.to(torch.int64).contiguous() for t in (src, pos, neg))
        a = _triplet_args(src, pos, neg, za, zb_, margin, eps, kind)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws_bytes = lib.segger_triplet_workspace_bytes(a.n_edges)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        a.loss, a.workspace, a.workspace_bytes = loss.data_ptr(), ws.data_ptr(), ws_bytes
        with _lib.on_device(dev):
            rc = lib.segger_triplet_fwd(C.byref(a), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_triplet_fwd")
        ctx.save_for_backward(za, zb_, src, pos, neg)
        ctx.cfg = (margin, eps, same)
        ctx.pos_groups, ctx.anchors_unique, ctx.kind = pos_groups, anchors_unique, kind
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        za, zb, src, pos, neg = ctx.saved_tensors
        margin, eps, same = ctx.cfg
        lib = _lib.load()
        dev = za.device
        a = _triplet_args(src, pos, neg, za, zb, margin, eps, ctx.kind)
        # anchor-matrix rows collect a handful of terms: packed 16-bit atomics straight into a gradient of the
        # embeddings' dtype; a separate (boundary) matrix sums dozens of terms per row and stays fp32
        # (small batches measured no gain from the packed variant: they keep fp32 atomics)
        packed = (za.dtype in (torch.bfloat16, torch.float16) and za.shape[1] % 2 == 0
                  and src.numel() >= ops._CONTRIB_MIN_EDGES)
        ga = torch.zeros(za.shape, dtype=za.dtype if packed else torch.float32, device=dev)
        pg = None if same else ctx.pos_groups
        uniq = False
        if same:
            gb = ga
        elif pg is not None:
            # boundary side: the positives -- a boundary's ~40 edges sit next to each other and would hammer one row
            # (0.58 ms of contended fp32 atomics at C2) -- are a segmented sum over the triplets grouped by positive
            # row (for tx-belongs-bd edges: the by-destination view the encoder already built), which also WRITES
            # every row of grad_b; the uniformly sampled negatives add themselves with (uncontended) fp32 atomics
            uniq = _anchors_unique(ctx.anchors_unique) and _one_walk_width(za.shape[1])
            gb = (torch.zeros if (uniq or ctx.kind == "bce") else torch.empty)(zb.shape, dtype=torch.float32, device=dev)
        else:
            gb = torch.zeros(zb.shape, dtype=torch.float32, device=dev)
        gs = g.detach().to(torch.float32).reshape(1).contiguous()   # upstream scalar stays on the device
        _triplet_grads(a, ga, gb, gs, packed, packed and same, pg, uniq)
        with _lib.on_device(dev):
            rc = lib.segger_triplet_bwd(C.byref(a), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_triplet_bwd")
        return ga.to(za.dtype), (None if same else gb.to(zb.dtype)), None, None, None, None, None, None, None, None


def triplet_edge_loss(za: Tensor, zb: Optional[Tensor], src: Tensor, pos: Tensor, neg: Tensor,
                      margin: float, eps: float = 1e-6, pos_groups: Optional[EdgeCSR] = None,
                      anchors_unique=False) -> Tensor:
    """mean_e max(||za[src]-zb[pos]+eps|| - ||za[src]-zb[neg]+eps|| + margin, 0).
    Pass ``zb=None`` (or ``zb is za``) when positives / negatives index the anchor matrix itself.
    ``pos_groups``: the triplets grouped by positive row (``indptr`` over rows of ``zb``, ``eid`` = triplet ids), e.g.
    the by-destination view of the edge store the triplets come from: the backward then needs no atomics for them.
    ``anchors_unique`` (bool, or a callable asked in the backward, e.g. ``EdgeGraph.src_unique``; with ``pos_groups``):
    no row of ``za`` anchors two triplets -- the backward is then one walk over the groups storing the anchors' rows."""
    if zb is za:
        zb = None
    if pos_groups is not None and (zb is None or pos_groups.n_rows != zb.shape[0] or pos_groups.n_edges != src.numel()):
        raise ValueError("triplet_edge_loss: pos_groups does not describe these triplets")
    return _TripletEdgeLoss.apply(za, zb, src, pos, neg, float(margin), float(eps), pos_groups, anchors_unique, "triplet")


def bce_edge_loss(za: Tensor, zb: Tensor, src: Tensor, pos: Tensor, neg: Tensor, pos_groups: Optional[EdgeCSR] = None,
                  anchors_unique=False) -> Tensor:
    """The BCE variant of the segmentation loss (reference lightning_model.py:190-207): ``BCEWithLogitsLoss`` over
    ``cat(<za[src], zb[pos]>, <za[src], zb[neg]>)`` with labels ``cat(1, 0)``, one kernel forward and one backward
    (``segger_triplet_fwd / _bwd`` with ``loss_kind = SEGGER_LOSS_BCE``).  ``pos_groups`` / ``anchors_unique`` as in
    :func:`triplet_edge_loss`."""
    if za.shape[1] % 2:
        raise ValueError("bce_edge_loss: even channel count")
    if pos_groups is not None and (pos_groups.n_rows != zb.shape[0] or pos_groups.n_edges != src.numel()):
        raise ValueError("bce_edge_loss: pos_groups does not describe these edges")
    return _TripletEdgeLoss.apply(za, zb, src, pos, neg, 0.0, 0.0, pos_groups, anchors_unique, "bce")


# The parts of a LossHeadSpec, as its docstring describes them (``pos_groups``: the segmentation triplets grouped by positive row)
TxTriplets = namedtuple("TxTriplets", "anchors pos neg margin eps")
BdMetric = namedtuple("BdMetric", "pos neg d_pos d_neg weight eps")
SgTriplets = namedtuple("SgTriplets", "src pos neg margin eps pos_groups anchors_unique", defaults=(None, False))
# their index tensors as the kernels read them (int64 / float32, contiguous; None: not there), saved last by every node
_Indices = namedtuple("_Indices", "bd_pos bd_neg bd_dpos bd_dneg bd_w tx_anchors tx_pos tx_neg sg_src sg_pos sg_neg",
                      defaults=(None,) * 6)
_LOSS_KIND = {"triplet": 0, "bce": 1}
_i64 = lambda t: t.to(torch.int64).contiguous()
_f32 = lambda t: t.to(torch.float32).contiguous()


def _metric_args(z: Tensor, idx: _Indices, eps: float, name: str = "z_bd") -> tuple:
    """The eleven leading arguments of ``segger_metric_fwd`` / ``_bwd``."""
    n, c = z.shape
    return (*_rows(z, c, name), n, c, DTYPE_CODE[z.dtype], idx.bd_pos.data_ptr(), idx.bd_neg.data_ptr(), idx.bd_dpos.data_ptr(),
            idx.bd_dneg.data_ptr(), idx.bd_w.data_ptr(), float(eps))


class _MetricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, pos, neg, d_pos, d_neg, w, eps):
        _lib.require_cuda(z, pos)
        lib = _lib.load()
        dev = z.device
        if z.dtype not in DTYPE_CODE:
            raise TypeError("metric_loss: unsupported embedding dtype")
        idx = _Indices(_i64(pos), _i64(neg), _f32(d_pos), _f32(d_neg), _f32(w))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.segger_triplet_workspace_bytes(z.shape[0]), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            rc = lib.segger_metric_fwd(*_metric_args(z, idx, eps, "z"), loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.stream_ptr(dev))
        _lib.check(rc, "segger_metric_fwd")
        ctx.save_for_backward(z, *idx)
        ctx.eps = eps
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        z, *idx = ctx.saved_tensors
        lib = _lib.load()
        dev = z.device
        gz = torch.zeros(z.shape, dtype=torch.float32, device=dev)
        gs = g.detach().to(torch.float32).reshape(1).contiguous()
        with _lib.on_device(dev):
            rc = lib.segger_metric_bwd(*_metric_args(z, _Indices(*idx), ctx.eps, "z"), gs.data_ptr(), gz.data_ptr(),
                                       _lib.stream_ptr(dev))
        _lib.check(rc, "segger_metric_bwd")
        return gz.to(z.dtype), None, None, None, None, None, None


def metric_loss(z: Tensor, pos: Tensor, neg: Tensor, d_pos: Tensor, d_neg: Tensor, w: Tensor, eps: float = 1e-8) -> Tensor:
    """sum_i w_i [(cos(z_i, z_pos_i) - (1 - d_pos_i))^2 + (cos(z_i, z_neg_i) - (1 - d_neg_i))^2]: MetricLoss
    (triplet_loss.py:176-204) on sampled triplets, one kernel forward and one backward; ``pos_i < 0`` skips node i."""
    return _MetricLoss.apply(z, pos, neg, d_pos, d_neg, w, float(eps))


class LossHeadSpec:
    """What :func:`loss_head` needs besides the embeddings.  ``tx`` = (anchors, positives, negatives, margin, eps) of
    loss_tx (rows of z_tx; ``-1`` = skip); ``bd`` = (positives, negatives, d_pos, d_neg, weights, eps) of loss_bd (rows
    of z_bd); ``sg`` = (src, pos, neg, margin, eps, pos_groups | None[, anchors_unique]) of the segmentation triplets, or
    None when the batch has at most one boundary (lightning_model.py:173-175: that loss is then 0).  ``anchors_unique``
    (bool, or a callable asked in the backward, e.g. ``EdgeGraph.src_unique``): no transcript is the anchor of two
    triplets -- the backward then walks the groups once and stores the anchors' gradient rows.  Plain tuples, or the
    named forms they are read as from here on (``TxTriplets``, ``BdMetric``, ``SgTriplets``)."""

    def __init__(self, tx, bd, sg, sg_kind: str = "triplet", tx_anchors_are_rows: bool = False, sg_of_tx=None,
                 tx_state: Optional[Tensor] = None, grad_out_hint: Optional[Tensor] = None, defer_finish: bool = False,
                 deterministic: bool = False):
        self.tx, self.bd, self.sg = TxTriplets(*tx), BdMetric(*bd), (None if sg is None else SgTriplets(*sg))
        self.sg_kind = sg_kind                                             # "bce": margin / eps unused
        # loss_tx's anchors are arange(n_tx) (possibly with -1 positives = skipped): lets the backward STORE the anchors'
        # gradient rows (loss_head, when z_tx comes straight out of ops.l2_normalize)
        self.tx_anchors_are_rows = bool(tx_anchors_are_rows)
        # one-launch loss head (segger_loss_head_fwd / _bwd): ``sg_of_tx`` int32 [n_tx] = the segmentation triplet anchored
        # at each transcript row (-1: none; :func:`anchor_index`), or a callable returning it; ``tx_state`` int32
        # [2 n_tx + 4] a buffer the caller has ALREADY zero-filled (a captured step does that in its staging launch);
        # ``grad_out_hint`` float32 [4]: the gradient the backward will receive (a training step: e_3) -- the forward then
        # leaves the three scale factors behind and the backward skips their launch when it is handed that very tensor
        self.sg_of_tx, self.tx_state, self.grad_out_hint = sg_of_tx, tx_state, grad_out_hint
        # one-launch head, with grad_out_hint: leave the finishing launch (the three means, the total) to the BACKWARD launch --
        # the returned loss tensor is then only valid once the backward has run (a captured training step reads it after the
        # replay); the caller promises that a backward with exactly the hinted gradient follows
        self.defer_finish = bool(defer_finish)
        # the ordered backward of the one-launch head (segger_loss_head_ordered_fwd / _bwd): every byte of the gradients and
        # the losses a function of the inputs alone, no float atomic; the routes through csrc/heads.hip's atomic kernels
        # ("anchor_rows", "kernel_by_kernel", and the atomic side launch of a transcript that anchors two segmentation
        # triplets) are refused with a NotImplementedError -- never silently non-deterministic
        self.deterministic = bool(deterministic)


def _indices(spec: LossHeadSpec, anchors: bool = True) -> _Indices:
    t, m, s = spec.tx, spec.bd, spec.sg
    return _Indices(_i64(m.pos), _i64(m.neg), _f32(m.d_pos), _f32(m.d_neg), _f32(m.weight),
                    _i64(t.anchors) if anchors else None, _i64(t.pos), _i64(t.neg),
                    *((None,) * 3 if s is None else (_i64(s.src), _i64(s.pos), _i64(s.neg))))


class _LossHead(torch.autograd.Function):
    """``LitISTEncoder.get_losses`` (lightning_model.py:151-213) after the sampling, as ONE autograd node:
    out = [a0 * loss_tx, a1 * loss_bd, a2 * loss_sg, sum_i b_i * out_i].  Forward: the three loss kernels write their
    means side by side and one launch combines them.  Backward: one launch turns the incoming gradient into the three
    scale factors (device scalars), then the three backward kernels accumulate into ONE gradient buffer per embedding
    matrix -- no per-loss zero fill, cast and add, and no chain of 0-dim torch ops around the weighted sum."""

    @staticmethod
    def forward(ctx, z_tx, z_bd, a, b, spec: LossHeadSpec, y_tx=None, eps_tx=0.0):
        # y_tx (optional): z_tx == l2_normalize(y_tx, eps_tx) is then a CONSTANT here and the gradient is returned for y_tx
        # (anchor rows stored + normalisation backward inside this node)
        _lib.require_cuda(z_tx, z_bd, a, b)
        lib = _lib.load()
        dev, dt = z_tx.device, z_tx.dtype
        if z_bd.dtype != dt or dt not in DTYPE_CODE:
            raise TypeError("loss_head: z_tx / z_bd must share a supported dtype")
        c = int(z_tx.shape[1])
        if z_bd.shape[1] != c:
            raise ValueError("loss_head: z_tx / z_bd must have the same width")
        a, b = _f32(a.detach()), _f32(b.detach())
        idx, sg = _indices(spec), spec.sg
        nb = int(z_bd.shape[0])
        keep = []
        stream = _lib.stream_ptr(dev)
        parts = (C.c_void_p * 3)()
        counts = (C.c_int64 * 3)(0, 0, 0)
        scales = (C.c_float * 3)(0.0, 0.0, 0.0)

        def triplet_partials(k, src, pos, neg, t, zb, kind):       # loss k: per-block partial sums only, and their scale
            ta = _triplet_args(src, pos, neg, z_tx, zb, float(t.margin), float(t.eps), kind)
            ws = torch.empty(lib.segger_triplet_workspace_bytes(ta.n_edges), dtype=torch.uint8, device=dev)
            ta.loss, ta.workspace, ta.workspace_bytes = None, ws.data_ptr(), ws.numel()
            _lib.check(lib.segger_triplet_fwd(C.byref(ta), stream), "segger_triplet_fwd")
            keep.append(ws)
            if ta.n_edges:
                parts[k], counts[k] = ws.data_ptr(), lib.segger_triplet_partial_count(ta.n_edges)
                scales[k] = (0.5 if kind == "bce" else 1.0) / ta.n_edges

        with _lib.on_device(dev):
            triplet_partials(0, idx.tx_anchors, idx.tx_pos, idx.tx_neg, spec.tx, z_tx, "triplet")
            ws = torch.empty(lib.segger_triplet_workspace_bytes(nb), dtype=torch.uint8, device=dev)
            _lib.check(lib.segger_metric_fwd(*_metric_args(z_bd, idx, spec.bd.eps), None, ws.data_ptr(), ws.numel(), stream),
                       "segger_metric_fwd")
            keep.append(ws)
            if nb:
                parts[1], counts[1], scales[1] = ws.data_ptr(), lib.segger_triplet_partial_count(nb), 1.0
            if sg is not None:
                if sg.pos_groups is not None and (sg.pos_groups.n_rows != nb or sg.pos_groups.n_edges != idx.sg_src.numel()):
                    raise ValueError("loss_head: pos_groups does not describe the segmentation triplets")
                triplet_partials(2, idx.sg_src, idx.sg_pos, idx.sg_neg, sg, z_bd, spec.sg_kind)
            out = torch.empty(4, dtype=torch.float32, device=dev)
            # the three means from their per-block partial sums and the weighted total: one launch
            _lib.check(lib.segger_loss_combine_partials_fwd(parts, counts, scales, a.data_ptr(), b.data_ptr(), 3,
                                                            out.data_ptr(), stream), "segger_loss_combine_partials_fwd")
        ctx.keep = keep                                      # (the partial sums are read by the launch above)
        ctx.save_for_backward(z_tx, z_bd, a, b, *idx)
        ctx.spec, ctx.y_tx, ctx.eps_tx = spec, y_tx, float(eps_tx)
        return out

    @staticmethod
    def backward(ctx, g_out):
        z_tx, z_bd, a, b, *idx = ctx.saved_tensors
        idx, spec, tx, sg = _Indices(*idx), ctx.spec, ctx.spec.tx, ctx.spec.sg
        lib = _lib.load()
        dev, dt = z_tx.device, z_tx.dtype
        c = int(z_tx.shape[1])
        g_out = g_out.detach().to(torch.float32).contiguous()
        graw = torch.empty(3, dtype=torch.float32, device=dev)
        # transcript rows collect a handful of terms (once as anchor of either loss, ~2 as positive / negative): packed
        # 16-bit atomics straight into a gradient of the embeddings' dtype on large batches; boundary rows sum dozens
        # of terms and stay fp32 (+ one cast)
        packed = dt in (torch.bfloat16, torch.float16) and c % 2 == 0 and idx.tx_anchors.numel() >= ops._CONTRIB_MIN_EDGES
        y_tx = ctx.y_tx
        pg = sg.pos_groups if sg is not None else None
        uniq = pg is not None and _one_walk_width(c) and _anchors_unique(sg.anchors_unique)
        gb_written = pg is not None and not uniq and spec.sg_kind != "bce"       # (the two-kernel route writes every row)
        # both gradient matrices out of ONE zero-filled buffer (one fill launch instead of two)
        ga_dt = dt if packed else torch.float32
        na = z_tx.numel() * (2 if packed else 4)
        na = (na + 255) // 256 * 256
        nbb = 0 if gb_written else z_bd.numel() * 4
        zbuf = torch.zeros(na + nbb, dtype=torch.uint8, device=dev)
        ga = zbuf[:z_tx.numel() * (2 if packed else 4)].view(ga_dt).view(z_tx.shape)
        gb = (torch.empty(z_bd.shape, dtype=torch.float32, device=dev) if gb_written
              else zbuf[na:].view(torch.float32).view(z_bd.shape))
        ga_rows = torch.empty_like(ga) if y_tx is not None else None      # every row written by loss_tx's kernel
        stream = _lib.stream_ptr(dev)
        with _lib.on_device(dev):
            _lib.check(lib.segger_loss_combine_bwd(g_out.data_ptr(), a.data_ptr(), b.data_ptr(), 3, graw.data_ptr(), stream),
                       "segger_loss_combine_bwd")
            if sg is not None:          # first: with pos_groups its positive side WRITES every row of gb
                sa = _triplet_args(idx.sg_src, idx.sg_pos, idx.sg_neg, z_tx, z_bd, float(sg.margin), float(sg.eps), spec.sg_kind)
                _triplet_grads(sa, ga, gb, graw[2:3], packed, False, pg, uniq)
                _lib.check(lib.segger_triplet_bwd(C.byref(sa), stream), "segger_triplet_bwd")
            _lib.check(lib.segger_metric_bwd(*_metric_args(z_bd, idx, spec.bd.eps), graw[1:2].data_ptr(), gb.data_ptr(), stream),
                       "segger_metric_bwd")
            ta = _triplet_args(idx.tx_anchors, idx.tx_pos, idx.tx_neg, z_tx, z_tx, float(tx.margin), float(tx.eps))
            _triplet_grads(ta, ga, ga, graw[0:1], packed, packed)
            if ga_rows is not None:
                ta.grad_a_rows = ga_rows.data_ptr()
            _lib.check(lib.segger_triplet_bwd(C.byref(ta), stream), "segger_triplet_bwd")
            if ga_rows is not None:
                # d loss / d y_tx = normalisation backward of (ga + ga_rows), read as two matrices
                g1, g2 = (ga, ga_rows) if ga.dtype == dt else (ga.to(dt), ga_rows.to(dt))
                gy = torch.empty_like(y_tx)
                yp, ldy = _rows(y_tx, c, "y_tx")
                _lib.check(lib.segger_l2norm_bwd2(yp, ldy, g1.data_ptr(), c, g2.data_ptr(), c, int(y_tx.shape[0]), c, ctx.eps_tx,
                                                  gy.data_ptr(), c, DTYPE_CODE[dt], stream), "segger_l2norm_bwd2")
                return None, gb.to(dt), None, None, None, gy, None
        return (ga if packed else ga.to(dt)), gb.to(dt), None, None, None, None, None


_TICKETS: dict = {}


def _ticket(dev) -> Tensor:
    """The zero-initialised int32 the one-launch loss head counts finished blocks in (every launch leaves it zero);
    one per device, never freed: captured graphs hold its address."""
    t = _TICKETS.get(dev)
    if t is None:
        t = _TICKETS[dev] = torch.zeros(16, dtype=torch.int32, device=dev)
    return t


@torch.no_grad()
def anchor_index(src: Tensor, n_rows: int) -> Tensor:
    """int32 [n_rows]: position in ``src`` of each row (-1: the row is not in ``src``).  For the tx-belongs-bd edge list
    (every transcript at most once, heterodata.py:147) this is "the segmentation triplet anchored at transcript r"."""
    inv = torch.full((int(n_rows),), -1, dtype=torch.int32, device=src.device)
    if src.numel():
        inv[src.long()] = torch.arange(src.numel(), dtype=torch.int32, device=src.device)
    return inv


def loss_head_fused_supported(z_tx: Tensor, z_bd: Tensor, spec: "LossHeadSpec") -> bool:
    n, c = int(z_tx.shape[0]), int(z_tx.shape[1])
    return (ops.ONE_LAUNCH_LOSS_HEAD and spec.tx_anchors_are_rows and z_tx.dtype in DTYPE_CODE and z_tx.dtype == z_bd.dtype
            and bool(_lib.load().segger_loss_head_supported(c, DTYPE_CODE[z_tx.dtype])) and int(z_bd.shape[1]) == c
            and 0 < n <= ops.LOSS_HEAD_ONE_LAUNCH_MAX_ROWS and spec.tx.anchors.numel() == n and z_bd.shape[0] > 0
            and (spec.sg is None or spec.sg.pos_groups is not None))


# what the one-launch forward hands its backward besides the saved tensors (``out`` / ``ws``: a deferred finish completes them)
_FusedState = namedtuple("_FusedState", "tx_w head nxt gbd graw hot_acc out ws hint deferred")


def _loss_head_args(z_tx, z_bd, a, b, idx: _Indices, spec: LossHeadSpec, graw, ws, st: Optional[_FusedState]):
    """The fields of ``segger_loss_head_args`` that the forward and the backward launch share (``st`` None: a forward that
    nobody differentiates, without the backward's buffers); each direction adds its own."""
    tx, sg = spec.tx, spec.sg
    n_tx, c = int(z_tx.shape[0]), int(z_tx.shape[1])
    g = _lib.LossHeadArgs()
    g.z_tx, g.ld_ztx = _rows(z_tx, c, "z_tx")
    g.z_bd, g.ld_zbd = _rows(z_bd, c, "z_bd")
    g.n_tx, g.n_bd, g.channels, g.dtype = n_tx, int(z_bd.shape[0]), c, DTYPE_CODE[z_tx.dtype]
    g.tx_pos, g.tx_neg, g.tx_margin, g.tx_eps = idx.tx_pos.data_ptr(), idx.tx_neg.data_ptr(), float(tx.margin), float(tx.eps)
    g.bd_pos, g.bd_neg, g.bd_dpos, g.bd_dneg = (t.data_ptr() for t in (idx.bd_pos, idx.bd_neg, idx.bd_dpos, idx.bd_dneg))
    g.bd_w, g.bd_eps = idx.bd_w.data_ptr(), float(spec.bd.eps)
    g.sg_kind = _LOSS_KIND[spec.sg_kind]
    if sg is not None and idx.sg_src.numel():
        g.sg_src, g.sg_pos, g.sg_neg = idx.sg_src.data_ptr(), idx.sg_pos.data_ptr(), idx.sg_neg.data_ptr()
        g.n_sg = int(idx.sg_src.numel())
        g.sg_margin, g.sg_eps = float(sg.margin), float(sg.eps)
    g.a, g.b, g.grad_raw = a.data_ptr(), b.data_ptr(), graw.data_ptr()
    g.workspace, g.workspace_bytes, g.ticket = ws.data_ptr(), ws.numel(), _ticket(z_tx.device).data_ptr()
    if st is not None:
        g.tx_w, g.grad_bd = st.tx_w.data_ptr(), st.gbd.data_ptr()
        if st.head is not None:                      # (the ordered route keeps no chains and no hot rows)
            g.tx_state, g.tx_next = st.head.data_ptr(), st.nxt.data_ptr()
            g.tx_hot_id, g.tx_hot_acc = st.nxt[2 * n_tx:].data_ptr(), st.hot_acc.data_ptr()
    return g


class _LossHeadFused(torch.autograd.Function):
    """``LitISTEncoder.get_losses`` after the sampling as ONE launch forward and ONE backward (``segger_loss_head_fwd`` /
    ``_bwd``, csrc/loss_head.hip).  ``t_tx`` / ``t_bd`` carry the gradient: the embeddings themselves, or -- with
    ``z_tx`` / ``z_bd`` given as constants -- the matrices they were normalised from (``z = t / max(|t|, eps)``): the
    transcript side's normalisation backward then happens inside the launch, the boundary side's in a second, tiny one
    that reads the fp32 gradient directly.  No float atomic touches the transcript matrix (rows are gathered, not
    scattered), nothing is zero-filled by a launch of its own."""

    @staticmethod
    def forward(ctx, t_tx, t_bd, a, b, spec: LossHeadSpec, z_tx=None, z_bd=None, eps_tx=0.0, eps_bd=0.0):
        prenorm = z_tx is not None
        if not prenorm:
            z_tx, z_bd = t_tx, t_bd
        _lib.require_cuda(z_tx, z_bd, a, b)
        lib = _lib.load()
        dev = z_tx.device
        n_tx, c = int(z_tx.shape[0]), int(z_tx.shape[1])
        n_bd = int(z_bd.shape[0])
        need = any(ctx.needs_input_grad[:2])
        a, b = _f32(a.detach()), _f32(b.detach())
        idx = _indices(spec, anchors=False)          # (the anchors are the rows themselves)
        n_sg = int(idx.sg_src.numel()) if idx.sg_src is not None else 0
        out = torch.empty(4, dtype=torch.float32, device=dev)
        graw = torch.empty(3, dtype=torch.float32, device=dev)
        ordered = spec.deterministic
        if ordered and n_sg and not callable(spec.sg.anchors_unique) and not spec.sg.anchors_unique:
            raise NotImplementedError(_REFUSED % "the atomic side launch (segger_triplet_bwd) of segmentation triplets whose "
                                                 "anchors are not unique")
        ws_bytes = (lib.segger_loss_head_ordered_workspace_bytes if ordered else lib.segger_loss_head_workspace_bytes)
        ws = torch.empty(ws_bytes(n_tx, n_bd, n_sg), dtype=torch.uint8, device=dev)
        st = None
        if need:
            tx_w = torch.empty((n_tx, 2), dtype=torch.float32, device=dev)
            head = nxt = hot_acc = None                      # (the ordered route: no chains, no hot rows; tx_state unused)
            if not ordered:
                head = spec.tx_state
                if head is None:
                    head = torch.zeros(2 * n_tx + 4, dtype=torch.int32, device=dev)
                elif head.dtype != torch.int32 or head.numel() < 2 * n_tx + 4 or not head.is_contiguous():
                    raise ValueError("loss_head: tx_state must be a contiguous int32 [2 n_tx + 4] tensor (zero-filled)")
                n_hot = int(lib.segger_loss_head_max_hot_rows(n_tx))
                nxt = torch.empty(2 * n_tx + n_tx + n_hot, dtype=torch.int32, device=dev)    # chain links | hot ids + arrivals
                hot_acc = torch.empty((n_hot, c), dtype=torch.float32, device=dev)
            gbd = torch.empty((n_bd, c), dtype=torch.float32, device=dev)
            hint = spec.grad_out_hint
            if hint is not None:
                hint = hint.detach()
                if hint.dtype != torch.float32 or hint.numel() != 4 or not hint.is_contiguous() or hint.device != dev:
                    raise ValueError("loss_head: grad_out_hint must be a contiguous float32 [4] tensor on the embeddings' device")
            st = _FusedState(tx_w, head, nxt, gbd, graw, hot_acc, out, ws, hint, bool(hint is not None and spec.defer_finish))
        g = _loss_head_args(z_tx, z_bd, a, b, idx, spec, graw, ws, st)
        g.out = out.data_ptr()
        if st is not None and st.hint is not None:
            g.grad_out, g.reserved_ = st.hint.data_ptr(), (_lib.LOSS_HEAD_DEFER_FINISH if st.deferred else 0)
        with _lib.on_device(dev):
            rc = (lib.segger_loss_head_ordered_fwd if ordered else lib.segger_loss_head_fwd)(C.byref(g), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_loss_head_ordered_fwd" if ordered else "segger_loss_head_fwd")
        if need:
            ctx.save_for_backward(t_tx, t_bd, z_tx, z_bd, a, b, *idx)
            ctx.spec, ctx.state, ctx.prenorm, ctx.eps = spec, st, prenorm, (float(eps_tx), float(eps_bd))
        return out

    @staticmethod
    def backward(ctx, g_out):
        t_tx, t_bd, z_tx, z_bd, a, b, *idx = ctx.saved_tensors
        idx, spec, st, sg = _Indices(*idx), ctx.spec, ctx.state, ctx.spec.sg
        lib = _lib.load()
        dev, dt = z_tx.device, z_tx.dtype
        n_tx, c = int(z_tx.shape[0]), int(z_tx.shape[1])
        n_bd = int(z_bd.shape[0])
        ordered = spec.deterministic
        if getattr(ctx, "_ran", False) and not ordered:             # (the ordered route writes every row: nothing to re-arm)
            # a second backward over the same graph (retain_graph=True): the forward launch zero-filled the boundary
            # gradient and armed the hot rows' accumulators / arrival counters ONCE -- re-arm them, or this pass would add
            # on top of the first one's sums and never finish a hot row
            st.gbd.zero_()
            st.hot_acc.zero_()
            st.nxt[3 * n_tx:].zero_()
        ctx._ran = True
        stream = _lib.stream_ptr(dev)
        g_out = g_out.detach().to(torch.float32).contiguous()
        hinted = st.hint is not None and g_out.data_ptr() == st.hint.data_ptr()
        # the segmentation triplets' anchor terms ride in the row walk when no transcript anchors two of them
        n_sg = int(idx.sg_src.numel()) if sg is not None else 0
        uniq, of_tx = False, None
        if n_sg:
            uniq = _anchors_unique(sg.anchors_unique)
            if ordered and not uniq:
                raise NotImplementedError(_REFUSED % "the atomic side launch (segger_triplet_bwd) of segmentation triplets "
                                                     "whose anchors are not unique")
            if uniq:
                of_tx = spec.sg_of_tx() if callable(spec.sg_of_tx) else spec.sg_of_tx
                if of_tx is None:
                    of_tx = anchor_index(idx.sg_src, n_tx)
                if of_tx.dtype != torch.int32 or of_tx.numel() < n_tx or not of_tx.is_contiguous():
                    raise ValueError("loss_head: sg_of_tx must be a contiguous int32 [n_tx] tensor")
            pg = sg.pos_groups
            if pg.n_rows != n_bd or pg.n_edges != n_sg:
                raise ValueError("loss_head: pos_groups does not describe the segmentation triplets")
        fuse_norm = ctx.prenorm and (not n_sg or uniq)
        out_dummy = torch.empty(4, dtype=torch.float32, device=dev)
        if st.deferred and not hinted:
            raise RuntimeError("loss_head: defer_finish promised a backward with the hinted gradient")
        # (the ordered route's workspace holds the forward's sorted keys: always the forward's own)
        ws = st.ws if st.deferred or ordered else torch.empty(lib.segger_loss_head_workspace_bytes(n_tx, n_bd, n_sg),
                                                              dtype=torch.uint8, device=dev)
        g = _loss_head_args(z_tx, z_bd, a, b, idx, spec, st.graw, ws, st)
        g.out = out_dummy.data_ptr()
        if st.deferred:
            # the forward left only its per-block partial sums: this launch finishes the losses (into the forward's output)
            g.out, g.grad_out, g.reserved_ = st.out.data_ptr(), st.hint.data_ptr(), _lib.LOSS_HEAD_DEFER_FINISH
        if n_sg:
            g.sg_pos_indptr, g.sg_pos_eid = pg.indptr.data_ptr(), (pg.eid.data_ptr() if pg.n_edges else None)
            g.sg_of_tx = _lib.ptr(of_tx)
        gtx = torch.empty((n_tx, c), dtype=dt, device=dev)
        g.grad_tx, g.ld_gtx = gtx.data_ptr(), c
        if fuse_norm:
            g.y_tx, g.ld_ytx = _rows(t_tx, c, "y_tx")
            g.norm_eps = ctx.eps[0]
        with _lib.on_device(dev):
            if not hinted:                                                       # (else the forward left the factors behind)
                _lib.check(lib.segger_loss_combine_bwd(g_out.data_ptr(), a.data_ptr(), b.data_ptr(), 3, st.graw.data_ptr(),
                                                       stream), "segger_loss_combine_bwd")
            if ordered:
                _lib.check(lib.segger_loss_head_ordered_bwd(C.byref(g), stream), "segger_loss_head_ordered_bwd")
            else:
                _lib.check(lib.segger_loss_head_bwd(C.byref(g), stream), "segger_loss_head_bwd")
            if n_sg and not uniq:
                # a transcript anchors two segmentation triplets (never in segger's data): their anchor terms by atomics
                # on top of the rows just written, the boundary side having been done by the launch above
                sa = _triplet_args(idx.sg_src, idx.sg_pos, idx.sg_neg, z_tx, z_bd, float(sg.margin), float(sg.eps), spec.sg_kind)
                scratch = torch.zeros((n_bd, c), dtype=torch.float32, device=dev)      # (its boundary side is discarded)
                _triplet_grads(sa, gtx, scratch, st.graw[2:3], dt != torch.float32)
                _lib.check(lib.segger_triplet_bwd(C.byref(sa), stream), "segger_triplet_bwd")
            if ctx.prenorm:
                # boundary side (and, in the rare case above, the transcript side) through the normalisation's backward
                gy_bd = torch.empty((n_bd, c), dtype=dt, device=dev)
                todo = [(t_bd, "y_bd", gy_bd, st.gbd, 1)]
                if not fuse_norm:
                    gz_tx, gtx = gtx, torch.empty((n_tx, c), dtype=dt, device=dev)
                    todo.append((t_tx, "y_tx", gtx, gz_tx, 0))
                segs = (_lib.L2NormSeg * 2)()
                for seg, (y, name, gy, gz, gz_f32) in zip(segs, todo):
                    seg.y, seg.ld_y = _rows(y, c, name)
                    seg.n, seg.out, seg.ld_out = int(y.shape[0]), gy.data_ptr(), c
                    seg.gz, seg.ld_gz, seg.gz_f32 = gz.data_ptr(), c, gz_f32
                # (the two eps are the same number in the encoder; the launch takes one)
                _lib.check(lib.segger_l2norm_many(segs, len(todo), c, ctx.eps[1], DTYPE_CODE[dt], stream), "segger_l2norm_many")
                return gtx, gy_bd, None, None, None, None, None, None, None
        return gtx, st.gbd.to(dt), None, None, None, None, None, None, None


_REFUSED = ("loss_head: deterministic=True is not implemented on the route through %s: its kernels (csrc/heads.hip) add "
            "with float atomics, whose order varies from run to run; only the one-launch head has an ordered backward")


def loss_head_route(z_tx: Tensor, z_bd: Tensor, spec: LossHeadSpec) -> str:
    """-> "one_launch_prenorm" | "one_launch" | "anchor_rows" | "kernel_by_kernel": the route :func:`loss_head` takes.
    With ``spec.deterministic`` the two one-launch routes run the ordered backward and the other two are refused."""
    pt = _prenorm_of(z_tx)
    if loss_head_fused_supported(z_tx, z_bd, spec):
        pb = _prenorm_of(z_bd)
        ok = lambda z, p: (p is not None and p[0].requires_grad and p[0].shape == z.shape and p[0].dtype == z.dtype)
        if torch.is_grad_enabled() and ok(z_tx, pt) and ok(z_bd, pb) and pt[1] == pb[1]:
            # both embeddings come straight out of the row normalisation: they are constants here and the gradient goes
            # to its inputs (the transcript side's normalisation backward inside the launch)
            return "one_launch_prenorm"
        return "one_launch"
    # (fp32 storage only: there loss_tx's backward is bound by 12 fp32 atomic instructions per triplet, a third of them the
    # anchor's -- 1.19 -> 0.8 ms at C2; with 16-bit embeddings the packed atomics are cheap enough that the second matrix
    # the normalisation backward then reads costs what the stores save: 13.40 vs 13.42 ms per step)
    if (ops.USE_ANCHOR_ROWS and z_tx.dtype == torch.float32
            and spec.tx_anchors_are_rows and pt is not None and pt[0].requires_grad and torch.is_grad_enabled()
            and z_tx.shape[1] % 8 == 0 and pt[0].shape == z_tx.shape and pt[0].dtype == z_tx.dtype
            and spec.tx.anchors.numel() == z_tx.shape[0]):
        # z_tx is the output of ops.l2_normalize: treat it as a constant and send the gradient to its input -- the anchors'
        # rows are then stored, not added atomically, and the normalisation backward reads the two matrices
        return "anchor_rows"
    return "kernel_by_kernel"


def loss_head(z_tx: Tensor, z_bd: Tensor, a: Tensor, b: Tensor, spec: LossHeadSpec) -> Tensor:
    """-> float32[4] = (a0 * loss_tx, a1 * loss_bd, a2 * loss_sg, sum_i b_i * (the three)): the three losses of
    ``LitISTEncoder.get_losses`` and their weighted sum as one autograd node (see :class:`_LossHead`).  ``a`` / ``b``:
    float32[3] on the device."""
    route = loss_head_route(z_tx, z_bd, spec)
    if spec.deterministic and route in ("anchor_rows", "kernel_by_kernel"):
        raise NotImplementedError(_REFUSED % f'"{route}" (the separate triplet, metric and loss_sg launches)')
    if route == "one_launch_prenorm":
        (y_tx, eps_tx), (y_bd, eps_bd) = _prenorm_of(z_tx), _prenorm_of(z_bd)
        return _LossHeadFused.apply(y_tx, y_bd, a, b, spec, z_tx.detach(), z_bd.detach(), eps_tx, eps_bd)
    if route == "anchor_rows":
        return _LossHead.apply(z_tx.detach(), z_bd, a, b, spec, *_prenorm_of(z_tx))
    return (_LossHeadFused if route == "one_launch" else _LossHead).apply(z_tx, z_bd, a, b, spec)
