"""One whole training step -- encoder forward, the three losses, backward, Adam -- as a single hipGraph replay.

At segger's default batch budget (``edges_per_batch = 1 000 000``, reference ``data/data_module.py:158``) a step is
under 2 ms of device work; eager, the host needs ~4 ms to queue its ~280 launches (50M-transcript FOV, one MI355X:
4.2 ms per step eager, 1.8 ms replayed).  Everything in the step is free
of host synchronisation and of data-dependent shapes (masks are weights, not compactions; samplers are kernels; the
dropout / sampling streams read DEVICE counters), so the step is captured ONCE per shape bucket and replayed for every
batch padded into the bucket's static buffers:

* nodes are padded with copies of node 0 (positions included: per-graph min / max unchanged; dummy transcripts carry
  the last gene id, so the rows-by-gene grouping of the embedding gradient only grows at its end), masked out of the
  losses (the samplers put them in the cluster nobody draws from);
* padding edges touch dummy nodes only and are laid out so that the CSR views need no sort: tx-neighbors-tx pads with
  self-loops on the dummies (identical by-destination and by-source views); tx-belongs-bd pads run from the dummy
  transcripts (round robin) to the dummy boundaries.  No loss term reads a dummy row, so every gradient that reaches a
  dummy is exactly zero: the one-pass tx-belongs-bd backward, which WRITES one source row per edge, may see a dummy
  source twice -- both writes store zero -- and the weight gradients, which sum over all rows, are untouched;
* the real part of every view is copied from the batch's own CSR (sliced from the slide-level sort by
  ``tiles.TilePartition``), the padding part is index arithmetic; real edges keep their COO positions, so the
  attention-dropout masks of real edges are the ones the eager step would draw;
* loss means are rescaled from padded to real counts on the device; padded triplets carry ``-1`` and are skipped by the
  kernels; negatives are drawn in ``[0, n_bd_real)``.

What it computes is ``LitISTEncoder.training_step`` + ``optimizer.step()`` (reference lightning_model.py:151-231 with
Lightning's automatic optimisation), for the default ``sg_loss_type='triplet'``.  The optimizer must be capturable
(``LitISTEncoder.configure_optimizers(capturable=True)``); ``ops.invalidate_weights(params)`` is called after every
replay because the parameters change without Python noticing.  The capture runs inside ``ops.pack_scope(aliases)``: the
weight refresh baked into the graph touches only the compute-dtype copies of THIS step's parameter aliases, which the
step keeps alive (``_pack_refs``), never another model's.

Data parallelism (``GraphedTrainer(..., grad_bucket=dp.FlatGradBucket(...))``): the step is captured as TWO graphs --
forward + backward + the packing of the gradients into the bucket's persistent flat buffer, and Adam reading that
buffer's slices -- with the gradient exchange between them run eagerly: one all-reduce + one divide per step on every
rank, whatever a rank is capturing; a rank that ran out of batches zeroes the buffer instead of replaying the first
graph.  Covered by a two-rank gloo test on one GPU; not yet run over RCCL on a multi-GPU box.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch
from torch import Tensor

from . import capture as cap, ops      # (`capture` is also an argument name here)
from .graph import EdgeCSR, EdgeGraph, batch_cache, edge_graph, graph_capture, padded_view_segments
from .hetero import TX_BD, TX_TX
from .ist_encoder import StagedInputs, rows_by_gene
from .triplet_loss import loss_inputs, masked_count

_EDGES = {"e_tt": TX_TX, "e_tb": TX_BD}                       # size key -> edge type


def step_bucket(batch, granularity: float = 1.06, floor: int = 256) -> Dict[str, int]:
    """Bucket sizes for one batch: counts rounded up to the next power of ``granularity`` (> the count: every node type
    keeps at least one dummy).  The boundary-side counts are a small part of the work and get one granule of headroom
    more, so that batches which agree on the transcript side share a bucket."""
    c = cap.counts(batch, _EDGES)
    up = lambda key, extra=0: cap.ladder(c[key], granularity, floor, extra)
    return {"tx": up("tx"), "bd": up("bd", 1), "e_tt": up("e_tt"), "e_tb": up("e_tb", 1), "graphs": up("graphs", 1)}


USE_ADAM_KERNEL = True       # (False: torch's fused Adam inside the captured step -- A/B switch)
MERGED_DRAWS = True          # (False: dropout planes, both samplers and the negatives as launches of their own, the dropout
                             #  counter advanced at the head of the step, Adam's step counters by a launch of their own)
DEFER_LOSS_FINISH = True     # (False: the one-launch loss head's finishing launch right behind its forward)
STEP_INC = 256               # what a training forward advances the encoder's dropout counter by (ist_encoder.py)


class StepEnd(NamedTuple):
    """What ``_run_grads`` leaves to the end of the step (``_opt_step``)."""
    counter_inc: int = 0          # the dropout-counter advance a merged-draws step read ahead of
    adam_advanced: bool = False   # Adam's step counters already moved (in the draws launch)


DYNAMIC_LOSS_SCALE = dict(init_scale=65536.0, growth=2.0, backoff=0.5, growth_interval=2000)   # torch.amp.GradScaler's defaults


def guard_config(clip_grad_norm=None, loss_scale=None, skip_nonfinite: bool = False) -> Optional[dict]:
    """The gradient guard a step was asked for -- ``ops.grad_guard``'s keyword arguments + ``init_scale`` -- or None when
    all three are off.  ``clip_grad_norm``: the maximal global L2 norm; ``loss_scale``: a float (static) or "dynamic";
    ``skip_nonfinite`` alone: scale 1, no clipping, only the skip."""
    if clip_grad_norm is None and loss_scale is None and not skip_nonfinite:
        return None
    cfg = dict(max_norm=0.0, init_scale=1.0, growth=2.0, backoff=0.5, growth_interval=0)
    if clip_grad_norm is not None:
        cfg["max_norm"] = float(clip_grad_norm)
        if not (0.0 < cfg["max_norm"] < float("inf")):
            raise ValueError(f"clip_grad_norm must be positive and finite, not {clip_grad_norm!r}")
    if isinstance(loss_scale, str):
        if loss_scale != "dynamic":
            raise ValueError(f'loss_scale is a float, "dynamic" or None, not {loss_scale!r}')
        cfg.update(DYNAMIC_LOSS_SCALE)
    elif loss_scale is not None:
        cfg["init_scale"] = float(loss_scale)
        if not (0.0 < cfg["init_scale"] < float("inf")):
            raise ValueError(f"loss_scale must be positive and finite, not {loss_scale!r}")
    return cfg


def make_guard(cfg: Optional[dict], optimizer, device):
    """The ``ops.GuardState`` of a guarded step; an optimizer the Adam kernel does not cover is refused HERE, with the
    reason: torch's own ``optimizer.step()`` inside the capture would silently drop the guard."""
    if cfg is None:
        return None
    if not USE_ADAM_KERNEL or ops.adam_hyper(optimizer) is None:
        raise RuntimeError("clip_grad_norm / loss_scale / skip_nonfinite are applied by the hand-written Adam kernel "
                           "(segger_adam_step_guarded), which does not cover this optimizer: it takes one parameter group "
                           "of a plain capturable torch.optim.Adam (no amsgrad / weight decay / maximize, a Python float "
                           "learning rate)" + ("" if USE_ADAM_KERNEL else "; USE_ADAM_KERNEL is off"))
    return ops.GuardState(device, cfg["init_scale"])


def accumulation_config(accumulate_grad_batches, optimizer, exchange) -> int:
    """``accumulate_grad_batches`` checked against what the captured step can do with it -> the window length N.  N == 1 is
    the step as it always was.  N > 1 is refused, with the reason, under data parallelism (when the collective runs
    relative to the window is a design of its own) and for an optimizer the Adam kernel does not cover (torch's own
    ``optimizer.step()`` inside the capture cannot be predicated on "the window closes now")."""
    n = ops.accumulate_batches(accumulate_grad_batches)
    if n == 1:
        return n
    if exchange.split:
        raise NotImplementedError("accumulate_grad_batches > 1 together with grad_sync / grad_bucket (data parallelism): when "
                                  "the gradient exchange runs relative to the accumulation window is not designed yet")
    if not USE_ADAM_KERNEL or ops.adam_hyper(optimizer) is None:
        raise NotImplementedError("accumulate_grad_batches > 1 closes its window inside the hand-written Adam kernel "
                                  "(segger_adam_step_windowed), which does not cover this optimizer: it takes one parameter "
                                  "group of a plain capturable torch.optim.Adam (no amsgrad / weight decay / maximize, a "
                                  "Python float learning rate)" + ("" if USE_ADAM_KERNEL else "; USE_ADAM_KERNEL is off"))
    return n


class GraphedTrainStep:
    """The captured step of ONE shape bucket (see :class:`GraphedTrainer` for the per-batch dispatch).  A batch is
    written into the bucket's static buffers by ONE launch (``ops.stage`` -> ``segger_stage``): node features, the three
    CSR views, the rows-by-gene grouping of the embedding gradient, the segmentation triplets and the loss samplers'
    indices are all "copy the batch's own (cached) arrays, fill the padding by a formula" segments.

    ``clip_grad_norm`` / ``loss_scale`` / ``skip_nonfinite`` (see :func:`guard_config`; all off by default, and the step
    then issues exactly the launches it always did): a gradient guard between the backward and Adam, on the device --
    the backward is seeded with the loss scale read from ``guard.scale`` (the forward and the returned losses are
    unscaled), ``ops.grad_guard`` decides clip factor / skip / next scale, the guarded Adam applies them.  ``guard``: the
    ``ops.GuardState`` to share (a :class:`GraphedTrainer` hands all its buckets one).

    ``deterministic`` (off by default, and the step then issues exactly the launches it always did): the loss head takes
    its ordered backward (``ops.LossHeadSpec(deterministic=True)``) -- the one place of a step where float atomics landed
    in a varying order -- so that the same seed and the same batches give the same bytes: parameters, Adam state, losses
    and the guard's state.  The warm-up's comparison of deferred against immediate sums then demands equal bytes.

    ``accumulate_grad_batches`` = N (1 by default, and the step then issues exactly the launches it always did; see
    :class:`GraphedTrainer` for the semantics): every step is a MICRO-step.  Behind the backward one launch
    (``ops.grad_accumulate``) adds the gradients, times 1 / N, into the fp32 accumulators of ``window`` (the
    ``ops.GradWindow`` to share: a trainer hands all its buckets one) -- overwriting them when the device-side window
    counter says this is the window's first micro-step -- and moves the counter on; the guard and Adam then read the
    ACCUMULATORS and act only when that launch closed the window.  The same graph serves every position of the window;
    Adam's step counters move in Adam's own counter launch (``adam_counters=False``, as in split mode), never at the head
    of the step."""

    def __init__(self, lit_model, optimizer, sizes: Dict[str, int], template, grad_sync=None, grad_bucket=None,
                 clip_grad_norm: Optional[float] = None, loss_scale=None, skip_nonfinite: bool = False, guard=None,
                 deterministic: bool = False, accumulate_grad_batches: int = 1, window=None):
        self.guard_cfg = guard_config(clip_grad_norm, loss_scale, skip_nonfinite)
        self.deterministic = bool(deterministic)
        self.exchange = cap.exchange_of(grad_sync, grad_bucket)
        self.accumulate_grad_batches = accumulation_config(accumulate_grad_batches, optimizer, self.exchange)
        self.split = self.exchange.split
        if self.exchange.bucket is not None:
            self.exchange.bucket._ensure()                    # the flat buffer must exist before anything is captured
        if lit_model.loss_tx is None or lit_model.loss_bd is None:
            raise RuntimeError("call setup() (or set_similarities) before training")
        if not all(g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError("the optimizer must keep its step counters on the device: "
                             "LitISTEncoder.configure_optimizers(capturable=True)")
        self.lit, self.opt, self.sizes = lit_model, optimizer, dict(sizes)
        dev = next(lit_model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("GraphedTrainStep needs the model on a GPU (hipGraph capture)")
        self.dev = dev
        for sel in (lit_model.loss_tx.selector, lit_model.loss_bd.selector):      # no host -> device copy in a capture
            sel.similarity, sel.dissimilarity = sel.similarity.to(dev), sel.dissimilarity.to(dev)
        nt, nb, ett, etb = sizes["tx"], sizes["bd"], sizes["e_tt"], sizes["e_tb"]
        z = cap.zeros_on(dev)
        i32, i64 = torch.int32, torch.int64
        self.n_genes = int(lit_model.model.lin_first["tx"].weight.shape[0])
        # positions / graph ids of both node types back to back: the encoder runs its positional embedder once over
        # the concatenation (boundary graph ids offset by the bucket's graph count), staged here without a launch
        self.pos_all, self.batch_all = z(nt + nb, 2), z(nt + nb, dtype=i64)
        # per-graph min / max of the positions (both node types: 2 * graphs rows): re-armed with +inf / -inf by the staging
        # launch of every step, so that the captured forward needs only the accumulating kernel (ops.segment_minmax)
        self.minmax = (z(2 * sizes["graphs"], 2), z(2 * sizes["graphs"], 2))
        self.nodes = {"tx": {"x": z(nt, dtype=i32), "pos": self.pos_all[:nt], "batch": self.batch_all[:nt]},
                      # boundary features staged in the compute dtype (the cast of ist_encoder.py's `x_dict['bd'].to(dt)` is
                      # made once per tile set and kept with it, not once per step)
                      "bd": {"x": z(nb, *template["bd"]["x"].shape[1:], dtype=self._bd_dtype(lit_model, template)),
                             "pos": self.pos_all[nt:], "batch": z(nb, dtype=i64)}}

        csr = lambda n_rows, n_cols, n_edges: cap.static_csr(n_rows, n_cols, n_edges, dev)
        self.g_tt = EdgeGraph(csr(nt, nt, ett), csr(nt, nt, ett), nt, nt, ett)
        self.g_tb = EdgeGraph(csr(nb, nt, etb), None, nt, nb, etb, None, True)        # one-pass backward (see above)
        by_gene_col = z(nt, dtype=i32)
        self.by_gene = EdgeCSR(z(self.n_genes + 1, dtype=i64), by_gene_col, by_gene_col, self.n_genes, nt)
        self.sg_src, self.sg_pos = z(etb, dtype=i64), z(etb, dtype=i64)
        # one-launch loss head: the segmentation triplet anchored at each transcript row (-1: none) and the rows'
        # contribution chains (heads + counts), zero-filled by the staging launch of every step
        self.sg_of_tx, self.tx_state = z(nt, dtype=i32), z(2 * nt + 4, dtype=i32)

        def sampler_index(selector, n):
            k = int(selector.similarity.shape[0])
            return dict(lab=z(n, dtype=i64), members=z(n, dtype=i64), counts=z(k + 1, dtype=i64),
                        offsets=z(k + 1, dtype=i64), cdf_pos_t=z(k, k), cdf_neg_t=z(k, k),
                        dists=(1.0 - selector.similarity).contiguous(), n_clusters=k)
        self.ix_tx = sampler_index(lit_model.loss_tx.selector, nt)
        self.ix_bd = sampler_index(lit_model.loss_bd.selector, nb)
        self.bd_weight = z(nb)
        self.n_bd = z(1, dtype=i64)                           # real boundary count of the staged batch
        # padded -> masked means (padded rows / masked tx count, 1, e_tb_pad / e_tb_real or 0 for <= 1 boundary), loss weights
        self.scal = z(6)
        self.head_a = self.scal[0:3]
        # Adam's (lr, beta1, beta2, eps) as the kernel reads them at replay time (segger_adam_step_dev), staged with every
        # batch from the optimizer's param_group: a learning-rate schedule is followed without a new capture
        self.hyper = z(4, dtype=torch.float64)
        self._hyper_on_device = USE_ADAM_KERNEL and ops.adam_hyper(optimizer) is not None
        self._e_loss = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)          # d / d out of out[3], the total loss
        # (guarded: [3] is overwritten with the loss scale at the head of every step, by a device-side copy)
        self.guard = (guard if guard is not None else make_guard(self.guard_cfg, optimizer, dev)) if self.guard_cfg else None
        self.out: Optional[Tensor] = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.graph_opt: Optional[torch.cuda.CUDAGraph] = None      # split mode (grad_sync): Adam as a graph of its own
        self.graph_flush: Optional[torch.cuda.CUDAGraph] = None    # accumulation: the close-only sequence (flush)
        self._grads: list = []
        self._training: Optional[bool] = None
        self._iota = torch.arange(nt, device=dev)
        self._captured_hp = None
        # The captured forward runs on ALIASES of the parameters (same storage, distinct autograd leaves).  A leaf's
        # gradient sink (its AccumulateGrad node) belongs to the stream it was created on and lives as long as any
        # autograd graph mentions it: after an eager step whose loss the caller still holds, the parameters' own
        # sinks sit on the default stream and would pull that stream into the capture (hipStreamEndCapture then
        # crashes).  The aliases' sinks are born inside the capture; the gradients are handed to the optimizer's
        # parameters by assignment.
        lit_model.model._materialize_bd(int(template["bd"]["x"].shape[1]), dev)
        self._alias = {n: ops.alias_of(p) for n, p in lit_model.model.named_parameters()}
        by_id = {id(p): self._alias[n] for n, p in lit_model.model.named_parameters()}
        self._params = [p for g in optimizer.param_groups for p in g["params"] if p.requires_grad and id(p) in by_id]
        self._leaves = [by_id[id(p)] for p in self._params]
        self.window = None                                    # accumulation: the shared window + accumulators
        if self.accumulate_grad_batches > 1:
            if window is not None and window.n != self.accumulate_grad_batches:
                raise ValueError(f"the shared window sums {window.n} micro-steps, this step was asked for {self.accumulate_grad_batches}")
            self.window = window if window is not None else ops.GradWindow(self._params, self.accumulate_grad_batches)
            self.window.ensure(self._params)                  # (allocated HERE, never inside a capture)
        self.draws = None                                     # tests: fixed (tx pos/neg, bd pos/neg/dp/dn, dst_neg)
        # queue the backward's partial sums and run them as one launch (ops.deferred_reductions).  Only sound when no
        # autograd node READS a parameter gradient before the backward ends (a parameter used by two nodes has its two
        # gradients added on the spot): verified numerically during the warm-up of every capture, see _warm_up, which
        # settles this for the runs that follow
        # (deterministic: the queued and the immediate sums add in two fixed but DIFFERENT orders -- conv.att's gradient differs
        # by an ulp -- so the warm-up's byte comparison could never pass: the sums are launched where they are produced,
        # without the warm-up's second run)
        self.defer_sums = not self.deterministic

    @staticmethod
    def _bd_dtype(lit_model, template):
        dt, src = lit_model.model.compute_dtype, template["bd"]["x"].dtype
        return dt if (src.is_floating_point and dt in (torch.bfloat16, torch.float16)) else src

    def fits(self, batch) -> bool:
        return cap.fits(self.sizes, batch, _EDGES)

    def waste(self, batch) -> float:
        """Padded / real size of the transcript side (what a step costs)."""
        return cap.waste(self.sizes, batch, _EDGES, "e_tt")

    # ------------------------------------------------------------------------------------------- staging
    def _sampler_segments(self, dst: dict, ix: dict, n_total: int) -> list:
        n = int(ix["lab"].numel())
        return [(dst["lab"], ix["lab"], "const", dst["n_clusters"], 0, 0),          # padding: the masked-out cluster
                (dst["members"], ix["members"], "div", n, 1, 0),
                (dst["counts"], ix["counts"], "const", 0, 0, 0), (dst["offsets"], ix["offsets"], "const", 0, 0, 0),
                (dst["cdf_pos_t"], ix["cdf_pos_t"], "const", 0, 0, 0), (dst["cdf_neg_t"], ix["cdf_neg_t"], "const", 0, 0, 0)]

    @torch.no_grad()
    def stage(self, batch) -> None:
        if not self.fits(batch):
            raise ValueError("batch does not fit this bucket")
        lit, s = self.lit, self.sizes
        tx, bd = batch["tx"], batch["bd"]
        n_tx, n_bd, nt = tx.num_nodes, bd.num_nodes, s["tx"]
        cache = batch_cache(batch)
        store = cache.get("persistent")
        g_tt = edge_graph(cache, TX_TX, batch[TX_TX].edge_index, n_tx, n_tx, need_by_src=True, validate="deferred")
        g_tb = edge_graph(cache, TX_BD, batch[TX_BD].edge_index, n_tx, n_bd, need_by_src="lazy", validate="deferred")
        if not g_tb.src_unique():
            raise NotImplementedError("a transcript with two tx-belongs-bd edges (heterodata.py:147 assigns one)")
        e_tb = g_tb.n_edges
        # what depends on the tile set only (kept across epochs by tiles.TilePartition; per batch object otherwise)
        keep = store if store is not None else cache
        ix_tx, ix_bd, _, of_tx = loss_inputs(lit.loss_tx, lit.loss_bd, batch, cache)
        a0 = ("rows_over_masked", nt)                         # loss_tx: mean over the padded rows -> mean over the masked real ones
        if a0 not in ix_tx:
            ix_tx[a0] = (float(nt) / masked_count(ix_tx["mask"])).reshape(1)
        by_gene = rows_by_gene(tx["x"], self.n_genes, cache)
        ei = batch[TX_BD].edge_index
        w = lit._scheduled_weights(lit._w_start, lit._w_end)
        bd_x, x_dt = bd["x"], self.nodes["bd"]["x"].dtype
        if bd_x.dtype != x_dt:
            key = ("bd_x", x_dt)
            hit = keep.get(key)
            if hit is None or hit.shape != bd_x.shape:
                hit = keep[key] = bd_x.to(x_dt).contiguous()
            bd_x = hit
        fb = ops.float_bits
        dummies = ("mod", n_tx, nt - n_tx)                    # dummy transcripts, round robin
        # nodes: dummies are copies of node 0 (gene id: the last gene, whose rows-by-gene group they extend)
        segs = cap.node_segments(self.nodes, tx, bd, self.n_genes - 1, bd_x) + [
            (self.batch_all[nt:], bd["batch"], "tile", 1, 0, 0, s["graphs"]),
            (self.by_gene.indptr, by_gene.indptr[: self.n_genes], "const", nt, 0, 0),
            (self.by_gene.col, by_gene.col, "div", n_tx, 1, 0),
            # segmentation triplets: padded ones carry -1 and are skipped by the kernels
            (self.sg_src, ei[0], *dummies, 0), (self.sg_pos, ei[1], "const", -1, 0, 0),
            (self.sg_of_tx, of_tx(), "const", -1, 0, 0), (self.tx_state, None, "const", 0, 0, 0),
            (self.bd_weight, ix_bd["weight"], "const", 0, 0, 0),
            (self.n_bd, None, "const", n_bd, 0, 0),
            (self.minmax[0], None, "const", fb(float("inf")), 0, 0), (self.minmax[1], None, "const", fb(float("-inf")), 0, 0),
            (self.scal[0:1], ix_tx[a0], "const", 0, 0, 0), (self.scal[1:2], None, "const", fb(1.0), 0, 0),
            (self.scal[2:3], None, "const", fb(s["e_tb"] / max(e_tb, 1) if n_bd > 1 else 0.0), 0, 0),   # :173-175
            (self.scal[3:4], None, "const", fb(w[0]), 0, 0), (self.scal[4:5], None, "const", fb(w[1]), 0, 0),
            (self.scal[5:6], None, "const", fb(w[2]), 0, 0),
        ]
        if self._hyper_on_device:
            hp = ops.adam_hyper(self.opt)
            if hp is None:
                raise RuntimeError("the optimizer's learning rate became a tensor / its groups changed after the capture")
            segs += [(self.hyper[i:i + 1], None, "const", ops.double_bits(v), 0, 0) for i, v in enumerate(hp)]
        segs += padded_view_segments(self.g_tt.by_dst, g_tt.by_dst, n_tx, None)
        segs += padded_view_segments(self.g_tt.by_src, g_tt.require_by_src(), n_tx, None)
        segs += padded_view_segments(self.g_tb.by_dst, g_tb.by_dst, n_bd, dummies)
        segs += self._sampler_segments(self.ix_tx, ix_tx, nt)
        segs += self._sampler_segments(self.ix_bd, ix_bd, s["bd"])
        ops.stage(segs, self.dev)

    # ------------------------------------------------------------------------------------------- the step
    def _run(self, warm: bool = False) -> None:
        accumulate = self.window is not None and not warm     # (a warm-up is rolled back: it must not touch the window)
        end = self._run_grads(self.defer_sums, adam_counters=not warm and not self.split and not accumulate, warm=warm)
        if accumulate:
            ops.grad_accumulate(self._params, self.window)    # acc (+)= grad / N, the window moves on; .grad = acc from here
        self._opt_step(end, warm=warm)

    def _opt_step(self, end: StepEnd, warm: bool = False) -> None:
        """Adam on the hand-written kernel (two launches for all tensors -- one when the step's first launch advanced the
        step counters; torch's fused multi-tensor Adam takes three and ~40 us for the encoder's 60 small tensors); any other
        optimizer steps itself.  The dropout counter a merged-draws step read un-advanced moves on here.  Guarded (not in
        a warm-up, which is rolled back and must not touch the guard's state): ``ops.grad_guard`` (two launches), then the
        guarded Adam; a skipped step's counters are taken back by the guard when the draws launch advanced them."""
        inc, adv = end
        enc = self.lit.model
        window = None if warm else self.window
        if (self.guard is not None or window is not None) and not warm:
            self._guarded_update(window, enc._step_dev if inc else None, inc, adv)
            return
        if USE_ADAM_KERNEL and ops.adam_step(self.opt, steps_advanced=adv, counter=enc._step_dev if inc else None,
                                             counter_inc=inc, hyper_dev=self.hyper if self._hyper_on_device else None):
            return
        if adv:
            raise RuntimeError("the step advanced Adam's counters for segger_adam_step, which then refused the optimizer")
        if self._hyper_on_device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("segger_adam_step refused an optimizer whose hyper-parameters this step stages on the "
                                   "device (non-fp32 / non-contiguous parameters or gradients, an AMP grad scaler attached)")
            # eager warm-up, optimizer state present, and the kernel still declines (what adam_hyper() cannot see from the
            # param_group: gradient dtype / layout, a GradScaler's grad_scale / found_inf): take the route that works from
            # here on -- torch's own step inside the capture, (lr, betas, eps) baked in and part of the re-capture key
            if any(self.opt.state.get(p) for g in self.opt.param_groups for p in g["params"]):
                self._hyper_on_device = False
        self.opt.step()
        if inc:
            ops.step_advance(enc._step_dev, inc)

    def _guarded_update(self, window, counter, inc: int, adv: bool) -> None:
        """The guard (when there is one) and Adam, both on the device's word: skipped on a non-finite gradient; inside an
        accumulation window (``window``: ``.grad`` is the accumulator) without effect until the window closes."""
        ops.adam_init_state(self.opt)                         # (an eager first step: nothing has created the state yet)
        if self.guard is not None:
            c = self.guard_cfg
            ops.grad_guard(self.opt, self.guard, max_norm=c["max_norm"], growth=c["growth"], backoff=c["backoff"],
                           growth_interval=c["growth_interval"], steps_advanced=adv, window=window)
        done = ops.adam_step(self.opt, steps_advanced=adv, counter=counter, counter_inc=inc, hyper_dev=self.hyper,
                             guard=self.guard, window=window)
        if not done:                                          # (guarded: adam_step raises itself)
            raise NotImplementedError("accumulate_grad_batches > 1: segger_adam_step_windowed declined this optimizer "
                                      "(non-fp32 / non-contiguous parameters or state, an AMP grad scaler attached), and "
                                      "torch's own optimizer.step() cannot wait for the window to close")

    def flush(self) -> None:
        """Close an open accumulation window early: guard, then Adam on the sum so far (every term still weighted 1 / N),
        then an empty window -- decided on the device, so with nothing open nothing changes.  Replayed from a graph of its
        own (Adam alone, as the empty step of split mode) once this bucket has captured its step; eager before that."""
        w = self.window
        if w is None:
            return
        for p in self._params:                                # (an eager warm-up of another bucket may have left raw gradients)
            if p.grad is not None:
                p.grad = w.acc(p)
        if all(p.grad is None for p in self._params):
            return                                            # no step ever ran: nothing is open

        def close_only():
            ops.window_flush(w, 0)
            self._guarded_update(w, None, 0, False)
            ops.window_flush(w, 1)
        if self.graph is None:
            close_only()
        else:
            if self.graph_flush is None:
                self.graph_flush = torch.cuda.CUDAGraph()
                with graph_capture(self.graph_flush, pool=self.graph.pool()):
                    close_only()
            self.graph_flush.replay()
        self._params_changed()

    def _run_grads(self, defer_sums: bool, adam_counters: bool, warm: bool = True) -> StepEnd:
        """Forward, losses, backward; ``.grad`` of the parameters and ``self.out`` set.  ``defer_sums``: see __init__.
        ``adam_counters``: the draws launch may advance Adam's step counters -- not in a warm-up, which ends in
        ``optimizer.step()``, and not in split mode, whose empty steps replay Adam's graph without this one.
        ``warm``: a warm-up's backward is seeded with 1 whatever the guard's loss scale is (its gradients are compared
        and thrown away; an overflow at the initial dynamic scale is the guard's business, not the warm-up's)."""
        lit, enc, s = self.lit, self.lit.model, self.sizes
        if self.guard is not None:
            with torch.no_grad():                             # the backward's seed: the loss scale as the device holds it NOW
                if warm:
                    self._e_loss[3:4].fill_(1.0)
                else:
                    self._e_loss[3:4].copy_(self.guard.scale.reshape(1))
        nt = s["tx"]
        tx, bd = self.nodes["tx"], self.nodes["bd"]
        graphs = {TX_TX: self.g_tt, TX_BD: self.g_tb}
        staged = StagedInputs(self.by_gene, self.pos_all, self.batch_all, self.minmax)
        fixed = self.draws
        drawn = None
        end = StepEnd()
        if MERGED_DRAWS and fixed is None:
            # ALL of the step's random draws in its first launch (ops.step_draws), from the dropout counter as it stands + the
            # advance it receives at the END of the step (inside Adam's launch): the same masks and triplets as advancing
            # first.  Adam's step counters move in the same launch (nothing reads them before the update).
            inc = STEP_INC if enc.training else 0
            views = enc.plane_views(graphs, seed_offset=inc) if enc.training else None
            p_drop = enc.conv_layers[0].conv[TX_TX].dropout
            adv = None
            if USE_ADAM_KERNEL and adam_counters:
                adv = ops.adam_step_counters(self.opt, self._params)
            planes, samples, dst_neg = ops.step_draws(
                [(c, sd) for _, _, c, sd in views] if views else [], enc.n_heads, p_drop,
                [(self.ix_tx, 0x7478 + inc), (self.ix_bd, 0x6264 + inc)], (self.sg_pos, 0, self.n_bd, 0x7367 + inc),
                enc._step_dev, advance=adv)
            staged = staged._replace(draws=(enc.planes_of(views, planes) if views else None, inc))
            drawn = (samples, dst_neg)
            end = StepEnd(inc, adv is not None)
        z = torch.func.functional_call(
            enc, self._alias,
            ({"tx": tx["x"], "bd": bd["x"]}, {TX_TX: None, TX_BD: None}, {"tx": tx["pos"], "bd": bd["pos"]},
             {"tx": tx["batch"], "bd": bd["batch"]}),
            dict(num_graphs=s["graphs"], graphs=graphs, staged=staged))
        step = enc._step_dev                                  # advanced by the forward: a fresh stream per replay
        # the three losses on the staged sampler indices and their weighted sum as one autograd node (ops.loss_head):
        # means are taken over the padded rows by the kernels and rescaled to the masked real ones by `head_a`
        if drawn is not None:
            (pos, neg, _, _), (bpos, bneg, dp, dn) = drawn[0]
            dst_neg = drawn[1]
        elif fixed is None:
            pos, neg, _, _ = ops.triplet_sample(self.ix_tx, seed=0x7478, seed_dev=step)
            bpos, bneg, dp, dn = ops.triplet_sample(self.ix_bd, seed=0x6264, seed_dev=step)
            # segmentation loss over the real tx-belongs-bd edges (lightning_model.py:167-189): negatives in [0, n_bd_real)
            dst_neg = ops.sample_negatives(self.sg_pos, 0, self.n_bd, seed=0x7367, seed_dev=step)
        else:
            (pos, neg), (bpos, bneg, dp, dn), dst_neg = fixed["tx"], fixed["bd"], fixed["dst_neg"]
        spec = ops.LossHeadSpec((self._iota, pos, neg, lit.loss_tx.margin, lit.loss_tx.eps),
                                (bpos, bneg, dp, dn, self.bd_weight, 1e-8),
                                (self.sg_src, self.sg_pos, dst_neg, lit._sg_margin, 1e-6, self.g_tb.by_dst, True),
                                sg_kind=lit._sg_loss_type, tx_anchors_are_rows=True, sg_of_tx=self.sg_of_tx,
                                tx_state=self.tx_state, grad_out_hint=self._e_loss,
                                defer_finish=DEFER_LOSS_FINISH,      # the losses are read after the backward (self.out after the replay)
                                deterministic=self.deterministic)
        out = ops.loss_head(z["tx"], z["bd"], self.head_a, self.scal[3:6], spec)
        if defer_sums:                                        # ~30 partial sums of the backward as one launch
            with ops.deferred_reductions(self.dev):
                grads = torch.autograd.grad(out, self._leaves, self._e_loss, allow_unused=True)
        else:
            grads = torch.autograd.grad(out, self._leaves, self._e_loss, allow_unused=True)
        for p, g in zip(self._params, grads):
            p.grad = g
        self.out = out.detach()
        return end

    def _warm_up(self, keep) -> None:
        """One eager step before the capture.  With deferred partial sums it is run twice from the same random
        streams -- sums launched where they are produced, then queued -- and the two sets of parameter gradients must
        agree (up to the order of float atomics in the loss kernels); if they do not, some autograd node consumed a
        gradient before the queued sums ran, and this step falls back to immediate sums."""
        if self.defer_sums:
            self._run_grads(False, adam_counters=False)
            ref = [None if p.grad is None else p.grad.detach().clone() for p in self._params]
            with torch.no_grad():
                self.lit.model._step_dev.copy_(keep[3])       # same dropout masks and sampler draws again
                self.tx_state.zero_()                         # (what the staging launch does before every step)
            self._run_grads(True, adam_counters=False)
            names = {id(p): n for n, p in self.lit.model.named_parameters()}
            why = None
            for p, r in zip(self._params, ref):
                g = p.grad
                if (g is None) != (r is None):
                    why = f"{names.get(id(p))}: gradient {'missing' if g is None else 'unexpected'}"
                elif g is not None:
                    scale, diff = float(r.abs().max()), float((g - r).abs().max())
                    # the loss kernels accumulate with (packed 16-bit) float atomics, so two runs of the same backward
                    # differ by a few per cent of a small gradient (seen: 1.4 % on lin_last's bias); a gradient that was
                    # read before its sum was launched is garbage, not a rounding difference: 10 % of the largest
                    # entry separates the two
                    # (deterministic: no atomic decides an order anywhere in the step -- the two runs give equal bytes)
                    if self.deterministic:
                        differs = not torch.equal(g, r)
                    else:
                        differs = not bool(torch.isfinite(g).all()) or diff > 0.1 * scale + 1e-6
                    if differs:
                        why = f"{names.get(id(p))}: differs by {diff:.3e} (scale {scale:.3e})"
                if why:
                    break
            if why:
                self.defer_sums = False
                self.tx_state.zero_()
                import warnings
                warnings.warn("GraphedTrainStep: a parameter gradient is consumed inside the backward pass "
                              f"({why}); partial sums are launched where they are produced (more kernel nodes)")
                self._run_grads(False, adam_counters=False)
            self.opt.step()
        else:
            self._run(warm=True)

    @torch.no_grad()
    def _snapshot(self):
        params = [p for g in self.opt.param_groups for p in g["params"]]
        state = {id(p): {k: v.clone() for k, v in self.opt.state.get(p, {}).items() if isinstance(v, Tensor)}
                 for p in params}
        return params, [p.detach().clone() for p in params], state, self.lit.model._step_dev.clone()

    @torch.no_grad()
    def _restore(self, keep) -> None:
        """Undo the warm-up step IN PLACE (the capture must see the tensors the optimizer keeps using): parameters
        and the dropout counter from the snapshot; optimizer state from the snapshot, or zeroed where the warm-up
        created it (Adam's own initial state)."""
        params, values, state, step_dev = keep
        torch._foreach_copy_(params, values)
        self.lit.model._step_dev.copy_(step_dev)
        for p in params:
            for k, v in self.opt.state.get(p, {}).items():
                if isinstance(v, Tensor):
                    old = state[id(p)].get(k)
                    v.zero_() if old is None else v.copy_(old)

    def _hyper(self) -> tuple:
        """The optimizer hyper-parameters a capture bakes in: none of (lr, betas, eps) when the Adam kernel reads them from
        the staged device array (``_hyper_on_device``: the common case -- a scheduler changing ``lr`` every step replays the
        same graph); otherwise (torch's own optimizer step inside the capture: Python floats become kernel arguments) all
        of them -- a change between steps then triggers a new capture instead of being ignored."""
        if self._hyper_on_device:
            return tuple((g.get("weight_decay", 0), bool(g.get("amsgrad")), bool(g.get("maximize"))) for g in self.opt.param_groups)
        return tuple((g["lr"] if not isinstance(g["lr"], Tensor) else id(g["lr"]), tuple(g["betas"]), g["eps"],
                      g.get("weight_decay", 0)) for g in self.opt.param_groups)

    def step(self, batch, capture: bool = True) -> Tensor:
        """-> [loss_tx, loss_bd, loss_sg, loss] (a static device tensor, overwritten by the next step).  Optimizer step
        hooks (``register_step_pre_hook`` / ``_post_hook``) do not run inside a replay; a changed learning rate / betas / eps
        is staged with the batch (no new capture) on the Adam-kernel route, and re-captures the bucket on any other."""
        lit = self.lit
        self.stage(batch)
        if self.graph is not None and self._captured_hp != self._hyper():
            self.graph = self.graph_opt = self.graph_flush = None      # (the old graphs' memory returns to the pool with them)
        if not capture:
            self._run()
        elif self.graph is None or self._training != lit.model.training:
            lit.model._materialize_bd(self.nodes["bd"]["x"].shape[1], self.dev)
            keep = self._snapshot()
            cap.on_side_stream(lambda: self._warm_up(keep))       # lazy inits, allocator, optimizer state
            self._restore(keep)                               # ... which must not count as a training step
            self.tx_state.zero_()                             # (the warm-up's forward left its chains: staged state again)
            aliases = list(self._alias.values())
            ops.invalidate_weights(aliases)                   # the captured step starts with the weight refresh ...
            self.graph = torch.cuda.CUDAGraph()
            with ops.pack_scope(aliases):                     # ... of this step's own packs only
                if not self.split:
                    with graph_capture(self.graph):
                        self._run()
                else:                                         # forward + backward (+ pack) | <exchange> | Adam
                    with graph_capture(self.graph):
                        end = self._run_grads(self.defer_sums, adam_counters=False, warm=False)
                        self.exchange.pack()                  # gradients -> a bucket's flat buffer; .grad = its slices
                    self.graph_opt = torch.cuda.CUDAGraph()
                    with graph_capture(self.graph_opt, pool=self.graph.pool()):
                        self._opt_step(end)                   # (the dropout counter advances here, on empty steps too)
            # the graph holds raw pointers into these buffers: they must outlive it whatever happens to the cache
            self._pack_refs = [(pk, pk.w, pk.b, pk._wt) for pk in ops.packs_of(aliases)]
            self._grads = [p.grad for p in self._params]
            self._training = lit.model.training
            self._captured_hp = self._hyper()
            self._replay()                                    # (capturing runs nothing)
        else:
            self._replay()
        self._params_changed()
        return self.out

    def _params_changed(self) -> None:
        """The replay stepped the parameters behind Python's back: eager users' compute-dtype copies are stale."""
        ops.invalidate_weights(p for g in self.opt.param_groups for p in g["params"])

    def _replay(self, empty: bool = False) -> None:
        """Fused mode: one replay.  Split mode: replay forward + backward (``empty``: zero the gradients instead -- this
        rank ran out of batches), hand this bucket's gradient tensors to the parameters, let the exchange reduce
        them (exactly ONE collective per step on every rank: the warm-up of a capture never synchronises), replay
        Adam."""
        if not self.split:
            self.graph.replay()
            return
        if empty:
            self.exchange.zero(self._params, self._grads)
        else:
            self.graph.replay()                               # (with a bucket: ends with the pack into the flat buffer)
            self.exchange.adopt(self._params, self._grads)
        self.exchange.reduce()
        self.graph_opt.replay()                               # reads the tensors .grad points at now

    def empty_step(self) -> None:
        self._replay(empty=True)
        self._params_changed()


class GraphedTrainer:
    """``trainer.step(batch)``: stage the batch into the tightest bucket it fits and replay.  A new bucket is captured
    when none fits or the tightest one would pad the transcript side by more than two granules; with ``max_buckets``
    captured, the tightest fit is used whatever it wastes, and a batch no bucket holds is an error."""

    def __init__(self, lit_model, optimizer, granularity: float = 1.06, max_buckets: int = 24, grad_sync=None,
                 grad_bucket=None, clip_grad_norm: Optional[float] = None, loss_scale=None, skip_nonfinite: bool = False,
                 deterministic: bool = False, accumulate_grad_batches: int = 1):
        """Data parallelism: ``grad_bucket`` = a ``dp.FlatGradBucket`` over the model's parameters (the captured
        backward packs into its flat buffer, Adam reads its slices; per step one all-reduce and one divide run eagerly
        between the two graphs), or ``grad_sync`` = any callable that averages the tensors ``.grad`` points at IN PLACE.
        One collective per ``step`` call on every rank; ``step(None)`` is the empty step of a rank that ran out of
        batches: zeros into the exchange, then Adam.

        ``clip_grad_norm`` / ``loss_scale`` (a float or "dynamic") / ``skip_nonfinite``: the gradient guard of
        :class:`GraphedTrainStep`, one state (``self.guard``: ``norm``, ``scale``, ``n_skipped``, ``n_clipped``,
        ``skipped`` as device views) shared by all buckets.  Under data parallelism the guard sits in the SECOND graph,
        behind the exchange: it sees the averaged gradients, every rank holds the same bytes and takes the same decision
        (a non-finite value survives a sum).

        ``deterministic``: every bucket's step takes the loss head's ordered backward (:class:`GraphedTrainStep`): one GPU,
        one seed and one sequence of batches and buckets give bit-identical parameters, Adam state and losses.  Across
        different bucket sequences only as far as padding stays out of every sum; under data parallelism only as far as
        the collective is reproducible.

        ``accumulate_grad_batches`` = N (an int >= 1; 1: off -- no accumulator, no added launch), Lightning's semantics: a
        window is N consecutive ``step(batch)`` calls, each micro-step's gradient counts with weight 1 / N; parameters,
        Adam's moments and step counters, the guard's scale / growth counter / skip count change only when the window
        closes; the dropout / sampler counter advances on every micro-step; ``step`` returns each micro-batch's own
        losses.  ``self.window`` (``ops.GradWindow``: the device-side position + one fp32 accumulator per parameter) is
        shared by all buckets, so a window may span buckets; the device decides what a replay does, the host nothing.
        Guard: the loss scale is constant within a window, a non-finite value in any micro-batch skips the whole window
        (one back-off), the clip norm is the accumulated gradient's.  ``flush()`` closes an open window early.  Refused
        (``NotImplementedError``) with ``grad_sync`` / ``grad_bucket`` and with an optimizer the Adam kernel declines."""
        self.deterministic = bool(deterministic)
        self.lit, self.opt, self.granularity, self.max_buckets = lit_model, optimizer, granularity, max_buckets
        self._guard_kw = dict(clip_grad_norm=clip_grad_norm, loss_scale=loss_scale, skip_nonfinite=skip_nonfinite)
        cfg = guard_config(**self._guard_kw)
        self.guard = None if cfg is None else make_guard(cfg, optimizer, next(lit_model.parameters()).device)
        self.exchange = cap.exchange_of(grad_sync, grad_bucket)
        self.accumulate_grad_batches = accumulation_config(accumulate_grad_batches, optimizer, self.exchange)
        self.window = None                    # ops.GradWindow, made with the first bucket (N > 1 only)
        self.micro_steps = 0                  # host-side mirror of the window's position: for reporting, decides nothing
        self.buckets: List[GraphedTrainStep] = []
        self.n_captures = 0
        self._last: Optional[GraphedTrainStep] = None

    def _empty_step(self) -> None:
        if not self.exchange.split:
            return
        if self._last is not None and self._last.graph_opt is not None:
            self._last.empty_step()
            return
        # no bucket captured yet on this rank: eager
        self.exchange.zero([p for g in self.opt.param_groups for p in g["params"] if p.requires_grad])
        self.exchange.reduce()
        self.opt.step()

    def step(self, batch) -> Optional[Tensor]:
        if batch is None:
            return self._empty_step()
        self._last = cap.pick(
            self.buckets, batch, lambda: self._capture(batch), self.granularity, self.max_buckets,
            f"no captured bucket holds this batch and {self.max_buckets} buckets exist: raise `granularity` or `max_buckets`")
        out = self._last.step(batch)
        self.micro_steps = (self.micro_steps + 1) % self.accumulate_grad_batches
        return out

    @property
    def window_closed(self) -> bool:
        """Did the last ``step`` / ``flush`` leave no window open (always, without accumulation)?"""
        return self.micro_steps == 0

    def flush(self) -> None:
        """Close an open accumulation window early, as Lightning does at the end of an epoch: apply the sum accumulated so
        far, each term still weighted 1 / N.  With nothing open (or without accumulation) it does nothing."""
        if self.window is not None and self._last is not None:
            self._last.flush()
        self.micro_steps = 0

    def _capture(self, batch) -> GraphedTrainStep:
        kw = dict(self._guard_kw)
        if self.accumulate_grad_batches > 1:
            if self.window is None:
                self.window = ops.GradWindow([p for g in self.opt.param_groups for p in g["params"]], self.accumulate_grad_batches)
            kw.update(accumulate_grad_batches=self.accumulate_grad_batches, window=self.window)
        made = GraphedTrainStep(self.lit, self.opt, step_bucket(batch, self.granularity), batch, self.exchange.sync,
                                self.exchange.bucket, guard=self.guard, deterministic=self.deterministic, **kw)
        self.n_captures += 1
        return made
