"""Inference-only edge scoring with hipGraph replay (BASELINE.json config 5).

``LitISTEncoder.predict_step`` (reference ``src/segger/models/lightning_model.py:263-298``) launches ~150 small
kernels per tile batch; at prediction-tile sizes (<= 50 k nodes, ``data_module.py:155``) the step is
launch-bound.  :class:`GraphedPredictor` captures encoder forward + the fused cosine / arg-max / assignment
kernel into one HIP graph per *shape bucket* and replays it for every batch padded to that bucket:

* a batch is padded to bucket sizes with isolated dummy nodes and dummy->dummy edges, so real nodes see exactly
  their own neighbourhoods (outputs of the real rows are unchanged);
* one ``segger_stage`` launch per batch writes node attributes and the three CSR views (copied from the batch's own
  views, padding by index arithmetic) into the captured buffers -- no per-batch sort or concatenation;
* masks (``predict_mask``) and the device->host copy stay outside the graph, as in the reference; ``predict_device``
  defers both to the caller so that a loop over batches never waits for the GPU; ``predict_into`` hands the rows to a
  ``postprocess.SegmentationAccumulator`` instead, which keeps only the best row per transcript.

hipGraph capture works because every C-ABI entry point only enqueues on the caller's stream and never
allocates or synchronises (include/segger_amd.h conventions).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import capture as cap, ops
from .graph import EdgeGraph, batch_cache, edge_graph, graph_capture, padded_view_segments
from .hetero import TX_BD, TX_NB_BD, TX_TX

_EDGES = {"__".join(et): et for et in (TX_TX, TX_BD, TX_NB_BD)}          # size key -> edge type
_E_TT = "__".join(TX_TX)


def bucket_sizes(batch, granularity: float = 1.25, floor: int = 1024, headroom: int = 0) -> Dict[str, int]:
    """Round every node / edge count up to the next power of ``granularity`` (>= floor + 1 for the dummy).  The boundary
    side is cheap: everything but the transcripts and their neighbour edges gets ``headroom`` granules more."""
    c = cap.counts(batch, _EDGES)
    return {k: cap.ladder(c[k], granularity, floor, 0 if k in ("tx", _E_TT) else headroom)
            for k in ("tx", "bd", *_EDGES)}


class GraphedPredictor:
    """Replays ``model.predict_step`` for batches of ONE bucket shape through a captured HIP graph.

    A batch is written into the static buffers by ONE launch (``ops.stage`` -> ``segger_stage``): node attributes are
    copied and padded with copies of node 0; the three CSR views (tx-neighbors-tx and tx-belongs-bd by destination,
    tx-neighbors-bd by source) are copied from the batch's own views -- slices of the slide-level sort when the batch
    comes from ``tiles.TilePartition`` -- and their padding edges are index arithmetic on the dummy rows
    (``graph.padded_view_segments``): no per-batch sort, no concatenation."""

    def __init__(self, model, sizes: Dict[str, int], bd_dim: int, min_similarity: Optional[float] = None,
                 max_graphs: int = 64):
        self.model, self.sizes, self.min_similarity = model, dict(sizes), min_similarity
        dev = next(model.parameters()).device
        self.dev = dev
        nt, nb = sizes["tx"], sizes["bd"]
        z = cap.zeros_on(dev)
        self.inp = {
            "tx_x": z(nt, dtype=torch.int32), "tx_pos": z(nt, 2), "tx_batch": z(nt, dtype=torch.long),
            "bd_x": z(nb, bd_dim), "bd_pos": z(nb, 2), "bd_batch": z(nb, dtype=torch.long),
            "bd_index": z(nb, dtype=torch.long),
        }
        self._nodes = {t: {a: self.inp[f"{t}_{a}"] for a in ("x", "pos", "batch")} for t in ("tx", "bd")}
        csr = lambda n_rows, n_cols, n_edges: cap.static_csr(n_rows, n_cols, n_edges, dev)
        e = {et: sizes[k] for k, et in _EDGES.items()}
        self.graphs: Dict[Tuple[str, str, str], EdgeGraph] = {
            TX_TX: EdgeGraph(csr(nt, nt, e[TX_TX]), None, nt, nt, e[TX_TX]),
            TX_BD: EdgeGraph(csr(nb, nt, e[TX_BD]), None, nt, nb, e[TX_BD]),
            TX_NB_BD: EdgeGraph(None, csr(nt, nb, e[TX_NB_BD]), nt, nb, e[TX_NB_BD]),
        }
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.out: Dict[str, Tensor] = {}
        # the per-graph min / max tables are sized for max_graphs, so one captured graph serves batches of any
        # number of tiles up to that (graphs without nodes are never read)
        self.num_graphs = int(max_graphs)
        self._limits = {**self.sizes, "graphs": self.num_graphs}

    def fits(self, batch) -> bool:
        return cap.fits(self._limits, batch, _EDGES)

    def waste(self, batch) -> float:
        return cap.waste(self.sizes, batch, _EDGES, _E_TT)

    # -- staging ------------------------------------------------------------------------------
    @torch.no_grad()
    def _stage(self, batch) -> None:
        if not self.fits(batch):
            raise ValueError("batch does not fit this predictor's bucket")
        tx, bd = batch["tx"], batch["bd"]
        n_tx, n_bd, nt, nb = tx.num_nodes, bd.num_nodes, self.sizes["tx"], self.sizes["bd"]
        cache = batch_cache(batch)
        # the same cache keys the eager predict_step uses: a batch scored both ways is sorted (or sliced) once
        g_tt = edge_graph(cache, TX_TX, batch[TX_TX].edge_index, n_tx, n_tx, need_by_src=False, validate=False)
        g_tb = edge_graph(cache, TX_BD, batch[TX_BD].edge_index, n_tx, n_bd, need_by_src=False, validate=False)
        g_nb = edge_graph(cache, TX_NB_BD, batch[TX_NB_BD].edge_index, n_tx, n_bd, need_by_dst=False, validate=False)
        # nodes: dummies are copies of node 0 (gene id 0)
        segs = cap.node_segments(self._nodes, tx, bd, 0) + [(self.inp["bd_index"], bd["index"], "tile", 1, 0, 0)]
        segs += padded_view_segments(self.graphs[TX_TX].by_dst, g_tt.by_dst, n_tx, None)
        segs += padded_view_segments(self.graphs[TX_BD].by_dst, g_tb.by_dst, n_bd, ("mod", n_tx, nt - n_tx))
        segs += padded_view_segments(self.graphs[TX_NB_BD].by_src, g_nb.by_src, n_tx, ("mod", n_bd, nb - n_bd))
        ops.stage(segs, self.dev)

    def _run(self) -> None:
        m = self.model.model
        z = m(
            {"tx": self.inp["tx_x"], "bd": self.inp["bd_x"]},
            {et: None for et in (TX_TX, TX_BD)},
            {"tx": self.inp["tx_pos"], "bd": self.inp["bd_pos"]},
            {"tx": self.inp["tx_batch"], "bd": self.inp["bd_batch"]},
            num_graphs=self.num_graphs, graphs={et: self.graphs[et] for et in (TX_TX, TX_BD)},
        )
        max_sim, _, seg, _ = ops.edge_cos_argmax(self.graphs[TX_NB_BD].by_src, z["tx"], z["bd"],
                                                 dst_index=self.inp["bd_index"], min_similarity=self.min_similarity)
        self.out = {"max_sim": max_sim, "seg_idx": seg}

    # -- public -------------------------------------------------------------------------------
    @torch.no_grad()
    def predict_device(self, batch):
        """-> (tx_index, seg_idx, max_sim, gene_id, predict_mask) on the DEVICE, all [n_tx] and NOT yet filtered by the
        mask: nothing here waits for the GPU, so a loop over batches queues ahead of it; apply the mask (one
        compaction, one sync) after the loop."""
        self._stage_and_replay(batch)
        n = batch["tx"].num_nodes
        return (batch["tx"]["index"], self.out["seg_idx"][:n].clone(), self.out["max_sim"][:n].clone(),
                batch["tx"]["x"], batch["tx"]["predict_mask"])

    def _stage_and_replay(self, batch) -> None:
        if self.model.training:
            raise RuntimeError("GraphedPredictor needs model.eval()")
        self._stage(batch)
        if self.graph is None:
            cap.on_side_stream(self._run)            # warm-up (lazy inits, allocator)
            self.graph = torch.cuda.CUDAGraph()
            with graph_capture(self.graph):
                self._run()
        self.graph.replay()

    @torch.no_grad()
    def predict_into(self, batch, acc) -> None:
        """Score ``batch`` and feed its rows to ``acc`` (a ``postprocess.SegmentationAccumulator``): stage, replay, then
        one ``acc.update`` straight from the static output buffers on the same stream -- no clone, no compaction, no
        sync.  The next batch's replay is ordered behind that update, so the buffers are free to be overwritten."""
        self._stage_and_replay(batch)
        n = batch["tx"].num_nodes
        acc.update(batch["tx"]["index"], self.out["seg_idx"][:n], self.out["max_sim"][:n], batch["tx"]["x"],
                   mask=batch["tx"]["predict_mask"])

    @torch.no_grad()
    def predict(self, batch):
        """-> (tx_index, seg_idx, max_sim, gene_id) on the CPU, exactly like ``predict_step``."""
        index, seg, sim, gene, mask = self.predict_device(batch)
        return tuple(t[mask].cpu() for t in (index, seg, sim, gene))


class GraphedPredictorPool:
    """``pool.predict(batch)`` / ``pool.predict_device(batch)``: the tightest captured bucket the batch fits; a new
    one is captured when none fits or the tightest would pad the transcript side by more than two granules."""

    def __init__(self, model, bd_dim: int, min_similarity: Optional[float] = None, granularity: float = 1.08,
                 max_buckets: int = 32, max_graphs: int = 64):
        self.model, self.bd_dim, self.min_similarity = model, bd_dim, min_similarity
        self.granularity, self.max_buckets, self.max_graphs = granularity, max_buckets, max_graphs
        self.buckets: list = []

    def _pick(self, batch) -> GraphedPredictor:
        return cap.pick(self.buckets, batch, lambda: self._capture(batch), self.granularity, self.max_buckets,
                        f"no captured bucket holds this batch and {self.max_buckets} buckets exist")

    def _capture(self, batch) -> GraphedPredictor:
        return GraphedPredictor(self.model, bucket_sizes(batch, self.granularity, floor=256, headroom=1), self.bd_dim,
                                self.min_similarity, max(self.max_graphs, int(getattr(batch, "num_graphs", 1))))

    def predict(self, batch):
        return self._pick(batch).predict(batch)

    def predict_device(self, batch):
        return self._pick(batch).predict_device(batch)

    def predict_into(self, batch, acc) -> None:
        self._pick(batch).predict_into(batch, acc)
