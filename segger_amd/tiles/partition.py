"""The tile partition of a slide graph: what feeds the hot path (reference ``data/partition/dataset.py:340-579``)."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from ..graph import EdgeCSR, EdgeGraph, batch_cache
from ..hetero import EdgeType, HeteroBatch
from .segments import Segments
from .tiling import QuadTreeTiling, SquareTiling

NODE_SKIP = ("batch", "num_nodes")


def _group_by_tile(data: HeteroBatch, labels: Dict[str, Tensor], num_tiles: int):
    """``data`` re-ordered so that every tile is a contiguous slice -> (stores, node segments, edge segments, node
    permutations).  Inter-tile edges are dropped; endpoints are stored relative to the tile's first node of each type."""
    out = HeteroBatch(num_graphs=1)
    nodes: Dict[str, Segments] = {}
    edges: Dict[EdgeType, Segments] = {}
    inv: Dict[str, Tensor] = {}
    sorted_labels: Dict[str, Tensor] = {}
    for nt in data.node_types:
        lab = labels[nt].long()
        seg = nodes[nt] = Segments.from_labels(lab, num_tiles, f"node type '{nt}'")
        for a, v in data[nt].items():
            if a in NODE_SKIP:
                continue
            out[nt][a] = v.index_select(0, seg.perm) if isinstance(v, Tensor) else v
        i = torch.empty_like(seg.perm)
        i[seg.perm] = torch.arange(seg.perm.numel(), device=seg.perm.device)
        inv[nt] = i
        sorted_labels[nt] = lab[seg.perm]
    for et in data.edge_types:
        s, _, d = et
        ei = data[et].edge_index.long()
        src, dst = inv[s][ei[0]], inv[d][ei[1]]
        ls, ld = sorted_labels[s][src], sorted_labels[d][dst]
        keep = ls == ld
        seg = edges[et] = Segments.from_labels(ls[keep], num_tiles, f"edge type {et}")
        src, dst, lab = src[keep][seg.perm], dst[keep][seg.perm], ls[keep][seg.perm]
        seg.perm = None                                      # (8 bytes per edge that nobody reads again)
        # TILE-LOCAL endpoints (every kept edge is intra-tile): a single-tile batch is then a plain view of this
        # store -- no index arithmetic, no launch -- and a batch of tiles adds each tile's offset inside the batch
        out[et]["edge_index"] = torch.stack([src - nodes[s].indptr[lab], dst - nodes[d].indptr[lab]])
    return out, nodes, edges, {nt: seg.perm for nt, seg in nodes.items()}


class TilePartition:
    """A full-slide graph re-ordered so that tile ``t`` owns nodes ``node_indptr[type][t:t+2]`` and edges
    ``edge_indptr[etype][t:t+2]`` (endpoints stored relative to the tile's first node of each type); edges whose
    endpoints lie in different tiles are dropped (the reference
    does the same, partition/dataset.py:480-494).  ``labels`` maps node type -> tile id per node."""

    # one `segger_csr_from_coo` call sorts fewer than 2^31 edges (int32 slot / edge ids); a slide-level edge store can be
    # larger (reference _patches.py:1-9 documents >INT_MAX edge masks; neighbors.py:159: "600M transcripts" = 9G kNN edges).
    # An instance may override it; its shards inherit the override
    csr_sort_max_edges = (1 << 31) - (1 << 20)

    def __init__(self, data: HeteroBatch, labels: Optional[Dict[str, Tensor]], num_tiles: int, *, grouped=None):
        """``grouped`` (:meth:`shard`): ``(node segments, edge segments, node permutations)`` of a ``data`` that is in tile
        order already; ``labels`` is not read then."""
        self.num_tiles = int(num_tiles)
        if grouped is None:
            data, *grouped = _group_by_tile(data, labels, self.num_tiles)
        # ALL the state of a partition, for a fresh one and for a shard alike
        self.data: HeteroBatch = data
        self._nseg: Dict[str, Segments] = grouped[0]
        self._eseg: Dict[EdgeType, Segments] = grouped[1]
        self._row_ends = {nt: seg.with_ends() for nt, seg in self._nseg.items()}      # the "ptr" stores of build_csr
        self.node_perm: Dict[str, Tensor] = grouped[2]
        self.node_sizes = {nt: seg.sizes for nt, seg in self._nseg.items()}
        self.node_indptr = {nt: seg.indptr for nt, seg in self._nseg.items()}
        self.edge_sizes = {et: seg.sizes for et, seg in self._eseg.items()}
        self.edge_indptr = {et: seg.indptr for et, seg in self._eseg.items()}
        self._csr: Optional[Dict[EdgeType, Dict[str, Dict[str, Tensor]]]] = None      # None: no slide-level sort
        self._src_unique: Dict[EdgeType, bool] = {}
        self.csr_max_tiles = 1                               # largest tile set that is assembled from the slide-level sort
        self.persist_max: Optional[int] = None               # None: two epochs' worth of single-tile batches
        self._persist: "OrderedDict[tuple, dict]" = OrderedDict()
        self._zero_vec: Dict[str, Tensor] = {}

    def __len__(self) -> int:
        return self.num_tiles

    # ---- helpers that keep batch assembly free of host <-> device synchronisation ------------------------
    def _zeros(self, nt: str, n: int) -> Tensor:
        """``batch`` vector of a single-tile batch: a view of one persistent zero vector."""
        z = self._zero_vec.get(nt)
        if z is None or z.numel() < n:
            z = self._zero_vec[nt] = torch.zeros(max(n, max(self._nseg[nt].layout(range(self.num_tiles))[0])),
                                                 dtype=torch.long, device=self.node_perm[nt].device)
        return z[:n]

    @staticmethod
    def _h2d(values: List[int], device) -> Tensor:
        """A small int64 list on the device through pinned memory (a pageable copy stalls the host on the stream)."""
        if torch.device(device).type != "cuda":
            return torch.tensor(values, dtype=torch.long, device=device)
        return torch.tensor(values, dtype=torch.long).pin_memory().to(device, non_blocking=True)

    def _layout(self, tile_ids: Sequence[int]) -> dict:
        """The running-offset arithmetic of one tile set, once: per node type and per edge type ``(sizes, first row of
        each tile inside the batch, total)``.  Every consumer of a batch reads it from here."""
        lay = {nt: seg.layout(tile_ids) for nt, seg in self._nseg.items()}
        lay.update((et, seg.layout(tile_ids)) for et, seg in self._eseg.items())
        return lay

    # ---- sorted edge views, once per slide ----------------------------------------------------------
    def _sort_chunks(self, et: EdgeType) -> List[tuple]:
        """Consecutive tile ranges [t0, t1) whose edges of ``et`` fit one sort.  Tiles are independent graphs with
        contiguous nodes and edges, so the sorted views of a range are the sorted views of its tiles back to back."""
        eptr, cap = self._eseg[et].ptr, int(self.csr_sort_max_edges)
        chunks, t0 = [], 0
        for t in range(self.num_tiles):
            if eptr[t + 1] - eptr[t] > cap:
                raise ValueError(f"tile {t} alone holds {eptr[t + 1] - eptr[t]} edges of {et}: more than one sort "
                                 f"takes ({cap}); use smaller tiles")
            if eptr[t + 1] - eptr[t0] > cap:
                chunks.append((t0, t)); t0 = t
        chunks.append((t0, self.num_tiles))
        return chunks

    def build_csr(self, edge_types: Optional[Sequence[EdgeType]] = None) -> None:
        """Sort every edge store ONCE for the whole slide (``segger_csr_from_coo``: by destination and by source)
        and keep the result in tile-local coordinates.  Tiles are independent graphs whose nodes and edges are
        contiguous, so the CSR views of any batch of tiles are concatenations of per-tile slices plus one offset
        per tile: :meth:`batch` then hands the encoder ready-made views and no batch is ever sorted again
        (5 radix sorts per batch otherwise).  An edge store of 2^31 edges or more is sorted in ranges of whole tiles
        (``csr_sort_max_edges``).  Needs the partition on the GPU."""
        from ..graph import csr_from_coo, sources_unique
        self._csr, self._src_unique = {}, {}
        for et in (edge_types or list(self.data._edges.keys())):
            s, _, d = et
            ei = self.data[et].edge_index                    # tile-local endpoints
            eptr = self._eseg[et].ptr
            tile_ids = torch.arange(self.num_tiles, device=ei.device)
            # once per slide (one sync here, none per batch): does every source have at most one out-edge?  Then the
            # backward of this edge type needs no by-source view (graph.EdgeGraph, segger_gatv2_bwd_args.src_unique)
            if ei.is_cuda:
                first_src = torch.repeat_interleave(self.node_indptr[s][:-1], self.edge_sizes[et], output_size=int(ei.shape[1]))
                self._src_unique[et] = bool(int(sources_unique(ei[0] + first_src, self.data[s].num_nodes)))
                del first_src
            else:
                self._src_unique[et] = False
            views = {}
            for side, (row_t, col_t, row, col) in {"by_dst": (d, s, ei[1], ei[0]), "by_src": (s, d, ei[0], ei[1])}.items():
                rptr, cptr = self._nseg[row_t].ptr, self._nseg[col_t].ptr
                parts = {"ptr": [], "col": [], "eid": []}
                for t0, t1 in self._sort_chunks(et):
                    e0, e1, r0, r1, c0, c1 = eptr[t0], eptr[t1], rptr[t0], rptr[t1], cptr[t0], cptr[t1]
                    tile_of_edge = torch.repeat_interleave(tile_ids[t0:t1], self.edge_sizes[et][t0:t1], output_size=e1 - e0)
                    # chunk-local coordinates for the sort: tile-local id + the tile's first node inside the chunk
                    csr = csr_from_coo(row[e0:e1] + (self.node_indptr[row_t][:-1][tile_of_edge] - r0),
                                       col[e0:e1] + (self.node_indptr[col_t][:-1][tile_of_edge] - c0),
                                       r1 - r0, max(c1 - c0, 1), validate=False)
                    # tile-local coordinates (edges of a tile stay contiguous under the sort: all of them are intra-tile)
                    eid_tile = tile_of_edge[csr.eid.long()]
                    parts["col"].append((csr.col.long() + c0 - self.node_indptr[col_t][:-1][eid_tile]).to(torch.int32))
                    parts["eid"].append((csr.eid.long() + e0 - self.edge_indptr[et][:-1][eid_tile]).to(torch.int32))
                    tile_of_row = torch.repeat_interleave(tile_ids[t0:t1], self.node_sizes[row_t][t0:t1], output_size=r1 - r0)
                    # row starts inside their tile, with every tile's END appended to its rows: tile t owns entries
                    # [nptr[t] + t, nptr[t + 1] + t + 1) -- a complete indptr, so a single-tile batch takes a view
                    # (``Segments.with_ends``)
                    starts = csr.indptr[:-1] + e0 - self.edge_indptr[et][:-1][tile_of_row]
                    k = t1 - t0
                    ptr_c = torch.empty(r1 - r0 + k, dtype=starts.dtype, device=starts.device)
                    ptr_c[torch.arange(r1 - r0, device=starts.device) + (tile_of_row - t0)] = starts
                    ptr_c[(self.node_indptr[row_t][t0 + 1:t1 + 1] - r0) + torch.arange(k, device=starts.device)] = \
                        self.edge_sizes[et][t0:t1].to(starts.dtype)
                    parts["ptr"].append(ptr_c)
                views[side] = {k: (v[0] if len(v) == 1 else torch.cat(v)) for k, v in parts.items()}
            self._csr[et] = views

    def _batch_graph(self, et: EdgeType, tile_ids: Sequence[int], lay: dict, need_by_dst: bool = True,
                     need_by_src: bool = True, edge_index: Optional[Tensor] = None):
        """Sorted views of one edge type for a batch of tiles, sliced from the slide-level sort.  ``edge_index`` (the
        batch's COO list) rides along so that a consumer that does need the skipped by-source view -- the generic
        GATv2 kernels have no one-pass backward -- can still sort it on demand (``EdgeGraph.require_by_src``)."""
        s, _, d = et
        eseg = self._eseg[et]
        e_sizes, e_base, n_edges = lay[et]
        k = len(tile_ids)
        out = {"by_dst": None, "by_src": None}
        unique = self._src_unique.get(et, False)
        if need_by_src == "lazy":                            # skipped when the slide-level check allows it
            need_by_src = not unique
        n_src, n_dst = lay[s][2], lay[d][2]
        for side, row_t, col_t, n_rows, n_cols, need in (("by_dst", d, s, n_dst, n_src, need_by_dst),
                                                         ("by_src", s, d, n_src, n_dst, need_by_src)):
            if not need:
                continue
            v = self._csr[et][side]
            rows = self._row_ends[row_t]
            if k == 1:                                       # views, already in batch coordinates: the tile's own indptr
                indptr, col, eid = rows.take(v["ptr"], tile_ids), eseg.take(v["col"], tile_ids), eseg.take(v["eid"], tile_ids)
            else:                                            # one H2D copy of all per-tile offsets
                dev = v["col"].device
                meta = self._h2d(e_sizes + e_base + lay[row_t][0] + lay[col_t][1], dev)
                es, eb, rs, cb = meta[:k], meta[k:2 * k], meta[2 * k:3 * k], meta[3 * k:]
                starts = torch.cat([v["ptr"][a:b - 1] for a, b in map(rows.span, tile_ids)])      # (rows; not the tiles' ends)
                ptr = starts + torch.repeat_interleave(eb, rs, output_size=n_rows)
                col = eseg.take(v["col"], tile_ids) + torch.repeat_interleave(cb, es, output_size=n_edges).to(torch.int32)
                eid = eseg.take(v["eid"], tile_ids) + torch.repeat_interleave(eb, es, output_size=n_edges).to(torch.int32)
                indptr = torch.empty(ptr.numel() + 1, dtype=torch.long, device=dev)
                indptr[:-1] = ptr
                indptr[-1:] = n_edges
            out[side] = EdgeCSR(indptr, col, eid, n_rows, n_cols).balanced_order()
        return EdgeGraph(out["by_dst"], out["by_src"], n_src, n_dst, n_edges, edge_index, unique)

    def _persistent_store(self, key: tuple) -> dict:
        """Per-tile-set scratch that survives the batch object (sampler indices, rows-by-gene grouping), kept in an
        LRU of ``persist_max`` entries: a shuffling sampler re-packs the tiles every epoch (``TileBatchSampler``,
        reference data_module.py:344), so almost every tile set is new each epoch and an unbounded store would grow by
        one batch-sized entry per step.  Default bound: two epochs' worth of single-tile batches."""
        store = self._persist
        entry = store.get(key)
        if entry is None:
            entry = store[key] = {}
            cap = self.persist_max or max(64, 2 * self.num_tiles)
            while len(store) > cap:
                store.popitem(last=False)
        else:
            store.move_to_end(key)
        return entry

    def shard(self, tile_ids: Sequence[int]) -> "TilePartition":
        """A partition holding ONLY the given tiles (renumbered 0 .. k-1 in the given order), with its own copies of
        their node / edge slices and of the slide-level CSR slices: what a data-parallel rank keeps resident once it
        knows which packed batches it will train on (tiles are independent graphs: ``partition/dataset.py:480-494``
        drops every inter-tile edge).  ``shard(ids).batch([i, j])`` equals ``self.batch([ids[i], ids[j]])``."""
        ids = [int(t) for t in tile_ids]
        if len(set(ids)) != len(ids) or any(not 0 <= t < self.num_tiles for t in ids):
            raise IndexError("shard: tile ids must be distinct and in range")
        # (tile-local endpoints and tile-local sorted views: slices carry over unchanged, nothing to rebase)
        own = lambda seg, v, dim=0: seg.take(v, ids, dim).clone(memory_format=torch.contiguous_format)
        sub = lambda seg: Segments(seg.sizes[seg.sizes.new_tensor(ids)])
        data = HeteroBatch(num_graphs=1)
        for nt, store in self.data._nodes.items():
            for a, v in store.items():
                data[nt][a] = own(self._nseg[nt], v) if isinstance(v, Tensor) else v
        for et, store in self.data._edges.items():
            data[et]["edge_index"] = own(self._eseg[et], store["edge_index"], 1)
        new = TilePartition(data, None, len(ids), grouped=(
            {nt: sub(seg) for nt, seg in self._nseg.items()}, {et: sub(seg) for et, seg in self._eseg.items()},
            {nt: own(seg, self.node_perm[nt]) for nt, seg in self._nseg.items()}))
        new.persist_max, new.csr_max_tiles = self.persist_max, self.csr_max_tiles
        if self.csr_sort_max_edges != TilePartition.csr_sort_max_edges:
            new.csr_sort_max_edges = self.csr_sort_max_edges
        if self._csr:
            new._src_unique = dict(self._src_unique)
            new._csr = {et: {side: {"ptr": own(self._row_ends[row_t], views[side]["ptr"]),
                                    "col": own(self._eseg[et], views[side]["col"]),
                                    "eid": own(self._eseg[et], views[side]["eid"])}
                             for side, row_t in (("by_dst", et[2]), ("by_src", et[0]))}
                        for et, views in self._csr.items()}
        return new

    def _kept(self) -> Tuple[List[Tensor], list]:
        """Every tensor this partition keeps -> (the integer stores batches hand out views of: edge lists, then sorted
        views, in the order :meth:`checksum` weighs them; everything: node / edge stores, permutations, pointers)."""
        handed = [st["edge_index"] for st in self.data._edges.values()]
        handed += [v for views in (self._csr or {}).values() for side in views.values() for v in side.values()]
        stores = [*self.data._nodes.values(), *self.data._edges.values(), self.node_perm, self.node_indptr, self.edge_indptr]
        return handed, handed + [v for st in stores for v in st.values()]

    def resident_bytes(self) -> int:
        """Bytes of every tensor this partition keeps (node / edge stores, permutations, CSR slices)."""
        seen, total = set(), 0
        for t in self._kept()[1]:
            if isinstance(t, Tensor) and t.data_ptr() not in seen:
                seen.add(t.data_ptr()); total += t.numel() * t.element_size()
        return total

    def checksum(self) -> int:
        """A cheap fingerprint of every integer store batches hand out views of (edge lists, sorted views): equal before
        and after an epoch <=> no consumer wrote through a view.  One reduction per tensor + one sync: debug / tests."""
        total = 0
        for i, t in enumerate(self._kept()[0]):
            if t.numel():
                f = t.reshape(-1)
                total += (i + 1) * (int(f.sum(dtype=torch.int64)) + 3 * int(f[::2].sum(dtype=torch.int64))
                                    + 7 * int(f[1::3].sum(dtype=torch.int64)))
        return total & ((1 << 62) - 1)

    def add_node_attr(self, node_type: str, name: str, value: Tensor, permuted: bool = False) -> None:
        self.data[node_type][name] = value if permuted else value.index_select(0, self.node_perm[node_type])

    def weights(self, mode: str = "edge") -> List[int]:
        """Per-tile packing weight: total edges (all edge types) or total nodes (sampler.py:56-64)."""
        src = self.edge_sizes if mode == "edge" else self.node_sizes
        return torch.stack([v.cpu() for v in src.values()]).sum(0).tolist()

    def tile(self, index: int) -> HeteroBatch:
        return self.batch([index])

    def batch(self, tile_ids: Sequence[int]) -> HeteroBatch:
        """The collated batch of the given tiles (== PyG ``Batch.from_data_list([tile(i) ...])`` for the
        fields of the contract): node slices concatenated, edge ids rebased, ``batch`` = graph id.

        READ-ONLY: a single-tile batch is made of VIEWS of the slide-level stores (node attributes, ``edge_index``, and --
        after :meth:`build_csr` -- the sorted views' ``indptr`` / ``col`` / ``eid``): no launch, no copy per batch.  An
        in-place edit by a consumer (``edge_index.add_``, a self-loop transform, ``sort_``) would corrupt the tile for
        every later epoch and every shard; clone what you need to change.  :meth:`checksum` lets a test or a debug run
        assert that nobody did."""
        tile_ids = [int(t) + (self.num_tiles if t < 0 else 0) for t in tile_ids]
        for t in tile_ids:
            if not 0 <= t < self.num_tiles:
                raise IndexError(f"Index {t} is out of range for dataset with {self.num_tiles} partitions.")
        k = len(tile_ids)
        out = HeteroBatch(num_graphs=k)
        lay = self._layout(tile_ids)
        for nt, store in self.data._nodes.items():
            seg, to = self._nseg[nt], out[nt]
            sizes, _, total = lay[nt]
            for a, v in store.items():                       # one tile is a contiguous slice: a view, no copy
                to[a] = seg.take(v, tile_ids) if isinstance(v, Tensor) else v
            if k == 1:
                to["batch"] = self._zeros(nt, total)
            else:                                            # output_size: no device -> host sync for the length
                dev = self.node_perm[nt].device
                to["batch"] = torch.repeat_interleave(torch.arange(k, device=dev), self._h2d(sizes, dev), output_size=total)
        for et, store in self.data._edges.items():
            s, _, d = et
            ei = self._eseg[et].take(store["edge_index"], tile_ids, 1)      # tile-local endpoints; one tile: a view
            if k > 1:
                e_sizes, _, n_e = lay[et]
                meta = self._h2d(e_sizes + lay[s][1] + lay[d][1], ei.device)
                shift = torch.stack([meta[k:2 * k], meta[2 * k:]])       # [2, k]: first node of tile j inside the batch
                ei = ei + torch.repeat_interleave(shift, meta[:k], dim=1, output_size=n_e)
            out[et]["edge_index"] = ei
        cache = batch_cache(out)
        # what never changes for this set of tiles (labels, masks -> the loss samplers' indices) survives the batch object
        cache["persistent"] = self._persistent_store(tuple(tile_ids))
        if self._csr and tile_ids:
            # graph.edge_graph() asks this factory before it sorts a batch's edge store itself
            mine = {et: (out[et]["edge_index"].data_ptr(), int(out[et]["edge_index"].shape[1])) for et in self._csr}

            def factory(key, edge_index, n_src, n_dst, need_by_dst=True, need_by_src=True):    # (no reference to `out`)
                # single-tile batches are pure slices; for many tiles one radix sort of the batch measured faster
                # than concatenating + re-basing 3 arrays x 18 tile slices per view (50M-tx FOV, 16M-edge batches)
                if k <= self.csr_max_tiles and mine.get(key) == (edge_index.data_ptr(), int(edge_index.shape[1])):
                    return self._batch_graph(key, tile_ids, lay, need_by_dst, need_by_src, edge_index)
                return None
            cache["graph_factory"] = factory
            cache["src_unique"] = self._src_unique           # slide-level: holds for every subset of its edges
        return out


def partition_by_tiling(data: HeteroBatch, tiling: Union[SquareTiling, QuadTreeTiling], margin: float,
                        pos_key: str = "pos") -> TilePartition:
    """``TileFitDataset``: label nodes by tile, partition, add the margin ``mask`` (tile_dataset.py:37-60,128-144).
    Takes either tiling: only ``label``, ``mask`` and ``len`` are used (every node must get a label >= 0, which holds
    for a :class:`QuadTreeTiling` built on all node positions, as in data_module.py:244-252)."""
    for nt in data.node_types:
        if "mask" in data[nt]:
            raise KeyError(f"Node type '{nt}' in the 'data' object must not contain an attribute 'mask'.")
    labels = {nt: tiling.label(data[nt][pos_key]) for nt in data.node_types}
    part = TilePartition(data, labels, len(tiling))
    for nt in data.node_types:
        part.add_node_attr(nt, "mask", tiling.mask(part.data[nt][pos_key], margin), permuted=True)
    return part
