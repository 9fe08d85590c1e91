"""Overlapping prediction tiles (reference ``data/tile_dataset.py:156-264``), by a whole-slide scan or from nodes binned once."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from ..hetero import EdgeType, HeteroBatch
from .partition import NODE_SKIP
from .segments import Segments
from .tiling import QuadTreeTiling, SquareTiling


class PredictTiles:
    """Overlapping prediction tiles: the subgraph of all nodes inside ``tile.buffer(margin)`` with a
    ``predict_mask`` marking nodes inside the tile proper (tile_dataset.py:218-246).  Boxes follow the
    reference's half-open outer test (``>= lo`` and ``< hi``) and closed inner test (``>=`` and ``<=``)."""

    def __init__(self, data: HeteroBatch, tiles: Tensor, margin: float = 0.0):
        missing = [nt for nt in data.node_types if "pos" not in data[nt]]
        if missing:
            raise ValueError(f"Missing 'pos' attribute for node type: {', '.join(missing)}")
        self.data, self.tiles, self.margin = data, tiles, float(margin)

    def __len__(self) -> int:
        return int(self.tiles.shape[0])

    def _box(self, idx: int) -> Tuple[float, ...]:
        if idx < 0 or idx >= len(self):
            raise IndexError(f"Requested {idx}, but tiling only contains {len(self)} tiles.")
        return tuple(float(v) for v in self.tiles[idx])

    def _subgraph_nodes(self, box: Tuple[float, ...], candidates: Optional[Dict[str, Tensor]] = None):
        """The node side of one prediction tile -> (batch holding the node stores, ``predict_mask`` and ``batch``; per node
        type the kept nodes' original ids, ascending like a boolean-mask subgraph).  ``candidates``: per node type, ids of
        a superset of the nodes inside the grown box, in any order (None: every node)."""
        x0, y0, x1, y1 = box
        m = self.margin
        out = HeteroBatch(num_graphs=1)
        subs: Dict[str, Tensor] = {}
        for nt, store in self.data._nodes.items():
            pos = store["pos"] if candidates is None else store["pos"].index_select(0, candidates[nt])
            keep = (pos[:, 0] >= x0 - m) & (pos[:, 0] < x1 + m) & (pos[:, 1] >= y0 - m) & (pos[:, 1] < y1 + m)
            sub = keep.nonzero(as_tuple=False).squeeze(1) if candidates is None else candidates[nt][keep].sort().values
            subs[nt] = sub
            for a, v in store.items():
                if a in NODE_SKIP:
                    continue
                out[nt][a] = v.index_select(0, sub) if isinstance(v, Tensor) else v
            p = out[nt]["pos"]
            out[nt]["predict_mask"] = (p[:, 0] >= x0) & (p[:, 0] <= x1) & (p[:, 1] >= y0) & (p[:, 1] <= y1)
            out[nt]["batch"] = torch.zeros(sub.numel(), dtype=torch.long, device=pos.device)
        return out, subs

    def __getitem__(self, idx: int) -> HeteroBatch:
        out, subs = self._subgraph_nodes(self._box(idx))
        new_id: Dict[str, Tensor] = {}
        for nt, sub in subs.items():
            nid = torch.full((self.data[nt]["pos"].shape[0],), -1, dtype=torch.long, device=sub.device)
            nid[sub] = torch.arange(sub.numel(), device=sub.device)
            new_id[nt] = nid
        for et, store in self.data._edges.items():
            s, _, d = et
            ei = store["edge_index"].long()
            a, b = new_id[s][ei[0]], new_id[d][ei[1]]
            ok = (a >= 0) & (b >= 0)
            out[et]["edge_index"] = torch.stack([a[ok], b[ok]])
        return out


class _BinnedPredictTiles(PredictTiles):
    """``PredictTiles`` with work per tile proportional to what the tile can contain instead of the whole slide: nodes
    are binned once (one stable sort), edges by the bin of their source, and a prediction tile only looks at the bins
    ``_bins(idx)`` names -- a superset of its nodes; the exact box test follows.  Returns exactly what
    ``PredictTiles.__getitem__`` returns (same node and edge order)."""

    def _bin_graph(self, bin_of: Dict[str, Tensor], n_bins: int) -> None:
        self._nseg: Dict[str, Segments] = {}
        self._nptr: Dict[str, List[int]] = {}
        self._new_id: Dict[str, Tensor] = {}
        for nt, store in self.data._nodes.items():
            pos = store["pos"]
            self._nseg[nt] = Segments.from_labels(bin_of[nt], n_bins, f"node type '{nt}'")
            self._nptr[nt] = self._nseg[nt].ptr
            self._new_id[nt] = torch.full((pos.shape[0],), -1, dtype=torch.long, device=pos.device)
        self._edges: Dict[EdgeType, Tensor] = {}
        self._eseg: Dict[EdgeType, Segments] = {}
        for et, store in self.data._edges.items():
            ei = store["edge_index"].long()
            seg = self._eseg[et] = Segments.from_labels(bin_of[et[0]][ei[0]], n_bins, f"edge type {et}")
            self._edges[et] = torch.cat([ei[:, seg.perm], seg.perm[None]], 0)      # rows: src, dst, original edge id
            seg.perm = None                                  # (kept as the table's third row)

    def _bins(self, idx: int) -> List[int]:
        raise NotImplementedError

    def __getitem__(self, idx: int) -> HeteroBatch:
        box = self._box(idx)
        neigh = self._bins(idx)
        out, subs = self._subgraph_nodes(box, {nt: seg.take(seg.perm, neigh) for nt, seg in self._nseg.items()})
        for nt, sub in subs.items():
            self._new_id[nt][sub] = torch.arange(sub.numel(), device=sub.device)
        for et in self.data._edges:
            s, _, d = et
            e = self._eseg[et].take(self._edges[et], neigh, 1)
            a, b = self._new_id[s][e[0]], self._new_id[d][e[1]]
            kept = ((a >= 0) & (b >= 0)).nonzero(as_tuple=False).squeeze(1)      # one compaction (one sync) per type
            kept = kept[torch.argsort(e[2][kept])]                                # back to the original edge order
            out[et]["edge_index"] = torch.stack([a[kept], b[kept]])
        for nt, sub in subs.items():
            self._new_id[nt][sub] = -1
        return out


class PredictTileIndex(_BinnedPredictTiles):
    """``PredictTiles`` over the tiles of a :class:`SquareTiling` with work per tile proportional to what the tile
    can contain instead of the whole slide: nodes are binned once (one stable sort), edges by the bin of their source,
    and a prediction tile only looks at the bins its margin can reach.  With ``2 * margin <= side`` every tile is
    binned into 3 x 3 sub-cells -- border strips of the margin's width around an interior -- and a prediction tile takes
    its own nine plus the strips of its eight neighbours that face it (~1.2x its own content for segger's 10 um margin
    on ~220 um tiles); wider margins fall back to whole 3 x 3 tile neighbourhoods (9x).  Returns exactly what
    ``PredictTiles.__getitem__`` returns (same node and edge order).  Needs ``margin <= side_length``."""

    def __init__(self, data: HeteroBatch, tiling: SquareTiling, margin: float = 0.0):
        super().__init__(data, tiling.tiles, margin)
        if margin > tiling.side_length:
            raise ValueError(f"margin ({margin}) must not exceed the tile side ({tiling.side_length})")
        self.nx, self.ny = tiling.nx, tiling.ny
        T = len(tiling)
        self.strips = 2.0 * margin <= tiling.side_length
        self._sub = 9 if self.strips else 1                  # bins per tile
        bin_of: Dict[str, Tensor] = {}
        tiles_t = tiling.tiles
        for nt, store in data._nodes.items():
            pos = store["pos"]
            ix, iy = tiling._cell(pos)                        # clamped: nodes outside the extent go to a border tile
            lab = ix * tiling.ny + iy
            if self.strips:
                # strip index inside the node's own tile: 0 / 2 = within the margin of the low / high border (a hair
                # wider than the margin: the exact box test in __getitem__ decides, this only has to be a superset)
                box = tiles_t.to(pos.device)[lab]
                w = margin * (1.0 + 1e-6) + 1e-6 * tiling.side_length
                sx = (pos[:, 0] >= box[:, 2] - w).long() * 2
                sx = torch.where(pos[:, 0] < box[:, 0] + w, torch.zeros_like(sx), torch.where(sx == 2, sx, torch.ones_like(sx)))
                sy = (pos[:, 1] >= box[:, 3] - w).long() * 2
                sy = torch.where(pos[:, 1] < box[:, 1] + w, torch.zeros_like(sy), torch.where(sy == 2, sy, torch.ones_like(sy)))
                # a tile narrower than two margins cannot happen here (2 * margin <= side), but low wins on a tie
                lab = lab * 9 + sx * 3 + sy
            bin_of[nt] = lab
        self._bin_graph(bin_of, T * self._sub)

    def _bins(self, idx: int) -> List[int]:
        """Bins a node of prediction tile ``idx`` can lie in (a node of a neighbouring tile must be within the margin of
        the shared border, i.e. in the strip facing this tile)."""
        ix, iy = idx // self.ny, idx % self.ny
        out: List[int] = []
        for jx in range(max(ix - 1, 0), min(ix + 2, self.nx)):
            for jy in range(max(iy - 1, 0), min(iy + 2, self.ny)):
                t = jx * self.ny + jy
                if not self.strips:
                    out.append(t)
                    continue
                dx, dy = jx - ix, jy - iy
                xs = (2,) if dx < 0 else (0,) if dx > 0 else (0, 1, 2)
                ys = (2,) if dy < 0 else (0,) if dy > 0 else (0, 1, 2)
                out.extend(t * 9 + sx * 3 + sy for sx in xs for sy in ys)
        return out


class PredictQuadTreeIndex(_BinnedPredictTiles):
    """``PredictTiles`` over the leaves of a :class:`QuadTreeTiling` -- the counterpart of :class:`PredictTileIndex` for
    tiles of unequal size (``PredictTiles.__getitem__`` scans the whole slide per tile: unusable at 50M transcripts x
    thousands of tiles).  Nodes are binned by their leaf label; a prediction tile looks only at the leaves whose box
    meets its own box grown by ``margin`` (a closed test and a hair wider, so a superset; computed once on the host from
    the ``[T, 4]`` table), then applies the exact box test.  Nodes without a leaf (label -1: outside the root, or in a
    quadrant that was empty at build time) share one extra bin that every tile scans."""

    def __init__(self, data: HeteroBatch, tiling: QuadTreeTiling, margin: float = 0.0):
        super().__init__(data, tiling.tiles, margin)
        T = len(tiling)
        bin_of = {}
        for nt, store in data._nodes.items():
            lab = tiling.label(store["pos"])
            bin_of[nt] = torch.where(lab >= 0, lab, torch.full_like(lab, T))
        self._bin_graph(bin_of, T + 1)
        # a node of leaf j lies in j's closed box, so it can only fall into tile i's grown box if the two boxes meet; the
        # exact test compares in the positions' own precision (float32 rounds the bounds), hence the hair of slack
        t = tiling.tiles
        grow = self.margin + 1e-6 * (1.0 + float(t.abs().max()))
        self._near: List[List[int]] = []
        for i0 in range(0, T, 1024):
            a = t[i0:i0 + 1024, None, :]
            meet = ((t[None, :, 0] <= a[..., 2] + grow) & (t[None, :, 2] >= a[..., 0] - grow) &
                    (t[None, :, 1] <= a[..., 3] + grow) & (t[None, :, 3] >= a[..., 1] - grow))
            self._near.extend(row.nonzero(as_tuple=False).squeeze(1).tolist() for row in meet)
        self._extra = T

    def _bins(self, idx: int) -> List[int]:
        return self._near[idx] + [self._extra]
