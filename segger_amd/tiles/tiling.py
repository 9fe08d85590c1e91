"""Tilings of a slide: the uniform square grid and the adaptive quadtree (reference ``data/tiling.py``)."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
from torch import Tensor


class SquareTiling:
    """Uniform square grid over the extent of ``positions`` (edge tiles are clipped to the extent)."""

    def __init__(self, positions: Tensor, side_length: float):
        if side_length <= 0:
            raise ValueError(f"side_length must be positive, but got {side_length}.")
        if positions.dim() != 2 or positions.shape[-1] != 2:
            raise ValueError(f"positions must be a tensor of shape (N, 2), but got {positions.shape}.")
        if len(positions) == 0:
            raise ValueError("positions cannot be empty.")
        self.min_x, self.max_x = positions[:, 0].min().item(), positions[:, 0].max().item()
        self.min_y, self.max_y = positions[:, 1].min().item(), positions[:, 1].max().item()
        self.side_length = float(side_length)
        self.nx = max(1, math.ceil((self.max_x - self.min_x) / self.side_length))
        self.ny = max(1, math.ceil((self.max_y - self.min_y) / self.side_length))

    def __len__(self) -> int:
        return self.nx * self.ny

    @property
    def tiles(self) -> Tensor:
        """[T, 4] boxes (x0, y0, x1, y1); tile id = ix * ny + iy (meshgrid 'ij' order of the reference)."""
        ix = torch.arange(self.nx, dtype=torch.float64).repeat_interleave(self.ny)
        iy = torch.arange(self.ny, dtype=torch.float64).repeat(self.nx)
        x0 = self.min_x + ix * self.side_length
        y0 = self.min_y + iy * self.side_length
        x1 = torch.minimum(x0 + self.side_length, torch.tensor(self.max_x, dtype=torch.float64))
        y1 = torch.minimum(y0 + self.side_length, torch.tensor(self.max_y, dtype=torch.float64))
        return torch.stack([x0, y0, x1, y1], 1)

    def _cell(self, pos: Tensor):
        fx = (pos[:, 0].double() - self.min_x) / self.side_length
        fy = (pos[:, 1].double() - self.min_y) / self.side_length
        ix = fx.floor().long().clamp_(0, self.nx - 1)
        iy = fy.floor().long().clamp_(0, self.ny - 1)
        return ix, iy

    def label(self, pos: Tensor) -> Tensor:
        """Tile index of every point ('intersects': boundaries included; a point on a shared edge goes to
        the upper tile, points on the extent's max edge to the last tile); -1 outside the extent."""
        ix, iy = self._cell(pos)
        lab = ix * self.ny + iy
        inside = ((pos[:, 0] >= self.min_x) & (pos[:, 0] <= self.max_x) &
                  (pos[:, 1] >= self.min_y) & (pos[:, 1] <= self.max_y))
        return torch.where(inside, lab, torch.full_like(lab, -1))

    def mask(self, pos: Tensor, margin: float) -> Tensor:
        """True where the point lies strictly inside its tile shrunk by ``margin`` ('contains').  A margin
        that would make a tile vanish is halved until every tile survives (tiling.py:103-127)."""
        if margin < 0:
            raise ValueError(f"The margin must be non-negative, but got {margin}.")
        t = self.tiles
        w = torch.minimum(t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]).min().item()
        eff = float(margin)
        while eff > 0 and 2 * eff >= w:
            eff = eff / 2 if eff > 1e-6 else 0.0
        ix, iy = self._cell(pos)
        tid = ix * self.ny + iy
        box = t.to(pos.device)[tid]
        x, y = pos[:, 0].double(), pos[:, 1].double()
        return ((x > box[:, 0] + eff) & (x < box[:, 2] - eff) & (y > box[:, 1] + eff) & (y < box[:, 3] - eff))


class QuadTreeTiling:
    """Adaptive tiling: the leaves of a point quadtree with at most ``max_tile_size`` points each (``len`` = T).

    Contract (exact integer arithmetic; the kernels and the torch path agree bit for bit):

    * root, in float64: ``x0 = min_x - b``, ``y0 = min_y - b``, ``x1 = max_x + b``, ``y1 = max_y + b`` with
      ``b = margin_bounds``; ``extent = max(x1 - x0, y1 - y0)``; ``D_raw`` = the smallest integer >= 1 with
      ``2^D_raw > extent``; ``depth = min(D_raw, 15)`` and ``cell = 2^(D_raw - depth)`` (quadtree.py:33-52);
    * cell of a point: ``ix = clamp(floor((double(x) - x0) / cell), 0, 2^depth - 1)``, ``iy`` alike; Morton key = two bits
      per level, x in the even bit and y in the odd bit (``keys_to_coordinates``, quadtree.py:56-94);
    * the node at depth ``d`` in ``1..depth`` is the prefix ``key >> 2 (depth - d)``; the root is never a tile.  A node
      with ``c > 0`` points is a leaf iff every proper ancestor holds more than ``max_tile_size`` points and
      (``c <= max_tile_size`` or ``d == depth``); empty quadrants are not tiles.  A leaf at the depth cap may be over size
      (coincident points): see ``counts``;
    * tile ids ascend in ``(d, prefix)``: the breadth-first order in which the reference's leaf filter keeps them;
    * ``tiles[i] = (x0 + kx s, y0 + ky s, min(x0 + (kx + 1) s, x1), min(y0 + (ky + 1) s, y1))`` with
      ``s = cell 2^(depth - d)`` and ``(kx, ky)`` decoded from the prefix (clipped as in quadtree.py:137-138).

    ``levels`` (the reference's ``level`` column, ``d - 1``), ``keys`` (prefixes) and ``counts`` are the per-leaf tables,
    ``tiles`` the ``[T, 4]`` float64 boxes (all on the host, like ``SquareTiling.tiles``); ``labels`` holds the leaf of
    every build point (int32, on the positions' device).

    Two deliberate departures from the reference: (1) above ``D_raw = 15`` its ``scale`` and its box formula disagree;
    boxes here stay powers of two (``cell = 2^(D_raw - 15)``).  (2) its ``intersects`` join + ``drop_duplicates`` gives a
    point on a shared border to whichever tile comes first in an unspecified order; ``label`` is half-open by construction
    (the upper cell), hence deterministic.

    float32 CUDA positions take the HIP kernels (``segger_quadtree_build`` / ``segger_quadtree_label``); anything else
    takes the torch path."""

    MAX_DEPTH = 15

    def __init__(self, positions: Tensor, max_tile_size: int, margin_bounds: float = 50.0):
        if positions.dim() != 2 or positions.shape[-1] != 2:
            raise ValueError(f"positions must be a tensor of shape (N, 2), but got {positions.shape}.")
        n = int(positions.shape[0])
        if n == 0:
            raise ValueError("positions cannot be empty.")
        if n >= 1 << 31:
            raise ValueError(f"one tree takes fewer than 2^31 points, but got {n}.")
        if int(max_tile_size) < 1:
            raise ValueError(f"max_tile_size must be at least 1, but got {max_tile_size}.")
        if margin_bounds < 0:
            raise ValueError(f"margin_bounds must be non-negative, but got {margin_bounds}.")
        self.max_tile_size = int(max_tile_size)
        lo, hi = torch.aminmax(positions, dim=0)
        min_x, min_y, max_x, max_y = torch.cat([lo, hi]).double().tolist()           # one host sync
        if not all(math.isfinite(v) for v in (min_x, min_y, max_x, max_y)):
            raise ValueError("positions must be finite.")
        b = float(margin_bounds)
        self.x0, self.y0, self.x1, self.y1 = min_x - b, min_y - b, max_x + b, max_y + b
        extent = max(self.x1 - self.x0, self.y1 - self.y0)
        d_raw = 1
        while 2.0 ** d_raw <= extent:
            d_raw += 1
        self.depth = min(d_raw, self.MAX_DEPTH)
        self.cell = 2.0 ** (d_raw - self.depth)
        self._tables: Dict[tuple, Tuple[Tensor, ...]] = {}
        if positions.is_cuda and positions.dtype == torch.float32:
            depths, keys, counts = self._build_device(positions.contiguous())
        else:
            depths, keys, counts = self._build_torch(positions)
        self.levels, self.keys, self.counts = depths - 1, keys, counts
        shift = 2 * (self.depth - depths)
        kx, ky = self._compact(keys), self._compact(keys >> 1)
        side = self.cell * torch.pow(2.0, (self.depth - depths).double())
        bx, by = self.x0 + kx.double() * side, self.y0 + ky.double() * side
        self.tiles = torch.stack([bx, by, (bx + side).clamp(max=self.x1), (by + side).clamp(max=self.y1)], 1)
        if not self._tables:                                 # torch path: the Morton-ordered range starts of the leaves
            m_lo = keys << shift
            order = torch.argsort(m_lo)
            self._tables[(torch.device("cpu"), torch.long)] = (keys, depths, m_lo[order], order)
            self.labels = self.label(positions).to(torch.int32)

    def __len__(self) -> int:
        return int(self.keys.numel())

    # ---- keys ------------------------------------------------------------------------------------------------
    @staticmethod
    def _spread(v: Tensor) -> Tensor:
        """bit i of a 15-bit value -> bit 2 i"""
        v = (v | (v << 8)) & 0x00ff00ff
        v = (v | (v << 4)) & 0x0f0f0f0f
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555

    @staticmethod
    def _compact(v: Tensor) -> Tensor:
        """the even bits of a key, packed: the inverse of :meth:`_spread`"""
        v = v & 0x55555555
        v = (v | (v >> 1)) & 0x33333333
        v = (v | (v >> 2)) & 0x0f0f0f0f
        v = (v | (v >> 4)) & 0x00ff00ff
        return (v | (v >> 8)) & 0x0000ffff

    def _key(self, pos: Tensor) -> Tuple[Tensor, Tensor]:
        """Morton key at the full depth (int64) and whether the point lies inside the closed root box."""
        x, y = pos[:, 0].double(), pos[:, 1].double()
        top = (1 << self.depth) - 1
        ix = ((x - self.x0) / self.cell).floor().clamp(0, top).long()
        iy = ((y - self.y0) / self.cell).floor().clamp(0, top).long()
        inside = (x >= self.x0) & (x <= self.x1) & (y >= self.y0) & (y <= self.y1)
        return self._spread(ix) | (self._spread(iy) << 1), inside

    # ---- build -----------------------------------------------------------------------------------------------
    def leaf_capacity(self, n: int) -> int:
        """Upper bound of the number of leaves: the nodes split at one depth are disjoint with more than
        ``max_tile_size`` points each, and a split turns one node into at most four."""
        return min(n, 4 + 3 * (self.depth - 1) * (n // (self.max_tile_size + 1)))

    def _build_torch(self, positions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        key, _ = self._key(positions)
        active = key.sort().values                           # keys of the points whose ancestors were all split
        depths, keys, counts = [], [], []
        for d in range(1, self.depth + 1):
            if active.numel() == 0:
                break
            prefix, cnt = torch.unique_consecutive(active >> (2 * (self.depth - d)), return_counts=True)
            leaf = cnt <= self.max_tile_size if d < self.depth else torch.ones_like(cnt, dtype=torch.bool)
            depths.append(torch.full_like(prefix[leaf], d))
            keys.append(prefix[leaf])
            counts.append(cnt[leaf])
            active = active[torch.repeat_interleave(~leaf, cnt)]
        return torch.cat(depths).cpu(), torch.cat(keys).cpu(), torch.cat(counts).cpu()

    def _build_device(self, positions: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        from .. import _lib
        dev, n = positions.device, int(positions.shape[0])
        cap = self.leaf_capacity(n)
        ws, ws_bytes = _lib.workspace("segger_quadtree_workspace_bytes", dev, n, self.depth, self.max_tile_size, cap)
        table = torch.empty((5, cap), dtype=torch.int32, device=dev)     # leaf key, depth, count; Morton start, id
        n_leaf = torch.empty(1, dtype=torch.int32, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.call("segger_quadtree_build", dev, positions.data_ptr(), n, self.x0, self.y0, self.cell, self.depth,
                  self.max_tile_size, cap, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(),
                  table[4].data_ptr(), n_leaf.data_ptr(), labels.data_ptr(), ws.data_ptr(), ws_bytes)
        t = int(n_leaf.item())                               # the one sync per slide (cf. knn_grid's extent)
        if not 1 <= t <= cap:
            raise _lib.SeggerAmdError(f"segger_quadtree_build: {t} leaves for a capacity of {cap}")
        table = table[:, :t].clone()                         # (lets go of the capacity-sized buffer)
        self._tables[(dev, torch.int32)] = (table[0], table[1], table[3], table[4])
        self.labels = labels
        host = table[:3].long().cpu()
        return host[1], host[0], host[2]

    def _table(self, device: torch.device, dtype: torch.dtype) -> Tuple[Tensor, ...]:
        """(leaf prefix, leaf depth, Morton-ordered range start, leaf id of that range) on ``device``: int32 for the
        kernel, int64 for the torch path.  Copied once per device and type (the tree is tiny)."""
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        have = self._tables.get((device, dtype))
        if have is None:
            src = next(iter(self._tables.values()))
            have = self._tables[(device, dtype)] = tuple(t.to(device=device, dtype=dtype) for t in src)
        return have

    # ---- queries ---------------------------------------------------------------------------------------------
    def label(self, pos: Tensor) -> Tensor:
        """Leaf index of every point (any points, not only the build set): the leaf whose prefix matches the point's
        key -- half-open by construction, so a point on a shared border goes to the upper cell (deterministic, where the
        reference's ``intersects`` + ``drop_duplicates`` keeps whichever tile comes first in an unspecified order); -1
        outside the closed root box ``[x0, x1] x [y0, y1]`` and inside an empty quadrant.  Every build point gets a
        label >= 0."""
        if pos.is_cuda and pos.dtype == torch.float32:
            return self._label_device(pos.contiguous()).long()
        keys, depths, m_lo, m_id = self._table(pos.device, torch.long)
        key, inside = self._key(pos)
        j = torch.searchsorted(m_lo, key, right=True) - 1    # the last range start <= key
        lab = m_id[j.clamp(min=0)]
        hit = inside & (j >= 0) & ((key >> (2 * (self.depth - depths[lab]))) == keys[lab])
        return torch.where(hit, lab, torch.full_like(lab, -1))

    def _label_device(self, pos: Tensor) -> Tensor:
        from .. import _lib
        dev, n = pos.device, int(pos.shape[0])
        keys, depths, m_lo, m_id = self._table(dev, torch.int32)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return out
        _lib.call("segger_quadtree_label", dev, pos.data_ptr(), n, self.x0, self.y0, self.x1, self.y1, self.cell, self.depth,
                  keys.data_ptr(), depths.data_ptr(), m_lo.data_ptr(), m_id.data_ptr(), int(keys.numel()), out.data_ptr())
        return out

    def mask(self, pos: Tensor, margin: float) -> Tensor:
        """True where the point lies strictly inside its own leaf box shrunk by ``margin``; a margin that would make the
        smallest (clipped) leaf vanish is halved until every leaf survives (the rule of ``SquareTiling.mask``,
        tiling.py:103-127).  False for a point without a leaf (label -1)."""
        if margin < 0:
            raise ValueError(f"The margin must be non-negative, but got {margin}.")
        t = self.tiles
        w = torch.minimum(t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]).min().item()
        eff = float(margin)
        while eff > 0 and 2 * eff >= w:
            eff = eff / 2 if eff > 1e-6 else 0.0
        lab = self.label(pos)
        box = t.to(pos.device)[lab.clamp(min=0)]
        x, y = pos[:, 0].double(), pos[:, 1].double()
        return ((lab >= 0) & (x > box[:, 0] + eff) & (x < box[:, 2] - eff) & (y > box[:, 1] + eff) & (y < box[:, 3] - eff))
