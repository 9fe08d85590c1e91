"""Graph construction on the device: kNN edges without leaving HBM.

Restates reference ``src/segger/data/utils/neighbors.py``:

* ``kdtree_neighbors`` (``:122-163``: scipy ``KDTree.query(k, distance_upper_bound)``, chunked, CPU)
  -> :func:`knn_grid` over the HIP kernel ``segger_knn_grid`` (exact, uniform grid);
* ``knn_to_edge_index`` (``:54-92``): dense neighbour table with padding -> COO ``edge_index`` whose
  row 0 is the QUERY point (source) and row 1 the neighbour (target);
* ``setup_transcripts_graph`` (``:166-180``) -> :func:`transcripts_graph`;
* ``setup_prediction_graph`` (``:200-241``): ``mode="uniform"`` -> :func:`prediction_graph_uniform`, the shape-based
  modes ``"cell"`` (the default) and ``"nucleus"`` -> :func:`prediction_graph_shape`; with the ``max_k`` the reference
  documents and its shape mode ignores -> ``prediction_graph_shape(..., max_k=...)`` and :func:`prediction_graph_nearest`.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib


def grid_rule(x0: float, y0: float, x1: float, y1: float, n: int, max_dist: float = math.inf,
              points_per_cell: float = 2.0) -> Tuple[float, int, int]:
    """The grid :func:`knn_grid` bins ``n`` points of the bounding box ``[x0, x1] x [y0, y1]`` into (host arithmetic
    only) -> ``(cell, nx, ny)``: about ``points_per_cell`` points per cell, a cell no wider than ``max_dist``, at most
    ``4n + O(sqrt n)`` cells and at most 30001 cells along an axis."""
    w, h = max(x1 - x0, 1e-6), max(y1 - y0, 1e-6)
    cell = math.sqrt(w * h * points_per_cell / n)
    if math.isfinite(max_dist):
        cell = min(cell, max_dist)
    cell = max(cell, math.sqrt(w * h / (4.0 * n)), max(w, h) / 30000.0)              # <= 4n cells, < 2^31 cells
    return cell, int(w / cell) + 1, int(h / cell) + 1


def knn_grid(points: Tensor, k: int, max_dist: float = math.inf, query: Optional[Tensor] = None,
             return_dist: bool = False, points_per_cell: float = 2.0) -> Tuple[Tensor, Optional[Tensor]]:
    """Neighbour table ``[m, k]`` (int32; ids into ``points`` sorted by distance; ``len(points)`` = padding).
    ``max_dist`` is a strict bound, as scipy's ``distance_upper_bound`` is: a point at exactly ``max_dist`` (in float32)
    is not a neighbour."""
    _lib.require_cuda(points)
    dev = points.device
    pts = points.to(torch.float32).contiguous()
    q = pts if query is None else query.to(device=dev, dtype=torch.float32).contiguous()
    n, m = int(pts.shape[0]), int(q.shape[0])
    nbr = torch.empty((m, k), dtype=torch.int32, device=dev)
    dist = torch.empty((m, k), dtype=torch.float32, device=dev) if return_dist else None
    if m == 0:
        return nbr, dist
    if n == 0:
        nbr.fill_(0)
        if dist is not None:
            dist.fill_(math.inf)
        return nbr, dist
    both = pts if query is None else torch.cat([pts, q])
    lo, hi = both.min(0).values, both.max(0).values
    x0, y0, x1, y1 = (float(v) for v in torch.stack([lo, hi]).flatten().tolist())    # one host sync per graph
    cell, nx, ny = grid_rule(x0, y0, x1, y1, n, max_dist, points_per_cell)
    ws, ws_bytes = _lib.workspace("segger_knn_workspace_bytes", dev, n, nx, ny)
    _lib.call("segger_knn_grid", dev, pts.data_ptr(), n, None if query is None else q.data_ptr(), m, k, float(max_dist),
              x0, y0, cell, nx, ny, nbr.data_ptr(), _lib.ptr(dist), ws.data_ptr(), ws_bytes)
    return nbr, dist


def knn_to_edge_index(neighbor_table: Tensor, padding_value: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """Dense ``[N, K]`` neighbour table -> ``(edge_index [2, E] int64, index_ptr [N + 1])``; entries equal to the
    padding value (default N) are dropped; edges keep row-major order (query 0's neighbours first)."""
    n, k = neighbor_table.shape
    if padding_value is None:
        padding_value = n
    valid = neighbor_table != padding_value
    flat = valid.reshape(-1).nonzero(as_tuple=False).squeeze(1)
    col = neighbor_table.reshape(-1)[flat].long()
    row = torch.div(flat, k, rounding_mode="floor")
    deg = valid.sum(1)
    indptr = torch.cat([deg.new_zeros(1), deg.cumsum(0)])
    return torch.stack([row, col]), indptr


def transcripts_graph(pos: Tensor, max_k: int, max_dist: float = math.inf) -> Tensor:
    """``tx-neighbors-tx`` edges: every transcript -> its ``max_k`` nearest transcripts (itself included)
    within ``max_dist``."""
    nbr, _ = knn_grid(pos, max_k, max_dist)
    ei, _ = knn_to_edge_index(nbr, padding_value=int(pos.shape[0]))
    return ei


def prediction_graph_uniform(tx_pos: Tensor, bd_pos: Tensor, max_k: int, max_dist: float = math.inf) -> Tensor:
    """``setup_prediction_graph(mode='uniform')`` (``neighbors.py:213-221``): kNN from boundary centroids
    (queries) into the transcripts (points); row 0 = query (boundary) id, row 1 = transcript id.  For polygon boundaries
    ``segger_amd.morphology.polygon_props(ring_offsets, xy)["centroid"]`` is the reference's ``bd.geometry.centroid``."""
    nbr, _ = knn_grid(tx_pos, max_k, max_dist, query=bd_pos)
    ei, _ = knn_to_edge_index(nbr, padding_value=int(tx_pos.shape[0]))
    return ei


def _nearest_edges(tx_pos: Tensor, ring_offsets: Tensor, xy: Tensor, max_k: int, buffer, predicate: str) -> Tensor:
    """the kept candidates of :func:`segger_amd.nearest.nearest_boundaries` as a ``[2, E]`` int64 edge index sorted by
    (transcript, polygon)"""
    from .nearest import nearest_boundaries
    polygon = nearest_boundaries(tx_pos, ring_offsets, xy, max_k, buffer=buffer, predicate=predicate)["polygon"]
    n_polygons = int(ring_offsets.numel()) - 1
    polygon = polygon.long().sort(dim=1).values                      # the padding, n_polygons, sorts last
    keep = polygon != n_polygons
    row = torch.arange(polygon.shape[0], device=polygon.device).unsqueeze(1).expand_as(polygon)
    return torch.stack([row[keep], polygon[keep]])


def prediction_graph_nearest(tx_pos: Tensor, ring_offsets: Tensor, xy: Tensor, max_k: int = 3, max_dist: float = 1.0,
                             predicate: str = "intersects") -> Tensor:
    """The prediction graph with a bounded degree: every transcript -> its ``max_k`` best boundaries among the polygons
    grown by ``max_dist`` that hold it -- the reference's documented ``prediction_graph_max_k = 3`` and
    ``prediction_graph_max_dist = 1.0`` (``data/data_module.py:110-115``), upstream segger's ``k_bd`` / ``dist_bd``, on polygon
    boundaries instead of centroids (:func:`prediction_graph_uniform` is wrong for elongated cells).  "Best" is
    :func:`segger_amd.nearest.nearest_boundaries`' order: the polygons the transcript is inside, deepest first, then the
    nearest ones outside, ties to the lower id.

    Returns the ``TX_NB_BD`` edge index ``[2, E]`` int64, row 0 the transcript and row 1 the polygon, sorted by
    (transcript, polygon) as :func:`prediction_graph_shape`'s; at most ``max_k`` edges a transcript.  ``max_k`` is
    ``1 .. SEGGER_NEAREST_MAX_K``; ``max_dist`` is a uniform buffer ``>= 0`` (negative: ``ValueError``; erosion is a mask
    over ``nearest_boundaries``' ``inside`` and ``dist2``, see :mod:`segger_amd.nearest`)."""
    return _nearest_edges(tx_pos, ring_offsets, xy, max_k, float(max_dist), predicate)


def prediction_graph_shape(tx_pos: Tensor, ring_offsets: Tensor, xy: Tensor, buffer_ratio: float = 0.05,
                           max_k: Optional[int] = None) -> Tensor:
    """``setup_prediction_graph(mode='cell' | 'nucleus')`` (``neighbors.py:223-238``), the reference's default
    (``ISTDataModule.prediction_graph_mode = "cell"``, ``prediction_graph_buffer_ratio = 0.05``): every boundary polygon
    is grown by ``d = sqrt(area / pi) * buffer_ratio`` and every transcript is joined to every grown polygon that contains
    it.  ``area`` comes from :func:`segger_amd.morphology.polygon_props` and ``d`` is float64 torch; the join is
    :func:`segger_amd.geometry.points_in_polygons` with ``predicate="contains"``, whose docstring says where the exact
    offset used here differs from GEOS's ``buffer`` (slivers at convex corners ~ 0.0012 d wide; unverified against GEOS).

    ``tx_pos`` is ``[N, 2]`` (float32 positions are converted to float64, which is exact); ``ring_offsets`` / ``xy`` are
    the CSR of rings.  Returns the ``TX_NB_BD`` edge index ``[2, E]`` int64 in the reference's direction: row 0 the
    transcript (``index_query``), row 1 the polygon (``index_match``), sorted by (transcript, polygon).

    The reference selects the rows of one ``boundary_type`` (cell or nucleus) before the call -- pass only those rings --
    and ignores ``max_k`` in this mode: ``max_k=None``, the default, does the same and every transcript gets as many edges
    as there are grown polygons over it.  An int (``1 .. SEGGER_NEAREST_MAX_K``) caps each transcript at its ``max_k`` best
    among the grown polygons, in :func:`segger_amd.nearest.nearest_boundaries`' order (deepest inside first, then nearest
    outside, ties to the lower id), which bounds the shape buckets of :class:`segger_amd.capture.GraphedPredictorPool`.
    ``buffer_ratio < 0`` is a ``ValueError``: GEOS's erosion (a negative buffer) is not built as geometry; membership in
    an eroded polygon is the mask ``inside & (dist2 >= d * d)`` over ``nearest_boundaries``' result
    (:mod:`segger_amd.nearest`)."""
    from .geometry import points_in_polygons
    from .morphology import polygon_props
    buffer_ratio = float(buffer_ratio)
    if not (buffer_ratio >= 0.0 and math.isfinite(buffer_ratio)):
        raise ValueError(f"prediction_graph_shape: buffer_ratio must be finite and >= 0 (erosion is not built), got {buffer_ratio}")
    area = polygon_props(ring_offsets, xy)["area"]
    d = torch.sqrt(area / math.pi) * buffer_ratio
    d = torch.where(area.isnan(), torch.zeros_like(d), d)           # an empty ring has no area and matches nothing
    if max_k is not None:
        return _nearest_edges(tx_pos, ring_offsets, xy, max_k, d, "contains")
    return points_in_polygons(tx_pos, ring_offsets, xy, buffer=d, predicate="contains")
