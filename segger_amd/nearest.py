"""Nearest boundaries on the device: for every point the ``k`` best of the polygons that
:func:`segger_amd.geometry.points_in_polygons` pairs it with, each with its squared distance to the ring and the crossing
parity -- the two numbers the join's predicate computes and folds into one bit.  This is
``segger_nearest_boundaries_count`` / ``_fill`` / ``_select`` (csrc/nearest_boundaries.hip; include/segger_amd.h has the
contract).  There is no CPU path.

What reads them:

* a prediction graph with a bounded degree (:func:`segger_amd.neighbors.prediction_graph_nearest`, and
  ``prediction_graph_shape(..., max_k=...)``): the reference documents ``prediction_graph_max_k`` ("maximum number of edges
  per transcript for prediction graphs", ``data/data_module.py:110-115``) and ignores it in its shape mode
  (``data/utils/neighbors.py:223-238``); "the k nearest boundaries within a distance" is upstream segger's ``k_bd`` /
  ``dist_bd``;
* the signed distance of a transcript to an outline, :func:`signed_distance`: negative inside, positive outside;
* EROSION, as a mask the caller writes: a point lies in a polygon shrunk by ``d`` exactly when
  ``result["inside"] & (result["dist2"] >= d * d)`` (closed; ``>`` for the open set) -- call with ``buffer=None`` and a
  ``k`` at least the overlap depth of the polygons (``count`` says whether it was).

The candidates are the join's pairs bit for bit: both kernels compile csrc/ring_predicate.h, and
:mod:`segger_amd.geometry`'s docstring defines the predicate and says how the exact offset differs from GEOS's buffer.

NOT BUILT: GEOS's eroded geometry as rings (``buffer(-d)``: only the membership mask above); holes and multi-part
polygons; ``k`` above ``SEGGER_NEAREST_MAX_K``; capture into :class:`segger_amd.capture.GraphedPredictorPool` (the
wrapper waits for the device to size the candidate list).  UNPINNED: the reference has no counterpart to run; what IS
checked is equality with the CPU oracle of tests/nearest_cases.py, built on the join's float64 oracle.
"""
from __future__ import annotations

from typing import Dict, Union

import torch
from torch import Tensor

from . import _lib as L
from .geometry import join_inputs
from .rings import raise_ring_errors

__all__ = ["COUNTER_NAMES", "nearest_boundaries", "signed_distance"]

COUNTER_NAMES = ("n_pairs", "n_kept", "n_truncated_points", "max_count")


def _padded(n_points: int, n_polygons: int, k: int, device) -> Dict[str, Tensor]:
    return {"polygon": torch.full((n_points, k), n_polygons, dtype=torch.int32, device=device),
            "dist2": torch.full((n_points, k), float("inf"), dtype=torch.float64, device=device),
            "inside": torch.zeros((n_points, k), dtype=torch.bool, device=device),
            "count": torch.zeros(n_points, dtype=torch.int32, device=device),
            "counters": torch.zeros(len(COUNTER_NAMES), dtype=torch.int64, device=device)}


def nearest_boundaries(points: Tensor, ring_offsets: Tensor, xy: Tensor, k: int, buffer: Union[None, float, Tensor] = None,
                       predicate: str = "intersects", points_per_cell: float = 2.0) -> Dict[str, Tensor]:
    """The ``k`` best boundaries of every point among the polygons grown by ``buffer`` that hold it.

    ``points`` ``[N, 2]``, ``ring_offsets`` ``[P + 1]``, ``xy`` ``[V, 2]``, ``buffer`` (``None``, a float, a ``[P]`` tensor),
    ``predicate`` and ``points_per_cell`` are :func:`segger_amd.geometry.points_in_polygons`'; the checks and their messages
    are that function's.  ``1 <= k <= SEGGER_NEAREST_MAX_K`` (16), else ``ValueError``.

    The CANDIDATES of a point are the polygons ``points_in_polygons(points, ring_offsets, xy, buffer, predicate)`` pairs it
    with.  With ``parity`` and ``dist2`` as that module defines them, the key of a candidate is
    ``s = 0 if dist2 == 0 else (-dist2 if parity else dist2)``, and candidates are ordered by ``(s, polygon id)``
    ascending: deeper inside first, then nearer outside; ties (duplicate polygons, a point on two rings) go to the lower id.

    Returns a dict of device tensors, the same bytes from call to call, for any ``points_per_cell``, any order of the
    points and -- after mapping the ids -- any order of the polygons:

    * ``polygon`` int32 ``[N, k]``: the ids in key order, padded with ``P`` (as :func:`segger_amd.neighbors.knn_grid` pads
      with ``N``);
    * ``dist2`` float64 ``[N, k]``: the squared distance to the ring itself (not to the grown ring), padded with ``+inf``;
    * ``inside`` bool ``[N, k]``: the parity, padded with ``False``;
    * ``count`` int32 ``[N]``: the candidates BEFORE the cap, so ``count > k`` marks a truncated point;
    * ``counters`` int64, named by ``COUNTER_NAMES``: ``n_pairs`` (the join's pair total), ``n_kept``,
      ``n_truncated_points``, ``max_count``.

    No points or no polygons returns the padded tensors and launches nothing; CPU tensors raise ``SeggerAmdError``.  Waits
    for the device four times: the longest ring (the shared ring validation), the extent of the points and the rings with
    the finiteness checks, the pair total, and the error word.  Memory beyond the result: the join's workspace, 8 bytes a
    point of offsets and 12 bytes a candidate pair."""
    who = "nearest_boundaries"
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= L.NEAREST_MAX_K:
        raise ValueError(f"{who}: k is an int in 1 .. SEGGER_NEAREST_MAX_K = {L.NEAREST_MAX_K}, got {k!r}")
    j = join_inputs(who, points, ring_offsets, xy, buffer, predicate, points_per_cell,
                    hint="tests/nearest_cases.py holds the CPU oracle")
    dev = xy.device
    if j is None:
        return _padded(int(points.shape[0]), int(ring_offsets.numel()) - 1, k, dev)
    pts, ring_offsets, xy, buf, n_points, n_polygons, n_vertices = j[:7]
    ws, ws_bytes = L.workspace("segger_nearest_boundaries_workspace_bytes", dev, n_points, n_polygons, j.grid[3], j.grid[4])
    pair_offsets = torch.empty(n_points + 1, dtype=torch.int64, device=dev)
    head = (pts.data_ptr(), n_points, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, L.ptr(buf), j.predicate,
            *j.grid, pair_offsets.data_ptr())
    L.call("segger_nearest_boundaries_count", dev, *head, ws.data_ptr(), ws_bytes)
    total = int(pair_offsets[-1])                                    # the third wait
    pair_key = torch.empty(total, dtype=torch.float64, device=dev)
    pair_polygon = torch.empty(total, dtype=torch.int32, device=dev)
    if total > 0:
        L.call("segger_nearest_boundaries_fill", dev, *head, pair_key.data_ptr(), pair_polygon.data_ptr(), total, ws.data_ptr(), ws_bytes)
    out = {"polygon": torch.empty((n_points, k), dtype=torch.int32, device=dev),
           "dist2": torch.empty((n_points, k), dtype=torch.float64, device=dev),
           "inside": torch.empty((n_points, k), dtype=torch.bool, device=dev),
           "count": torch.empty(n_points, dtype=torch.int32, device=dev),
           "counters": torch.empty(len(COUNTER_NAMES), dtype=torch.int64, device=dev)}
    L.call("segger_nearest_boundaries_select", dev, pair_offsets.data_ptr(), L.ptr(pair_key if total else None),
           L.ptr(pair_polygon if total else None), total, n_points, n_polygons, k, out["polygon"].data_ptr(), out["dist2"].data_ptr(),
           out["inside"].data_ptr(), out["count"].data_ptr(), out["counters"].data_ptr())
    raise_ring_errors(who, int(ws[:4].view(torch.int32)), ring_offsets, n_vertices)          # the fourth
    return out


def signed_distance(result: Dict[str, Tensor]) -> Tensor:
    """``[N, k]`` float64 from what :func:`nearest_boundaries` returns: ``-sqrt(dist2)`` where ``inside``, ``+sqrt(dist2)``
    elsewhere, ``+inf`` in the padding.  Column 0 is the signed distance of a point to its best boundary: how deep inside,
    or how far outside.  Plain torch."""
    d = torch.sqrt(result["dist2"])
    return torch.where(result["inside"], -d, d)
