"""Boundary morphology features on the device: the reference's ``get_polygon_props``
(``src/segger/geometry/morphology.py:4-43``), stacked into ``ad.obsm['X_morphology']`` at
``src/segger/data/utils/anndata.py:296-311`` and used as ``bd.x`` when ``cells_representation="morphology"``.

With ``P`` a polygon, ``H`` its convex hull, ``B`` its axis-aligned bounding box, ``R`` its minimum-area enclosing
rectangle of any orientation and ``r`` the radius of its smallest enclosing circle, the four columns are

    area = area(P)    convexity = area(H) / area(P)    elongation = area(R) / area(B)    circularity = area(P) / r^2

as float32, rounded once from float64.  The reference computes them on the CPU through geopandas / shapely, one polygon at
a time; here one wave owns one polygon (``segger_polygon_props``, csrc/morphology.hip; include/segger_amd.h has the
arithmetic, the hull's tie rules and the degenerate cases).  Divisions follow IEEE as numpy / pandas do: ``x / 0`` is
``+-inf``, ``0 / 0`` is ``nan``; nothing is clamped.  There is no CPU path.

UNVERIFIED -- neither shapely nor GEOS could be imported where this was written, so two statements about shapely 2.1.2
and its bundled GEOS rest on knowledge of those libraries, not on a run:

* ``minimum_rotated_rectangle()`` is the true minimum-area rectangle, which has one side collinear with a hull edge;
* ``minimum_bounding_radius()`` is the radius of the exact smallest enclosing circle.

All four quantities are unique geometric values, so if the two statements hold, any exact algorithm agrees with GEOS to
rounding.  What IS checked: tests/morphology_cases.py holds a float64 and an exact rational oracle, pinned to
``scipy.spatial.ConvexHull`` for the hull.

Polygons are single exterior rings: no holes, no multi-part polygons, no buffering.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
from torch import Tensor

from . import _lib as L

__all__ = ["polygon_props", "morphology_features", "rings_from_padded"]

_COLS = ("area", "hull_area", "rect_area", "envelope_area", "radius")


def _rings(ring_offsets: Tensor, xy: Tensor) -> Tuple[Tensor, Tensor, int, int]:
    if not isinstance(ring_offsets, Tensor) or not isinstance(xy, Tensor):
        raise ValueError("polygon_props: ring_offsets and xy are tensors")
    if ring_offsets.dim() != 1 or ring_offsets.numel() < 1 or ring_offsets.dtype not in (torch.int64, torch.int32):
        raise ValueError("polygon_props: ring_offsets is an int64 (or int32) vector of n_polygons + 1 entries")
    if xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_floating_point():
        raise ValueError("polygon_props: xy is a floating-point [n_vertices, 2] tensor")
    if ring_offsets.device != xy.device:
        raise ValueError("polygon_props: ring_offsets and xy are on different devices")
    n_polygons, n_vertices = int(ring_offsets.numel()) - 1, int(xy.shape[0])
    ring_offsets = ring_offsets.detach().to(torch.int64).contiguous()
    xy = xy.detach().to(torch.float64).contiguous()
    if n_polygons > 0:
        # the cap is refused here, before the call: the ring lengths are device memory the C entry point cannot read
        # without a synchronisation (a closing duplicate vertex does not count, hence the + 1)
        longest, where = (ring_offsets[1:] - ring_offsets[:-1]).max(dim=0)
        longest, where = int(longest), int(where)
        if longest > L.MORPH_MAX_VERTS + 1 or (longest == L.MORPH_MAX_VERTS + 1 and not torch.equal(
                xy[int(ring_offsets[where])], xy[int(ring_offsets[where + 1]) - 1])):
            raise ValueError(f"polygon_props: polygon {where} has {longest} vertices, more than SEGGER_MORPH_MAX_VERTS = "
                             f"{L.MORPH_MAX_VERTS}")
    return ring_offsets, xy, n_polygons, n_vertices


def polygon_props(ring_offsets: Tensor, xy: Tensor) -> Dict[str, Tensor]:
    """The geometry of every ring of a CSR of polygons: ``ring_offsets`` ``[P + 1]`` int64 and ``xy`` ``[V, 2]`` (any float
    dtype, converted to float64) on the device; polygon ``p`` is ``xy[ring_offsets[p]:ring_offsets[p + 1]]``, either
    orientation, with or without a closing duplicate of its first vertex.

    Returns float64 device tensors ``area``, ``hull_area``, ``rect_area``, ``envelope_area``, ``radius`` ``[P]``, the four
    ratios ``convexity``, ``elongation``, ``circularity`` (plain torch divisions of those) next to ``area``, ``centroid``
    ``[P, 2]`` (the reference's ``bd.geometry.centroid``), ``bounds`` ``[P, 4]`` (xmin, ymin, xmax, ymax) and ``n_hull``
    int32.  An empty ring gives ``nan``; one with 1 or 2 vertices, or only collinear ones, gives zero areas and half its
    extent as ``radius``.  Raises ``ValueError`` for bad shapes or dtypes, for a ring above ``SEGGER_MORPH_MAX_VERTS``
    (naming the polygon, before anything is launched) and for offsets the device found descending or out of range.  Waits
    for the device twice (the longest ring, the error word)."""
    ring_offsets, xy, n_polygons, n_vertices = _rings(ring_offsets, xy)
    L.need_device("polygon_props", ring_offsets, xy, hint="tests/morphology_cases.py holds the CPU oracle")
    dev = xy.device
    props = torch.empty(n_polygons, L.MORPH_COLS, dtype=torch.float64, device=dev)
    if n_polygons > 0:
        ws, ws_bytes = L.workspace("segger_morphology_workspace_bytes", dev, n_polygons)
        L.call("segger_polygon_props", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, props.data_ptr(),
               ws.data_ptr(), ws_bytes)
        flag = int(ws[:4].view(torch.int32))
        if flag & L.MORPH_ERR_OFFSETS:
            bad = (ring_offsets[:-1] < 0) | (ring_offsets[1:] < ring_offsets[:-1]) | (ring_offsets[1:] > n_vertices)
            raise ValueError(f"polygon_props: ring_offsets of polygon {int(bad.nonzero()[0])} are negative, descending or beyond "
                             f"the {n_vertices} vertices")
        if flag:
            raise ValueError(f"polygon_props: the device reported error word {flag}")
    out = {name: props[:, c] for c, name in enumerate(_COLS)}
    out["convexity"] = out["hull_area"] / out["area"]
    out["elongation"] = out["rect_area"] / out["envelope_area"]
    out["circularity"] = out["area"] / out["radius"] ** 2
    out["centroid"] = props[:, 5:7]
    out["bounds"] = props[:, 7:11]
    n_hull = props[:, 11]
    out["n_hull"] = torch.where(n_hull.isnan(), torch.zeros_like(n_hull), n_hull).to(torch.int32)
    return out


def morphology_features(ring_offsets: Tensor, xy: Tensor, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """The reference's ``X_morphology`` ``[P, 4]``: ``area``, ``convexity``, ``elongation``, ``circularity`` in the
    reference's order, rounded once from float64 to ``out_dtype``.  With ``bd_in_channels=4`` this is ``bd.x`` of
    ``cells_representation="morphology"``."""
    p = polygon_props(ring_offsets, xy)
    return torch.stack([p["area"], p["convexity"], p["elongation"], p["circularity"]], dim=1).to(out_dtype)


def rings_from_padded(vertices: Tensor, counts: Tensor) -> Tuple[Tensor, Tensor]:
    """``(ring_offsets, xy)`` from padded rings: ``vertices`` ``[P, L, 2]`` of which row ``p`` uses its first
    ``counts[p]`` entries (Xenium's boundaries are fixed 13- or 25-vertex rings).  Plain torch on the tensors' device."""
    if vertices.dim() != 3 or vertices.shape[2] != 2 or counts.dim() != 1 or counts.numel() != vertices.shape[0]:
        raise ValueError("rings_from_padded: vertices is [P, L, 2] and counts [P]")
    counts = counts.to(torch.int64)
    if counts.numel() and (int(counts.min()) < 0 or int(counts.max()) > vertices.shape[1]):
        raise ValueError("rings_from_padded: counts outside 0 .. L")
    ring_offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=vertices.device)
    torch.cumsum(counts, 0, out=ring_offsets[1:])
    used = torch.arange(vertices.shape[1], device=vertices.device)[None, :] < counts[:, None]
    return ring_offsets, vertices[used]
