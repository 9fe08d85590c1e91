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

from typing import Dict

import torch
from torch import Tensor

from . import _lib as L
from .rings import raise_ring_errors, ring_csr, rings_from_padded

__all__ = ["polygon_props", "morphology_features", "rings_from_padded"]

_COLS = ("area", "hull_area", "rect_area", "envelope_area", "radius")


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
    ring_offsets, xy, n_polygons, n_vertices = ring_csr("polygon_props", ring_offsets, xy)
    L.need_device("polygon_props", ring_offsets, xy, hint="tests/morphology_cases.py holds the CPU oracle")
    dev = xy.device
    props = torch.empty(n_polygons, L.MORPH_COLS, dtype=torch.float64, device=dev)
    if n_polygons > 0:
        ws, ws_bytes = L.workspace("segger_morphology_workspace_bytes", dev, n_polygons)
        L.call("segger_polygon_props", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, props.data_ptr(),
               ws.data_ptr(), ws_bytes)
        raise_ring_errors("polygon_props", int(ws[:4].view(torch.int32)), ring_offsets, n_vertices)
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
