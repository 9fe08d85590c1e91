"""Points in buffered polygons on the device: the reference's ``points_in_polygons``
(``src/segger/geometry/query.py:178-245``, a cuSpatial quadtree join) over ``polygons.buffer(d)``, which builds the
``("tx", "neighbors", "bd")`` prediction graph of the default ``prediction_graph_mode="cell"``
(``src/segger/data/utils/neighbors.py:223-238``).  There is no cuSpatial on ROCm; this is ``segger_polygon_join_count`` /
``segger_polygon_join_fill`` (csrc/polygon_join.hip; include/segger_amd.h has the contract).  There is no CPU path.

The predicate.  For a point ``t``, a ring ``P`` and a distance ``d >= 0``:

* ``parity(t, P)`` is the crossing-number test with the half-open rule: an edge ``(a, b)`` counts when
  ``a.y <= t.y < b.y`` or ``b.y <= t.y < a.y``, and the crossing lies strictly to the right of ``t``;
* ``dist2(t, P)`` is the smallest squared distance from ``t`` to a closed edge segment of the ring;
* ``contains``: ``dist2 < d*d or (parity and dist2 > 0)`` -- the open set: a point on the ring itself is out when
  ``d == 0`` and in when ``d > 0``;
* ``intersects``: ``dist2 <= d*d or parity`` -- the closed set, what the reference's
  ``ISTPreprocessor.assign_transcripts_to_boundaries`` uses through ``sjoin``.

float64 throughout, coordinates translated to the ring's first vertex before any product, FMA contraction off (cross
products of exactly representable coordinates are exact); either orientation; a closing duplicate vertex is dropped; a
ring with fewer than 3 vertices after that matches nothing under either predicate.  Polygons are single exterior rings,
as in :mod:`segger_amd.morphology`: no holes, no multi-part polygons.

This is the EXACT offset of the polygon (its Minkowski sum with a disc).  The reference's ``polygons.buffer(d)`` goes
through GEOS, which replaces each round corner by a polyline -- 16 segments per quarter circle is geopandas' default -- so
the two sets differ only in slivers at convex corners, at most ``d * (1 - cos(pi / 64))`` ~ ``0.0012 d`` wide: about
0.3 nm at the default ratio on a 10 um cell.

UNVERIFIED -- neither shapely nor GEOS could be imported where this was written, so the statement about GEOS's buffer
rests on knowledge of those libraries, not on a run.  GEOS's arc vertices are not reproduced.  What IS checked:
tests/polygon_join_cases.py holds a float64 and an exact rational oracle of the predicate above.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib as L
from .rings import raise_ring_errors, ring_csr

__all__ = ["points_in_polygons"]

_PREDICATES = {"contains": L.PJOIN_CONTAINS, "intersects": L.PJOIN_INTERSECTS}


def _empty(device) -> Tensor:
    return torch.empty(2, 0, dtype=torch.int64, device=device)


class JoinInputs(NamedTuple):
    """What the two units that walk points against grown rings (this one and :mod:`segger_amd.buffered_counts`) hand to
    their entry points: the tensors as the device code reads them, the sizes and the grid."""
    pts: Tensor
    ring_offsets: Tensor
    xy: Tensor
    buf: Optional[Tensor]
    n_points: int
    n_polygons: int
    n_vertices: int
    predicate: int
    grid: Tuple[float, float, float, int, int]                       # x0, y0, cell, nx, ny


def join_inputs(who: str, points: Tensor, ring_offsets: Tensor, xy: Tensor, buffer: Union[None, float, Tensor], predicate: str,
                points_per_cell: float, others: Tuple[Optional[Tensor], ...] = (), hint: str = "") -> Optional[JoinInputs]:
    """The argument checks, the ``buffer`` forms, the extent and finiteness synchronisation and the grid rule of
    :func:`points_in_polygons`, in the name of the caller ``who``; ``others`` are further tensors that must be on the
    device.  ``None``: no points, no polygons or no vertices -- nothing matches and nothing is launched."""
    if predicate not in _PREDICATES:
        raise ValueError(f"{who}: predicate {predicate!r} is neither 'contains' nor 'intersects'")
    if not isinstance(points, Tensor) or points.dim() != 2 or points.shape[1] != 2 or not points.is_floating_point():
        raise ValueError(f"{who}: points is a floating-point [n_points, 2] tensor")
    if not points_per_cell > 0 or not math.isfinite(points_per_cell):
        raise ValueError(f"{who}: points_per_cell must be positive and finite")
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    if points.device != xy.device:
        raise ValueError(f"{who}: points and the rings are on different devices")
    n_points = int(points.shape[0])
    if isinstance(buffer, Tensor):
        if buffer.dim() != 1 or buffer.numel() != n_polygons or not buffer.is_floating_point():
            raise ValueError(f"{who}: buffer is None, a float or a floating-point [n_polygons] tensor")
        if buffer.device != xy.device:
            raise ValueError(f"{who}: buffer and the rings are on different devices")
        buf: Optional[Tensor] = buffer.detach().to(torch.float64).contiguous()
    elif buffer is None:
        buf = None
    else:
        d = float(buffer)
        if not (d >= 0.0 and math.isfinite(d)):
            raise ValueError(f"{who}: buffer must be finite and >= 0, got {d}")
        buf = None if d == 0.0 else torch.full((n_polygons,), d, dtype=torch.float64, device=xy.device)
    if isinstance(buffer, Tensor) and not buf.is_cuda and n_polygons and not bool(((buf >= 0) & buf.isfinite()).all()):
        raise ValueError(f"{who}: buffer must be finite and >= 0")   # host tensors: refused before the device is asked for
    L.need_device(who, points, ring_offsets, xy, buf, *others, hint=hint)
    if n_points == 0 or n_polygons == 0:
        return None
    if n_vertices == 0:
        if bool((ring_offsets != 0).any()):
            raise ValueError(f"{who}: ring_offsets of polygon {int((ring_offsets[1:] != 0).nonzero()[0])} are negative, "
                             f"descending or beyond the 0 vertices")
        return None
    pts = points.detach().to(torch.float64).contiguous()

    # one synchronisation: the extent of the points, of the rings and of the buffer; a NaN anywhere is a NaN in its
    # minimum and maximum, an infinity is one of the two
    d_lo, d_hi = (buf.min(), buf.max()) if buf is not None else (pts.new_zeros(()), pts.new_zeros(()))
    ext = torch.cat([pts.min(0).values, pts.max(0).values, xy.min(0).values, xy.max(0).values, torch.stack([d_lo, d_hi])])
    px0, py0, px1, py1, rx0, ry0, rx1, ry1, d_lo, d_hi = ext.tolist()
    if not all(math.isfinite(v) for v in (px0, py0, px1, py1)):
        raise ValueError(f"{who}: points holds a non-finite coordinate")
    if not all(math.isfinite(v) for v in (rx0, ry0, rx1, ry1)):
        raise ValueError(f"{who}: xy holds a non-finite coordinate")
    if not (d_lo >= 0.0 and math.isfinite(d_hi)):
        raise ValueError(f"{who}: buffer must be finite and >= 0")
    x0, y0 = min(px0, rx0 - d_hi), min(py0, ry0 - d_hi)
    x1, y1 = max(px1, rx1 + d_hi), max(py1, ry1 + d_hi)
    w, h = max(x1 - x0, 1e-6), max(y1 - y0, 1e-6)
    cell = math.sqrt(w * h * points_per_cell / n_points)                               # knn_grid's rule
    cell = max(cell, math.sqrt(w * h / (4.0 * n_points)), max(w, h) / 30000.0)         # <= 4n cells, < 2^31 cells
    nx, ny = int(w / cell) + 1, int(h / cell) + 1
    return JoinInputs(pts, ring_offsets, xy, buf, n_points, n_polygons, n_vertices, _PREDICATES[predicate], (x0, y0, cell, nx, ny))


def points_in_polygons(points: Tensor, ring_offsets: Tensor, xy: Tensor, buffer: Union[None, float, Tensor] = None,
                       predicate: str = "contains", points_per_cell: float = 2.0) -> Tensor:
    """Every (point, polygon) pair with the point in the polygon grown by its ``buffer``.

    ``points`` is ``[N, 2]`` of any float dtype (converted to float64, exact for float32 positions); ``ring_offsets``
    ``[P + 1]`` and ``xy`` ``[V, 2]`` are the CSR of rings :func:`segger_amd.morphology.polygon_props` takes; ``buffer`` is
    ``None`` (0), a float, or a ``[P]`` tensor of distances ``>= 0``; ``predicate`` is ``"contains"`` or ``"intersects"``
    (the module docstring defines both).

    Returns an int64 ``[2, E]`` device tensor, row 0 the point id and row 1 the polygon id -- the reference's
    ``index_query`` and ``index_match`` -- sorted by (point, polygon), without duplicates, bit-identical from call to
    call and for any ``points_per_cell`` (the grid that bins the points decides the speed and nothing else; it follows
    :func:`segger_amd.neighbors.knn_grid`'s sizing rule over the union of the points' and the grown rings' extents).

    Raises ``ValueError`` for bad shapes or dtypes, an unknown predicate, a ring above ``SEGGER_MORPH_MAX_VERTS`` (naming
    the polygon), negative or non-finite ``buffer``, non-finite coordinates, and offsets the device found descending or out
    of range.  No polygons or no points gives ``[2, 0]`` and launches nothing.  Waits for the device four times: the
    longest ring (in the shared ring validation), the extent of the points and the rings together with the finiteness
    checks, the pair total, and the error word."""
    who = "points_in_polygons"
    j = join_inputs(who, points, ring_offsets, xy, buffer, predicate, points_per_cell,
                    hint="tests/polygon_join_cases.py holds the CPU oracle")
    if j is None:
        return _empty(xy.device)
    pts, ring_offsets, xy, buf, n_points, n_polygons, n_vertices = j[:7]
    dev = xy.device
    x0, y0, cell, nx, ny = j.grid

    ws, ws_bytes = L.workspace("segger_polygon_join_workspace_bytes", dev, n_points, n_polygons, nx, ny)
    pair_offsets = torch.empty(n_polygons + 1, dtype=torch.int64, device=dev)
    args = (pts.data_ptr(), n_points, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, L.ptr(buf),
            j.predicate, x0, y0, cell, nx, ny, pair_offsets.data_ptr())
    L.call("segger_polygon_join_count", dev, *args, ws.data_ptr(), ws_bytes)
    total = int(pair_offsets[-1])                                                       # the second synchronisation
    point_id = torch.empty(total, dtype=torch.int64, device=dev)
    if total > 0:
        L.call("segger_polygon_join_fill", dev, *args, point_id.data_ptr(), total, ws.data_ptr(), ws_bytes)
    raise_ring_errors(who, int(ws[:4].view(torch.int32)), ring_offsets, n_vertices)          # the third
    # polygon-major -> sorted by (point, polygon): within a point the stable sort keeps the polygons ascending
    polygon_id = torch.repeat_interleave(torch.arange(n_polygons, dtype=torch.int64, device=dev),
                                         pair_offsets[1:] - pair_offsets[:-1], output_size=total)
    point_id, order = torch.sort(point_id, stable=True)
    return torch.stack([point_id, polygon_id[order]])
