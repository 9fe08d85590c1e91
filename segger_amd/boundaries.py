"""Cell boundary polygons on the device: one ring per segmented cell, the convex hull of the cell's transcripts -- the
``boundaries`` element of the reference's ``segger export`` (``src/segger/cli/export.py:18-19,119-124``), built by
``generate_boundaries`` / ``cell_boundary`` (``src/segger/export/boundary.py:157-217``) in a Python loop with one shapely
call per cell.  Here one wave owns one cell (``segger_cell_boundaries``, csrc/boundaries.hip; include/segger_amd.h has the
stages, the march's tie rules and the arithmetic).  There is no CPU path.

What is built is the reference's ``method="convex_hull"``, with its rule for degenerate cells (fewer than 3 distinct
points, or only collinear ones: no polygon, the cell is dropped), the optional Chaikin smoothing (``boundary.py:42-54``) and
``n_transcripts`` per cell.

The reference's DEFAULT, ``method="delaunay"`` (``boundary.py:57-154``: the outline of a pruned Delaunay triangulation), is
built as entry points of its own, :func:`cell_outlines` and :func:`segmentation_outlines` (``segger_cell_outlines``,
csrc/outlines.hip; one single-wave workgroup owns one cell).  NOT BUILT: the ``method="delaunay"`` SPELLING on
:func:`cell_boundaries`, which still raises ``NotImplementedError`` -- that function returns the convex outline that
``segger export --method convex_hull`` writes; cells above ``SEGGER_OUTLINE_MAX_POINTS`` distinct points unless
``large_cells="global"`` is passed (a route through global memory, csrc/outlines_large.hip); GEOS's order
among components of equal area; ``buffer(0)`` repairs of a smoothed concave ring.

The rings come back as the ring CSR of :mod:`segger_amd.rings`, open (no closing duplicate), counter-clockwise from the
lexicographically lowest vertex: :func:`segger_amd.morphology.polygon_props` and
:func:`segger_amd.geometry.points_in_polygons` take them as they are.  Shapely orients and starts its hull ring
differently; the polygon is the same.

UNVERIFIED -- shapely could not be imported where this was written, so two statements about it rest on knowledge of the
library, not on a run: ``MultiPoint(points).convex_hull`` is a ``Polygon`` exactly when the points are not all collinear
(otherwise a ``LineString`` or ``Point``, which ``_as_polygon`` turns into ``None``), and ``.buffer(0)`` after the
smoothing leaves a ring unchanged that is already valid -- Chaikin's corner cutting keeps a convex ring convex.  What IS
checked: tests/boundaries_cases.py holds an exact-arithmetic hull oracle pinned to ``scipy.spatial.ConvexHull``, and the
smoothing is compared bit for bit with the numpy iteration the reference writes.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L

__all__ = ["cell_boundaries", "segmentation_boundaries", "cell_outlines", "segmentation_outlines"]

METHODS = ("convex_hull", "delaunay")
COUNTERS = ("n_counted", "n_present", "n_kept", "n_vertices", "n_bad_cell", "n_non_finite", "n_refused", "refused_cell")
OUTLINE_COUNTER_NAMES = COUNTERS + ("n_failed", "failed_cell")
LARGE_OUTLINE_COUNTER_NAMES = OUTLINE_COUNTER_NAMES + ("n_large_cells", "n_large_points", "n_large_rows")
LARGE_CELLS = ("refuse", "global")
MAX_ROWS = (1 << 31) - 2


def _check_options(who: str, smoothing, method) -> int:
    if method not in METHODS:
        raise ValueError(f"{who}: method {method!r} is neither 'convex_hull' nor 'delaunay'")
    if method == "delaunay":
        raise NotImplementedError(f"{who}: method='delaunay', the reference's default (src/segger/export/boundary.py:57-154, a "
                                  f"sequential pruning of a Delaunay triangulation), is not built; use method='convex_hull'")
    return _check_smoothing(who, smoothing)


def _oracle_hint(who: str) -> str:
    return f"tests/{'outline' if who.endswith('outlines') else 'boundaries'}_cases.py holds the CPU oracle"


def _check_smoothing(who: str, smoothing) -> int:
    if isinstance(smoothing, bool) or not isinstance(smoothing, int) or not 0 <= smoothing <= L.BOUNDARY_MAX_SMOOTHING:
        raise ValueError(f"{who}: smoothing must be an int in 0 .. {L.BOUNDARY_MAX_SMOOTHING} (Chaikin iterations; each doubles "
                         f"the vertices), got {smoothing!r}")
    return smoothing


def cell_boundaries(xy: Tensor, cell: Tensor, n_cells: Optional[int] = None, *, keep: Optional[Tensor] = None,
                    smoothing: int = 0, method: str = "convex_hull") -> Dict[str, Tensor]:
    """The boundary polygon of every cell: the convex hull of its transcripts, after ``smoothing`` Chaikin iterations.

    ``xy`` is ``[N, 2]`` (any float dtype, converted to float64) and ``cell`` ``[N]`` (any integer dtype) on the device;
    ``keep`` is an optional ``[N]`` mask.  Row ``i`` is counted iff ``0 <= cell[i] < n_cells`` and ``keep[i]`` is true.  A
    negative id means unassigned and is skipped, as is everything about a row with ``keep[i]`` false.  ``n_cells`` is the
    id domain; it defaults to ``max(cell) + 1`` (one more wait for the device).

    Returns device tensors for the ``K`` cells that got a polygon, in ascending cell id:

    * ``ring_offsets`` int64 ``[K + 1]`` and ``xy`` float64 ``[V, 2]``: the ring CSR, rings open and counter-clockwise from
      their lowest (x, then y) vertex; a hull vertex is an input coordinate bit for bit (``-0.0`` comes back as ``+0.0``), a
      point on a hull edge or equal to another point is never a vertex; with ``smoothing = s`` a ring of ``h`` hull vertices
      has ``h * 2**s``, with the bits of the reference's ``_chaikin`` on the hull;
    * ``cell_ids`` int32 ``[K]``, ``n_transcripts`` int64 ``[K]`` (counted rows, duplicates included);
    * ``n_dropped`` (a Python int): cells with a counted row but no polygon -- fewer than 3 distinct points, or all
      collinear (the reference returns ``None`` for them and drops the row).

    The same rows in any order give the same bytes (include/segger_amd.h says when a rounded orientation test can break
    that: never for coordinates on an integer grid below 2^25).  Waits for the device once, to read the counters.

    Raises ``ValueError`` for bad shapes, dtypes or options, ``NotImplementedError`` for ``method="delaunay"``, and
    ``SeggerAmdError`` when a kept row has a cell id ``>= n_cells`` or a non-finite coordinate (such a row is used nowhere;
    the other rows of its cell were hulled without it, but nothing is returned), or when a cell above
    ``SEGGER_MORPH_MAX_VERTS`` points kept a running hull above ``SEGGER_BOUNDARY_CHUNK_MAX_HULL`` vertices (the cell is
    named)."""
    who = "cell_boundaries"
    smoothing = _check_options(who, smoothing, method)
    dev, pts, ids, mask, n, n_cells = _rows(who, xy, cell, n_cells, keep)
    capacity, ring_offsets, out, cell_ids, n_tx, counters = _outputs(dev, n, n_cells, smoothing, L.BOUNDARY_COUNTERS)
    if n:
        ws, ws_bytes = L.workspace("segger_cell_boundaries_workspace_bytes", dev, n, n_cells)
        L.call("segger_cell_boundaries", dev, pts.data_ptr(), ids.data_ptr(), L.ptr(mask), n, n_cells, smoothing,
               ring_offsets.data_ptr(), out.data_ptr(), capacity, cell_ids.data_ptr(), n_tx.data_ptr(), counters.data_ptr(),
               ws.data_ptr(), ws_bytes)
        del ws
    c = dict(zip(COUNTERS, counters.tolist()))               # the one wait for the device
    _raise_for_rows(who, c, n_cells)
    if c["n_refused"]:
        raise L.SeggerAmdError(f"{who}: {c['n_refused']} cells of more than {L.MORPH_MAX_VERTS} transcripts kept a running hull "
                               f"above {L.BOUNDARY_CHUNK_MAX_HULL} vertices (SEGGER_BOUNDARY_CHUNK_MAX_HULL) while points "
                               f"remained, cell {c['refused_cell'] - 1} among them; such a cell gets no polygon")
    return _result(c, capacity, ring_offsets, out, cell_ids, n_tx)


def _rows(who: str, xy, cell, n_cells, keep):
    """the checks and conversions of the rows both entry points take -> (device, xy float64, ids int32, mask, n, n_cells)"""
    if not isinstance(xy, Tensor) or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_floating_point():
        raise ValueError(f"{who}: xy is a floating-point [n_rows, 2] tensor")
    if not isinstance(cell, Tensor) or cell.dim() != 1 or cell.is_floating_point() or cell.dtype == torch.bool:
        raise ValueError(f"{who}: cell is an integer [n_rows] tensor")
    n = _n_rows(who, int(xy.shape[0]))
    if int(cell.numel()) != n or (keep is not None and (not isinstance(keep, Tensor) or keep.dim() != 1 or int(keep.numel()) != n)):
        raise ValueError(f"{who}: xy, cell and keep have different numbers of rows")
    if cell.device != xy.device or (keep is not None and keep.device != xy.device):
        raise ValueError(f"{who}: xy, cell and keep are on different devices")
    if n_cells is not None and not 1 <= int(n_cells) < (1 << 31):
        raise ValueError(f"{who}: n_cells must be in 1 .. 2^31 - 1, got {n_cells}")
    L.need_device(who, xy, cell, keep, hint=_oracle_hint(who))
    dev = xy.device
    pts = xy.detach().to(torch.float64).contiguous()
    ids = cell.detach()
    if ids.dtype != torch.int32:                             # wider ids must not wrap: above the domain they stay above it
        ids = ids.clamp(min=-1, max=(1 << 31) - 1).to(torch.int32)
    ids = ids.contiguous()
    mask = None if keep is None else (keep.detach() != 0).to(torch.uint8).contiguous()
    if n_cells is None:
        n_cells = max(int(ids.max()) + 1, 1) if n else 1
    n_cells = min(int(n_cells), (1 << 31) - 1)
    return dev, pts, ids, mask, n, n_cells


def _outputs(dev, n: int, n_cells: int, smoothing: int, n_counters: int):
    """the worst-case output arrays of a call: (capacity, ring_offsets, xy, cell_ids, n_transcripts, counters)"""
    cap = max(min(n, n_cells), 1)
    capacity = n << smoothing
    return (capacity, torch.zeros(cap + 1, dtype=torch.int64, device=dev), torch.empty(capacity, 2, dtype=torch.float64, device=dev),
            torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
            torch.zeros(n_counters, dtype=torch.int64, device=dev))


def _raise_for_rows(who: str, c: dict, n_cells: int) -> None:
    if c["n_bad_cell"] or c["n_non_finite"]:
        raise L.SeggerAmdError(f"{who}: {c['n_bad_cell']} kept rows have a cell id outside [0, {n_cells}) and "
                               f"{c['n_non_finite']} a NaN or infinite coordinate; they took part in nothing")


def _result(c: dict, capacity: int, ring_offsets, out, cell_ids, n_tx) -> Dict[str, Tensor]:
    K, V = c["n_kept"], c["n_vertices"]
    assert V <= capacity, (V, capacity)                      # h <= n for every cell
    verts = out[:V]
    if 4 * V < capacity:                                     # do not keep the worst-case allocation alive behind a small view
        verts = verts.clone()
    return {"ring_offsets": ring_offsets[:K + 1], "xy": verts, "cell_ids": cell_ids[:K], "n_transcripts": n_tx[:K],
            "n_dropped": c["n_present"] - K}


def _n_rows(who: str, n: int) -> int:
    if n > MAX_ROWS:
        raise ValueError(f"{who}: {n} rows: 2^31 - 1 rows or more (the row index is half of the sort key)")
    return n


def segmentation_boundaries(result: Dict[str, Tensor], xy: Tensor, n_cells: Optional[int] = None, **kw) -> Dict[str, Tensor]:
    """:func:`cell_boundaries` of the segmented transcripts of ``result`` (what ``assign_transcripts_to_cells`` or
    ``SegmentationAccumulator.segmentation()`` returns).  ``xy`` is ``[n_transcripts_of_the_slide, 2]``, indexed by
    ``row_index``; ``kw`` is ``smoothing`` and ``method``.

    A transcript is counted iff ``cell_encoding >= 0`` and ``similarity >= similarity_threshold`` (NaN on either side: not
    counted; equality: counted) -- exactly the rows :func:`segger_amd.postprocess.expression_matrix` counts, the
    reference's ``writer.py:97-99``.  The reference's ``_load_assigned`` (``cli/export.py:47-95``) applies the same rule by
    default -- ``segger_cell_id`` not null and ``segger_similarity >= similarity_threshold``, a null on either side failing
    the comparison -- but then ALSO drops every cell with fewer than ``min_transcripts`` (default 10) kept transcripts,
    and offers ``--include-all-transcripts`` and ``--min-similarity`` instead of the per-gene threshold.  None of the
    three is applied here: filter the returned ``n_transcripts`` for the first, pass your own mask to
    :func:`cell_boundaries` for the others."""
    return _segmented("segmentation_boundaries", cell_boundaries, result, xy, n_cells, kw)


def _segmented(who: str, fn, result, xy, n_cells, kw) -> Dict[str, Tensor]:
    cols = [result[k] for k in ("row_index", "cell_encoding", "similarity", "similarity_threshold")]
    L.need_device(who, *cols, hint=_oracle_hint(who))
    n = int(cols[0].numel())
    if any(int(t.numel()) != n for t in cols):
        raise ValueError(f"{who}: columns of different lengths")
    if not isinstance(xy, Tensor) or xy.dim() != 2 or xy.shape[1] != 2:
        raise ValueError(f"{who}: xy is a floating-point [n_transcripts, 2] tensor")
    dev = cols[0].device
    keep = cols[2].to(torch.float32).double() >= cols[3].double()          # false when either side is NaN
    pts = xy.detach().to(device=dev)[cols[0].to(dev)]                      # the gather by row_index is plumbing
    return fn(pts, cols[1], n_cells, keep=keep, **kw)


def cell_outlines(xy: Tensor, cell: Tensor, n_cells: Optional[int] = None, *, keep: Optional[Tensor] = None,
                  connectivity: float = 2.0, smoothing: int = 0, large_cells: str = "refuse",
                  _lds_max_points: Optional[int] = None) -> Dict[str, Tensor]:
    """The concave outline of every cell: the reference's DEFAULT ``method="delaunay"`` (``_CellOutline``,
    ``boundary.py:57-154``) -- triangulate the cell's distinct transcripts, peel off the rim every triangle with a rim edge
    longer than ``2 * connectivity * d_max``, then every one with a rim edge that is long and faces an obtuse angle or
    faces an angle above ``180 - 11.25 / connectivity`` degrees, and return the outline of the largest piece that remains,
    after ``smoothing`` Chaikin iterations.  ``d_max`` is the cell's largest nearest-neighbour distance.

    The arguments, the counted rows and the returned dict (``ring_offsets``, ``xy``, ``cell_ids``, ``n_transcripts``,
    ``n_dropped``) are :func:`cell_boundaries`'s; ``connectivity`` is a finite number > 0.  A ring is open,
    counter-clockwise from its lowest (x, then y) vertex, and lists every vertex of the outline, collinear ones included;
    a vertex is an input coordinate bit for bit.  ``n_dropped`` counts the present cells without a polygon: fewer than 3
    distinct points, all collinear, or every triangle peeled.  One wait for the device.

    What the ring is, and why it does not depend on the order in which the reference's ``_prune`` visits its edges:
    DESIGN 3.5j.  What is NOT reproduced: the choice among components of EQUAL area (GEOS's order there; here the one
    with the lower lowest vertex); qhull's choice among co-circular points (here the fan from their lowest vertex);
    ``.buffer(0)`` after the smoothing, which can alter a smoothed concave ring that touches itself; and the orientation
    and start vertex shapely hands to ``_chaikin`` -- the smoothed vertices have the same bits either way, since a vertex
    is ``0.75 p + 0.25 q`` of an edge ``p q`` whichever way the ring runs, only their order differs.

    UNVERIFIED, as in this module's header: not verified against shapely, so ``polygonize`` (one polygon per
    edge-connected piece, dangling edges ignored) rests on knowledge of the library.  The pruning itself is pinned to a
    run of the reference's ``_CellOutline.refine`` (tests/golden/outlines_small.npz).

    ``large_cells`` says what happens to a cell with more than ``SEGGER_OUTLINE_MAX_POINTS`` = 2048 distinct points, the
    LDS budget of one cell.  ``"refuse"`` (the default): the call raises and names the cell.  ``"global"``: such a cell
    takes the route through global memory (``segger_cell_outlines_large``, csrc/outlines_large.hip: one workgroup per
    cell, its state in a slice of the workspace, 175 bytes per row of the cell) and gets the ring it would get from the
    LDS route, bit for bit; the call then costs one more wait for the device (a ``bincount`` sizes the slices by the rows
    of the cells with more than 2048 kept rows), and such a cell takes far longer than a small one -- README has the
    figures.  Still refused under ``"global"``: a single cell of more than 2^28 rows.  ``_lds_max_points`` (tests and
    timing only) lowers the threshold; 0 sends every cell through global memory.

    Raises ``ValueError`` for bad shapes, dtypes or options and ``SeggerAmdError`` for a kept row with a cell id
    ``>= n_cells`` or a non-finite coordinate, for a cell that was refused as above (the cell is named), and for a cell
    whose triangulation contradicted itself (rounded predicates on coordinates that share no grid can do that; the cell
    is named)."""
    who = "cell_outlines"
    smoothing = _check_smoothing(who, smoothing)
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, float)) or not 0 < connectivity < float("inf"):
        raise ValueError(f"{who}: connectivity must be a finite number > 0, got {connectivity!r}")
    if large_cells not in LARGE_CELLS:
        raise ValueError(f"{who}: large_cells {large_cells!r} is neither 'refuse' nor 'global'")
    if _lds_max_points is None:
        _lds_max_points = L.OUTLINE_MAX_POINTS
    if (isinstance(_lds_max_points, bool) or not isinstance(_lds_max_points, int) or not 0 <= _lds_max_points <= L.OUTLINE_MAX_POINTS
            or (large_cells == "refuse" and _lds_max_points != L.OUTLINE_MAX_POINTS)):
        raise ValueError(f"{who}: _lds_max_points must be an int in 0 .. {L.OUTLINE_MAX_POINTS}, and {L.OUTLINE_MAX_POINTS} unless "
                         f"large_cells='global', got {_lds_max_points!r}")
    dev, pts, ids, mask, n, n_cells = _rows(who, xy, cell, n_cells, keep)
    to_global = large_cells == "global"
    names = LARGE_OUTLINE_COUNTER_NAMES if to_global else OUTLINE_COUNTER_NAMES
    capacity, ring_offsets, out, cell_ids, n_tx, counters = _outputs(dev, n, n_cells, smoothing, len(names))
    if n and to_global:
        # the rows of the cells that can leave the LDS routes: plumbing, and one more wait for the device
        ok = (ids >= 0) & (ids < n_cells) if mask is None else (ids >= 0) & (ids < n_cells) & (mask != 0)
        per_cell = torch.bincount(ids[ok].long(), minlength=1)
        large_rows = int(per_cell[per_cell > _lds_max_points].sum())
        ws, ws_bytes = L.workspace("segger_cell_outlines_large_workspace_bytes", dev, n, n_cells, large_rows)
        L.call("segger_cell_outlines_large", dev, pts.data_ptr(), ids.data_ptr(), L.ptr(mask), n, n_cells, float(connectivity),
               smoothing, ring_offsets.data_ptr(), out.data_ptr(), capacity, cell_ids.data_ptr(), n_tx.data_ptr(),
               counters.data_ptr(), ws.data_ptr(), ws_bytes, _lds_max_points, large_rows)
        del ws
    elif n:
        ws, ws_bytes = L.workspace("segger_cell_outlines_workspace_bytes", dev, n, n_cells)
        L.call("segger_cell_outlines", dev, pts.data_ptr(), ids.data_ptr(), L.ptr(mask), n, n_cells, float(connectivity), smoothing,
               ring_offsets.data_ptr(), out.data_ptr(), capacity, cell_ids.data_ptr(), n_tx.data_ptr(), counters.data_ptr(),
               ws.data_ptr(), ws_bytes)
        del ws
    c = dict(zip(names, counters.tolist()))                       # the one wait for the device
    _raise_for_rows(who, c, n_cells)
    if c["n_refused"] and to_global:
        raise L.SeggerAmdError(f"{who}: {c['n_refused']} cells were refused by the global-memory route (a cell of more than 2^28 "
                               f"rows, or slices beyond the {large_rows} rows sized for), cell {c['refused_cell'] - 1} among them; "
                               f"such a cell gets no polygon")
    if c["n_refused"]:
        raise L.SeggerAmdError(f"{who}: {c['n_refused']} cells have more than {L.OUTLINE_MAX_POINTS} distinct points "
                               f"(SEGGER_OUTLINE_MAX_POINTS, the LDS budget of one cell), cell {c['refused_cell'] - 1} among "
                               f"them; such a cell gets no polygon")
    if c["n_failed"]:
        raise L.SeggerAmdError(f"{who}: the triangulation of {c['n_failed']} cells contradicted itself (rounded predicates), "
                               f"cell {c['failed_cell'] - 1} among them; such a cell gets no polygon")
    return _result(c, capacity, ring_offsets, out, cell_ids, n_tx)


def segmentation_outlines(result: Dict[str, Tensor], xy: Tensor, n_cells: Optional[int] = None, **kw) -> Dict[str, Tensor]:
    """:func:`cell_outlines` of the segmented transcripts of ``result``, chosen by the rule of
    :func:`segmentation_boundaries`; ``kw`` is ``connectivity``, ``smoothing`` and ``large_cells``."""
    return _segmented("segmentation_outlines", cell_outlines, result, xy, n_cells, kw)
