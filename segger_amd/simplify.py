"""Ring simplification and validity on the device: the two steps the reference's CosMx intake takes right after
``masks_to_contours`` (``src/segger/io/cosmx.py:94-96``)::

    tol = np.sqrt(fov_poly.area).mean() * TOL_FRAC      # TOL_FRAC = 1/50
    fov_poly.geometry = fov_poly.geometry.simplify(tolerance=tol)

-- GEOS's topology-preserving simplifier, per polygon -- and the ``is_valid`` that ``fix_invalid_geometry`` asks first
(``io/utils.py:127-136``; the Xenium intake asks it of every boundary file, ``io/preprocessor.py:472``).  Without the
simplification a ring from :func:`segger_amd.label_contours` keeps every direction change of its pixel chain, and every
consumer of the ring CSR (``polygon_props``, ``morphology_features``, ``points_in_polygons``) costs per vertex.

:func:`simplify_rings` is Douglas-Peucker over the closed vertex sequence with a guard: a section is flattened to its chord
only if the chord touches no input edge outside the section and no chord emitted before it (include/segger_amd.h has the
contract, DESIGN 3.5m the reasoning; csrc/simplify.hip the kernels).  :func:`rings_simple` is what ``is_valid`` asks of a
single-shell polygon.  :func:`contour_tolerance` is the reference's tolerance.  All three are checked against a sequential
float64 oracle and an exact integer one (tests/simplify_cases.py).

UNPINNED: neither shapely nor GEOS could be imported where this was written and the reference was never run.  GEOS's
simplifier has the same structure (farthest point; a candidate segment refused when it has an interior intersection with
input or output segments; depth-first recursion), but three of its details are not reproduced and may differ between GEOS
versions: its minimum-size rule at shallow depth, its optional removal of the ring's endpoint, and its "jump" check.
Downstream code accepts any start vertex.

What ``fix_invalid_geometry`` does next with the rings that are not simple, ``resort_coordinates``, is
:func:`segger_amd.repair.resort_rings`; :func:`segger_amd.repair.repair_rings` is the whole check / re-sort / check.

NOT BUILT: the ``buffer(0)`` repair, holes and multi-part polygons, rings above ``SEGGER_MORPH_MAX_VERTS`` (refused,
naming the polygon, as the other ring consumers do)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib as L
from .rings import raise_ring_errors, ring_csr

__all__ = ["simplify_rings", "rings_simple", "contour_tolerance", "COUNTER_NAMES"]

COUNTER_NAMES = ("n_vertices_in", "n_vertices_out", "n_sections", "n_refused", "n_passed_through", "n_restored", "longest_ring")
TOL_FRAC = 1.0 / 50.0
_ROUTES = {None: L.SIMPLIFY_SMALL_VERTS, "auto": L.SIMPLIFY_SMALL_VERTS, "large": 0}


def _small_max(who: str, route) -> int:
    try:
        return _ROUTES[route]
    except (KeyError, TypeError):
        raise ValueError(f"{who}: _route is None, 'auto' or 'large', got {route!r}") from None


def simplify_rings(ring_offsets: Tensor, xy: Tensor, tolerance: Union[float, Tensor], preserve_topology: bool = True, *,
                   _route: Optional[str] = None) -> Dict[str, Tensor]:
    """Simplify every ring of a CSR of polygons (``ring_offsets`` ``[P + 1]``, ``xy`` ``[V, 2]`` on the device, as
    ``polygon_props`` takes them) the way ``GeoSeries.simplify(tolerance, preserve_topology)`` does per polygon.

    ``tolerance`` is a float, a 0-dim tensor (one value for all; a device tensor, such as :func:`contour_tolerance` returns, is
    taken without a wait for the device) or a ``[P]`` tensor (one per polygon); finite and ``>= 0``.

    Returns ``ring_offsets`` ``[P + 1]`` int64 and ``xy`` ``[V', 2]`` float64 -- the kept vertices, the input's bytes, open
    rings --, ``vertex_index`` ``[V']`` int64, the row of the input ``xy`` each came from, and ``counters`` (int64,
    :data:`COUNTER_NAMES`: open vertices in, vertices out, sections visited, chords refused by the guard, rings passed
    through, rings restored after collapse, the longest output ring).

    What is kept, for a ring of ``n >= 3`` open vertices (a closing duplicate is dropped bit for bit): Douglas-Peucker over
    the closed sequence ``v0 .. v(n-1), v0``, depth first, left before right, in float64 on the ring translated to its first
    vertex.  A section ``(i, j)`` is flattened to its chord iff (a) its farthest interior vertex (squared distance to the
    closed segment, the lowest index among equals) is within ``tolerance`` and (b), with ``preserve_topology``, the chord
    touches no input edge outside the section and no chord emitted so far; otherwise it is split there.  Two segments touch
    when they share a point, unless that is a single point which is an endpoint of both.  Vertex 0 is always kept.  The
    guard keeps a ring from collapsing once the root is split (the chord back over an emitted chord is a touch);
    ``preserve_topology=False`` is the classical algorithm.  In either mode a ring that comes out with fewer than 3 vertices
    is returned as it went in and counted, and a ring of fewer than 3 open vertices passes through.

    UNPINNED against GEOS, which could not be run: its minimum-size rule at shallow depth, its optional removal of the ring's
    endpoint and its "jump" check are not reproduced (see the module's docstring).

    ``_route`` (tests and timing only): ``"large"`` sends every ring through the 4096-vertex LDS tier; the bytes are the same.

    Waits for the device twice (the longest ring; the counters, which size the result).  An empty CSR launches nothing.
    Raises ``ValueError`` for bad shapes, dtypes or tolerances, a ring above ``SEGGER_MORPH_MAX_VERTS`` (naming the polygon)
    or offsets the device found out of range, and ``SeggerAmdError`` for CPU tensors: there is no CPU fallback."""
    who = "simplify_rings"
    small_max = _small_max(who, _route)
    tol_value = None
    if isinstance(tolerance, Tensor):
        if not tolerance.is_floating_point() or tolerance.dim() > 1:
            raise ValueError(f"{who}: tolerance is a float, a 0-dim tensor or a floating-point [n_polygons] tensor")
        if tolerance.dim() == 0 and not tolerance.is_cuda:
            tol_value = float(tolerance)
    elif isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)):
        raise ValueError(f"{who}: tolerance is a float, a 0-dim tensor or a floating-point [n_polygons] tensor")
    else:
        tol_value = float(tolerance)
    if tol_value is not None and not (tol_value >= 0.0 and math.isfinite(tol_value)):
        raise ValueError(f"{who}: tolerance must be finite and >= 0, got {tol_value!r}")
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    if tol_value is None:
        if tolerance.dim() == 1 and tolerance.numel() != n_polygons:
            raise ValueError(f"{who}: tolerance has {tolerance.numel()} entries for {n_polygons} polygons")
        if tolerance.device != xy.device:
            raise ValueError(f"{who}: tolerance and xy are on different devices")
    L.need_device(who, ring_offsets, xy, hint="tests/simplify_cases.py holds the CPU oracle")
    dev = xy.device
    counters = torch.zeros(L.SIMPLIFY_COUNTERS, dtype=torch.int64, device=dev)
    if n_polygons == 0:
        return {"ring_offsets": torch.zeros(1, dtype=torch.int64, device=dev), "xy": torch.empty(0, 2, dtype=torch.float64, device=dev),
                "vertex_index": torch.empty(0, dtype=torch.int64, device=dev), "counters": counters[:len(COUNTER_NAMES)]}
    if tol_value is not None:
        tol = torch.full((1,), tol_value, dtype=torch.float64, device=dev)
    else:
        tol = tolerance.detach().to(torch.float64).reshape(-1).contiguous()
    stride = 1 if tol_value is None and tolerance.dim() == 1 else 0
    out_offsets = torch.empty(n_polygons + 1, dtype=torch.int64, device=dev)
    ws, ws_bytes = L.workspace("segger_simplify_rings_workspace_bytes", dev, n_polygons, n_vertices)
    L.call("segger_simplify_rings_mark", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, tol.data_ptr(), stride,
           int(bool(preserve_topology)), small_max, out_offsets.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes)
    c = counters.tolist()                                            # the wait for the device
    flag = c[len(COUNTER_NAMES)]
    if flag & L.SIMPLIFY_ERR_TOL:
        raise ValueError(f"{who}: tolerance must be finite and >= 0 for every polygon")
    raise_ring_errors(who, flag, ring_offsets, n_vertices)
    n_out = c[1]
    xy_out = torch.empty(n_out, 2, dtype=torch.float64, device=dev)
    vertex_index = torch.empty(n_out, dtype=torch.int64, device=dev)
    L.call("segger_simplify_rings_emit", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, out_offsets.data_ptr(),
           xy_out.data_ptr(), vertex_index.data_ptr(), n_out, ws.data_ptr(), ws_bytes)
    return {"ring_offsets": out_offsets, "xy": xy_out, "vertex_index": vertex_index, "counters": counters[:len(COUNTER_NAMES)]}


def rings_simple(ring_offsets: Tensor, xy: Tensor, *, _route: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """What ``is_valid`` asks of a single-shell polygon, for every ring of a CSR: ``(ok, reason)`` with ``ok`` ``[P]`` bool and
    ``reason`` ``[P, 3]`` int32 ``(code, i, j)``.

    A ring is simple iff at least 3 vertices are left when consecutive duplicates are dropped (otherwise code
    ``RING_TOO_FEW`` = 1, ``i = j = -1``) and no two of its edges touch (otherwise ``RING_TOUCH`` = 2 and the lowest pair
    ``i < j`` of touching edges in ``(i, j)`` order; edge ``k`` runs from open vertex ``k`` to ``k + 1``, the last one back to
    vertex 0).  ``RING_OK`` = 0 comes with ``i = j = -1``.  Two segments touch when they share a point, unless that is a single
    point which is an endpoint of both: adjacent edges may share their common endpoint, a fold-back is a touch.  By the same
    rule a ring that merely revisits a vertex (a contour through a one-pixel neck) without crossing or running along itself
    there is reported simple; GEOS is believed to call that a ring self-intersection (UNPINNED, it was not run).  Float64 on
    the ring translated to its first vertex; exact for coordinates that are integers below 2^25 in magnitude.  Holes and
    multi-part polygons are not represented in a ring CSR.

    Waits for the device twice (the longest ring, the error word).  Raises as :func:`simplify_rings` does."""
    who = "rings_simple"
    small_max = _small_max(who, _route)
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    L.need_device(who, ring_offsets, xy, hint="tests/simplify_cases.py holds the CPU oracle")
    dev = xy.device
    ok = torch.zeros(n_polygons, dtype=torch.uint8, device=dev)
    reason = torch.empty(n_polygons, 3, dtype=torch.int32, device=dev)
    if n_polygons > 0:
        ws, ws_bytes = L.workspace("segger_simplify_rings_workspace_bytes", dev, n_polygons, 0)
        L.call("segger_rings_simple", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, ok.data_ptr(),
               reason.data_ptr(), small_max, ws.data_ptr(), ws_bytes)
        raise_ring_errors(who, int(ws[:4].view(torch.int32)), ring_offsets, n_vertices)
    return ok.bool(), reason


def contour_tolerance(ring_offsets: Tensor, xy: Tensor, frac: float = TOL_FRAC) -> Tensor:
    """The reference's tolerance ``np.sqrt(fov_poly.area).mean() * TOL_FRAC`` (``cosmx.py:94``) for the rings of one call: the
    mean over the polygons of the square root of ``polygon_props``'s area, times ``frac``.  Plain torch on the device; a
    0-dim float64 device tensor, which :func:`simplify_rings` takes as it is.  ``nan`` for an empty CSR, as numpy's mean."""
    from .morphology import polygon_props
    if isinstance(frac, bool) or not isinstance(frac, (int, float)) or not (frac >= 0.0 and math.isfinite(frac)):
        raise ValueError(f"contour_tolerance: frac must be finite and >= 0, got {frac!r}")
    return polygon_props(ring_offsets, xy)["area"].sqrt().mean() * float(frac)
